"""``FMLPRec`` / ``FMLPRecEngine``: the filter-enhanced all-MLP sequence model (Zhou, Yu, Zhao and Wen, "Filter-enhanced
MLP is All You Need for Sequential Recommendation", WWW 2022) on libhiprec.so.

There is no counterpart in the reference; the paper and ``tests/fmlprec_torch.py`` (a restatement in plain torch ops with
``torch.fft``) are the specification, ``include/hiprec.h`` states the contract:

* items are ``1 .. n_items`` and 0 is padding (``item_emb.weight`` row 0 is zero and stays zero); a batch is
  ``(u, seq [B, L <= maxlen], pos [B], neg [B])``; ``seq`` is left-padded with 0 to ``maxlen`` here, because the filter
  has ``maxlen // 2 + 1`` frequency bins; ``u`` is ignored;
* ``x = drop(LN(item_emb[seq] + pos_emb[t]))`` (padded positions carry ``pos_emb[t]``, as published); per block
  ``h = LN(x + drop(filter(x)))``, ``x = LN(h + drop(fc2(gelu(fc1(h)))))`` with
  ``filter(x) = irfft(rfft(x) * complex_weight)`` along the positions; ``f`` is ``x`` at the last position;
* the loss is ``mean(softplus(-<f, E[pos]>) + softplus(<f, E[neg]>))`` over the rows with ``pos != 0``; a batch without
  one gives loss 0 and a zero gradient.  There is no regulariser.

Config keys under ``config["model"]``: ``n_users n_items emb_dim maxlen num_blocks dropout_rate batch_size optimizer lr``
and, optional, ``ffn_dim`` (a multiple of 16 up to 512, default ``4 * emb_dim``), ``dropout_rng`` (``"device"``, the only
stream there is) and ``dropout_seed``.  ``train_single_batch(batch, keep_masks=[...])`` takes the ``1 + 2 * num_blocks``
keep masks explicitly, each ``[B, maxlen, emb_dim]``: embedding, then per block the filter's and the feed-forward's output.

The filter runs in ``csrc/fmlprec.hip`` as two dense exact-fp32 MFMA products against a table of ``maxlen`` cosines and
sines held in LDS; the spectrum never reaches memory.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._seqrec import MAX_DIM, MAX_LEN, _SeqEngine, _SeqModel
from .flat_engine import _ParamView, index_tensor

MAX_BLOCKS, MAX_FFN = 16, 512


def twiddle_table(seq_len, device):
    """``[seq_len, 2]`` (cos, sin) of ``2 pi j / seq_len`` as the kernels read it: evaluated in double by the library."""
    host = np.empty((int(seq_len), 2), dtype=np.float32)
    _lib.check(_lib.load().hiprec_fmlprec_twiddle(int(seq_len), host.ctypes.data))
    return torch.from_numpy(host).to(device)


def spec(n_items, maxlen, D, nb, H):
    """``(name, shape)`` of every parameter in ``state_dict()`` order: the layout of the flat buffer."""
    s = [("item_emb.weight", (n_items + 1, D)), ("pos_emb.weight", (maxlen, D)), ("emb_norm.weight", (D,)),
         ("emb_norm.bias", (D,))]
    for b in range(nb):
        p = f"blocks.{b}."
        s += [(p + "filter.complex_weight", (maxlen // 2 + 1, D, 2)), (p + "norm1.weight", (D,)), (p + "norm1.bias", (D,)),
              (p + "fc1.weight", (H, D)), (p + "fc1.bias", (H,)), (p + "fc2.weight", (D, H)), (p + "fc2.bias", (D,)),
              (p + "norm2.weight", (D,)), (p + "norm2.bias", (D,))]
    return s


class _FilterParams(nn.Module):
    def __init__(self, w):
        super().__init__()
        self.complex_weight = nn.Parameter(w, requires_grad=False)


class _BlockParams(nn.Module):
    """One block's parameters as views of the flat buffer, registered in its order."""

    def __init__(self, v, b):
        super().__init__()
        p = f"blocks.{b}."
        self.filter = _FilterParams(v[p + "filter.complex_weight"])
        for n in ("norm1", "fc1", "fc2", "norm2"):
            setattr(self, n, _ParamView(v[p + n + ".weight"], v[p + n + ".bias"]))


class FMLPRec(_SeqModel):
    """Flat buffer in ``state_dict()`` order (``spec``).  Normal(0, 0.02) tables, Linear weights and filter weights, zero
    biases, unit LayerNorm weights; the padding row is zero."""

    _PARAM_FLOATS = "hiprec_fmlprec_param_floats"

    def __init__(self, config):
        super().__init__()
        self._configure(config)
        D, T, nb, H, n_items = self.hidden_units, self.maxlen, self.num_blocks, self.ffn_dim, self.item_num
        v = self._build(spec(n_items, T, D, nb, H))
        for name, view in v.items():
            if name.endswith("bias"):
                continue
            if "norm" in name:
                view.fill_(1.0)
            elif name.endswith("complex_weight"):
                view.copy_(torch.randn(view.shape) * 0.02)
            else:
                view.normal_(0.0, 0.02)
        v["item_emb.weight"][0].zero_()
        self.item_emb = _ParamView(v["item_emb.weight"])
        self.pos_emb = _ParamView(v["pos_emb.weight"])
        self.emb_norm = _ParamView(v["emb_norm.weight"], v["emb_norm.bias"])
        self.blocks = nn.ModuleList(_BlockParams(v, b) for b in range(nb))
        self._twiddle = None

    def _configure(self, config):
        """The model's own keys (no heads, no regulariser); the limits are csrc/fmlprec.hip's."""
        self.config = config
        self.user_num = config.get("n_users")
        self.item_num = int(config["n_items"])
        self.hidden_units = int(config["emb_dim"])
        self.maxlen = int(config["maxlen"])
        self.num_blocks = int(config["num_blocks"])
        self.dropout_rate = float(config.get("dropout_rate", 0.0))
        self.batch_size = config.get("batch_size")
        self.ffn_dim = int(config["ffn_dim"]) if config.get("ffn_dim") is not None else 4 * self.hidden_units
        if not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
        D = self.hidden_units
        if D % 16 or not 16 <= D <= MAX_DIM:
            raise ValueError(f"emb_dim must be a multiple of 16 in 16..{MAX_DIM}, got {D}")
        if not 1 <= self.maxlen <= MAX_LEN:
            raise ValueError(f"maxlen must be in 1..{MAX_LEN}, got {self.maxlen}")
        if not 1 <= self.num_blocks <= MAX_BLOCKS:
            raise ValueError(f"num_blocks must be in 1..{MAX_BLOCKS}, got {self.num_blocks}")
        self.shape = _lib.FmlprecShape(self.item_num, D, self.maxlen, self.num_blocks, self.ffn_dim)
        lib = _lib.load()
        if lib.hiprec_fmlprec_param_floats(ctypes.byref(self.shape)) < 0:      # n_items, ffn_dim: the library's text
            raise ValueError((lib.hiprec_last_error() or b"beyond the library's limits").decode())
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, seq_len=None):
        need = lib.hiprec_fmlprec_workspace_bytes(ctypes.byref(self.shape), int(batch))
        if need == 0:
            raise ValueError(f"unsupported batch {batch}: batch x maxlen {self.maxlen} must stay within 2^24")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def twiddle(self):
        """The table of ``maxlen``, made once per device and kept with the workspace."""
        if self._twiddle is None or self._twiddle.device != self._flat.device:
            self._twiddle = twiddle_table(self.maxlen, self._flat.device)
        return self._twiddle

    def sequences(self, seqs):
        """``[B, L <= maxlen]`` ids as ``(flat int64 device tensor [B * maxlen], B, maxlen)``, left-padded with 0."""
        flat, B, L = super().sequences(seqs)
        T = self.maxlen
        if L < T:
            flat = torch.nn.functional.pad(flat.view(B, L), (T - L, 0)).reshape(-1).contiguous()
        return flat, B, T

    def feats(self, seqs):
        """The eval forward: ``f`` at the last position of every sequence, ``[B, D]`` on the device."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, B, _ = self.sequences(seqs)
        stats = self._device_stats()
        out = torch.empty((B, self.hidden_units), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B)
        _lib.check(lib.hiprec_fmlprec_feats(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(seq_t), B,
                                            _lib.ptr(self.twiddle()), _lib.ptr(out), _lib.ptr(stats), _lib.ptr(ws),
                                            ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def predict(self, seqs, item_indices):
        """``[B, K]`` scores of ``f`` against the rows of ``item_indices`` (1-D, ids in ``0 .. n_items``)."""
        f = self.feats(seqs)
        return self._predict_from_feats(f.view(f.shape[0], 1, -1), item_indices)


def filter_stage(x, weight, keep=None, keep_scale=1.0, dy=None):
    """The filter stage alone (``hiprec_fmlprec_filter``) on device tensors ``x [B, T, D]`` and
    ``weight [T // 2 + 1, D, 2]``: ``y = keep(filter(x))`` and, with ``dy``, ``(y, dx, dw)``."""
    lib = _lib.load()
    dev = x.device
    B, T, D = (int(n) for n in x.shape)
    need = lib.hiprec_fmlprec_filter_scratch_floats(B, T, D)
    if need < 0 or tuple(weight.shape) != (T // 2 + 1, D, 2):
        raise ValueError("filter_stage: x [B, T <= 256, D a multiple of 16 up to 128], weight [T // 2 + 1, D, 2]")
    x, weight = x.contiguous().float(), weight.contiguous().float()
    tw = twiddle_table(T, dev)
    y = torch.empty_like(x)
    dx = dw = scratch = None
    if dy is not None:
        dy = dy.contiguous().float()
        dx, dw = torch.empty_like(x), torch.empty_like(weight)
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
    _lib.check(lib.hiprec_fmlprec_filter(
        _lib.ptr(x), _lib.ptr(weight), _lib.ptr(tw), None if keep is None else _lib.ptr(keep), float(keep_scale),
        None if dy is None else _lib.ptr(dy), B, T, D, _lib.ptr(y), None if dy is None else _lib.ptr(dx),
        None if dy is None else _lib.ptr(dw), None if dy is None else _lib.ptr(scratch), need if dy is not None else 0,
        _lib.stream_ptr(dev)))
    return y if dy is None else (y, dx, dw)


class FMLPRecEngine(_SeqEngine):
    """``train_single_batch((u, seq, pos, neg)) -> float``, ``backward_only``, ``train_an_epoch(sampler, epoch_id)``,
    ``predict``, ``recommend_next``; checkpoints through the flat-model base."""

    _N_FIXED_MASKS, _MASK_NAMES = 1, "embedding, then per block the filter's and the feed-forward's output"

    def __init__(self, config):
        self.config = config
        m = config["model"]
        if m.setdefault("dropout_rng", "device") != "device":
            raise ValueError("FMLPRec draws its dropout masks on the device: dropout_rng must be 'device'")
        self.model = FMLPRec(m)
        self.num_batch = max(1, int(m["n_users"]) // int(m["batch_size"])) if "n_users" in m and "batch_size" in m else 1
        self._dropout_step = 0
        super(FMLPRecEngine, self).__init__(config)

    def _mask_shapes(self, B, T):
        return [(B * T, self.model.hidden_units)] * (1 + 2 * self.model.num_blocks)

    def _enqueue_grad(self, batch_data, keep_masks=None):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 4:
            raise ValueError("an FMLPRec batch is (u, seq [B, L], pos [B], neg [B]): u is ignored")
        _, seq, pos, neg = batch_data
        seq_t, B, T = m.sequences(seq)
        pos_t, neg_t = index_tensor(pos, dev), index_tensor(neg, dev)
        if pos_t.numel() != B or neg_t.numel() != B:
            raise ValueError(f"pos and neg must be [{B}]: one label pair for the last position of every sequence")
        keep_arr = self._keep_array(B, T, keep_masks)
        ks = 1.0 / (1.0 - m.dropout_rate)
        ws = m.workspace(lib, B)
        _lib.check(lib.hiprec_fmlprec_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), _lib.ptr(pos_t),
            _lib.ptr(neg_t), B, _lib.ptr(m.twiddle()), keep_arr, ks, None, _lib.ptr(self._stats), _lib.ptr(self._scratch),
            self._scratch.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))

    def train_an_epoch(self, sampler, epoch_id):
        """``n_users // batch_size`` calls of ``sampler.next_batch()`` (``(u, seq, pos, neg)`` with ``pos`` / ``neg``
        ``[B, T]`` as ``data.SequenceSampler`` yields them, or ``[B]``): the last position's pair is the label."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        total_loss = 0.0
        for _ in range(self.num_batch):
            u, seq, pos, neg = (np.array(a) for a in sampler.next_batch())
            if pos.ndim == 2:
                pos, neg = pos[:, -1], neg[:, -1]
            total_loss += self.train_single_batch((u, seq, pos, neg))
        print("[Training Epoch {}], Loss {}".format(epoch_id, total_loss))
        self.writer.add_scalar("model/loss", total_loss, epoch_id)
        return total_loss

    # ---- inference ---------------------------------------------------------------------------------------------
    def predict(self, seqs, item_indices):
        """Eval-mode scores ``[B, K]`` of the candidate list ``item_indices [K]`` for every sequence."""
        self.model.eval()
        return self.model.predict(seqs, item_indices)

    def recommend_next(self, seqs, k, seen=None):
        """The ``k`` best next items for every sequence of ``seqs [n, L]``: ``f`` against ``item_emb.weight[1:]`` through
        ``recommend.topk_factors``; the padding id is never returned.  ``seen``: None, or a ``(rows, items)`` pair of
        equally long id columns -- row ``r`` is never recommended item ``i`` (0 entries are ignored).  Returns
        ``(items [n, k] int64, scores [n, k] fp32)`` on the device, ``-1`` / ``-inf`` in a tail with nothing left."""
        self.model.eval()
        f = self.model.feats(seqs)
        return self._recommend_from_feats(f.view(f.shape[0], 1, -1), k, seen)
