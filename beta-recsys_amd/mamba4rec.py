"""``Mamba4Rec`` / ``Mamba4RecEngine``: the selective state-space sequence model (Liu, Lin, Wang, Zhang, Yin and Liu,
"Mamba4Rec: Towards Efficient Sequential Recommendation with Selective State Space Models", 2024) on libhiprec.so.

There is no counterpart in the reference; the paper and ``tests/mamba4rec_torch.py`` (a restatement in plain torch ops with a
Python loop over the positions) are the specification, ``include/hiprec.h`` states the contract:

* items are ``1 .. n_items`` and 0 is padding (``item_emb.weight`` row 0 is zero and stays zero); a batch is
  ``(u, seq [B, L <= maxlen], pos [B], neg [B])``; ``seq`` is left-padded with 0 to ``maxlen``; ``u`` is ignored;
* ``x = LN(drop(item_emb[seq]))`` (no positional table); per layer ``h = LN(drop(Mamba(x * m)) + x)`` (without the
  residual when ``num_blocks == 1``, as published), ``x = LN(h + drop(fc2(drop(gelu(fc1(h))))))``; the scan holds its
  state and its output at 0 through the padded slots; ``f`` is ``x`` at the last slot;
* the loss is ``mean(softplus(-<f, E[pos]>) + softplus(<f, E[neg]>))`` over the rows with ``pos != 0``; a batch without
  one gives loss 0 and a zero gradient.  There is no regulariser (the paper's cross-entropy over the catalogue is not built).

Config keys under ``config["model"]``: ``n_users n_items emb_dim maxlen num_blocks`` (or ``num_layers``) ``dropout_rate
batch_size optimizer lr`` and, optional, ``d_state`` (32), ``d_conv`` (4), ``expand`` (2), ``dt_rank`` (``"auto"``:
``ceil(emb_dim / 16)``), ``ffn_dim`` (``4 * emb_dim``), ``dropout_rng`` (``"device"``, the only stream there is) and
``dropout_seed``.  ``train_single_batch(batch, keep_masks=[...])`` takes the ``1 + 3 * num_blocks`` keep masks explicitly:
embedding ``[B, maxlen, emb_dim]``, then per layer the Mamba output, the feed-forward's hidden ``[B, maxlen, ffn_dim]`` and
its output.

The selective scan runs in ``csrc/mamba4rec.hip`` with the positions in the lanes of a wave; no ``[B, T, d_inner, d_state]``
tensor exists.  There is no CPU path.
"""
import ctypes
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._seqrec import _SeqEngine, _SeqModel
from .flat_engine import _ParamView, index_tensor


def spec(n_items, D, nb, H, Di, N, Kc, R):
    """``(name, shape)`` of every parameter in ``state_dict()`` order: the layout of the flat buffer."""
    s = [("item_emb.weight", (n_items + 1, D)), ("emb_norm.weight", (D,)), ("emb_norm.bias", (D,))]
    for b in range(nb):
        p, m = f"layers.{b}.", f"layers.{b}.mamba."
        s += [(m + "in_proj.weight", (2 * Di, D)), (m + "conv1d.weight", (Di, 1, Kc)), (m + "conv1d.bias", (Di,)),
              (m + "x_proj.weight", (R + 2 * N, Di)), (m + "dt_proj.weight", (Di, R)), (m + "dt_proj.bias", (Di,)),
              (m + "A_log", (Di, N)), (m + "D", (Di,)), (m + "out_proj.weight", (D, Di)),
              (p + "norm1.weight", (D,)), (p + "norm1.bias", (D,)), (p + "fc1.weight", (H, D)), (p + "fc1.bias", (H,)),
              (p + "fc2.weight", (D, H)), (p + "fc2.bias", (D,)), (p + "norm2.weight", (D,)), (p + "norm2.bias", (D,))]
    return s


class _MambaParams(nn.Module):
    def __init__(self, v, m):
        super().__init__()
        self.in_proj = _ParamView(v[m + "in_proj.weight"])
        self.conv1d = _ParamView(v[m + "conv1d.weight"], v[m + "conv1d.bias"])
        self.x_proj = _ParamView(v[m + "x_proj.weight"])
        self.dt_proj = _ParamView(v[m + "dt_proj.weight"], v[m + "dt_proj.bias"])
        self.A_log = nn.Parameter(v[m + "A_log"], requires_grad=False)
        self.D = nn.Parameter(v[m + "D"], requires_grad=False)
        self.out_proj = _ParamView(v[m + "out_proj.weight"])


class _LayerParams(nn.Module):
    """One layer's parameters as views of the flat buffer, registered in its order."""

    def __init__(self, v, b):
        super().__init__()
        p = f"layers.{b}."
        self.mamba = _MambaParams(v, p + "mamba.")
        for n in ("norm1", "fc1", "fc2", "norm2"):
            setattr(self, n, _ParamView(v[p + n + ".weight"], v[p + n + ".bias"]))


class Mamba4Rec(_SeqModel):
    """Flat buffer in ``state_dict()`` order (``spec``).  ``A_log = log(1 .. N)`` per row, ``D = 1``, ``dt_proj.bias`` the
    inverse softplus of a log-uniform step in [1e-3, 1e-1], ``dt_proj.weight`` uniform in ``+-R^-0.5``; everything else
    Normal(0, 0.02), zero biases, unit LayerNorm weights; the padding row is zero."""

    _PARAM_FLOATS = "hiprec_mamba4rec_param_floats"

    def __init__(self, config):
        super().__init__()
        self._configure(config)
        D, nb, H, n_items = self.hidden_units, self.num_blocks, self.ffn_dim, self.item_num
        Di, N, R = self.d_inner, self.d_state, self.dt_rank
        v = self._build(spec(n_items, D, nb, H, Di, N, self.d_conv, R))
        for name, view in v.items():
            if name.endswith("A_log"):
                view.copy_(torch.log(torch.arange(1, N + 1, dtype=torch.float32)).expand(Di, N))
            elif name.endswith(".D"):
                view.fill_(1.0)
            elif name.endswith("dt_proj.weight"):
                view.uniform_(-R ** -0.5, R ** -0.5)
            elif name.endswith("dt_proj.bias"):
                dt = torch.exp(torch.rand(Di) * (math.log(1e-1) - math.log(1e-3)) + math.log(1e-3))
                view.copy_(dt + torch.log(-torch.expm1(-dt)))
            elif name.endswith("bias"):
                continue
            elif "norm" in name:
                view.fill_(1.0)
            else:
                view.normal_(0.0, 0.02)
        v["item_emb.weight"][0].zero_()
        self.item_emb = _ParamView(v["item_emb.weight"])
        self.emb_norm = _ParamView(v["emb_norm.weight"], v["emb_norm.bias"])
        self.layers = nn.ModuleList(_LayerParams(v, b) for b in range(nb))

    def _configure(self, config):
        """The model's own keys; every limit is csrc/mamba4rec.hip's and comes back in the library's words."""
        self.config = config
        self.user_num = config.get("n_users")
        self.item_num = int(config["n_items"])
        self.hidden_units = D = int(config["emb_dim"])
        self.maxlen = int(config["maxlen"])
        self.num_blocks = int(config["num_blocks"] if "num_blocks" in config else config["num_layers"])
        self.dropout_rate = float(config.get("dropout_rate", 0.0))
        self.batch_size = config.get("batch_size")
        self.ffn_dim = int(config["ffn_dim"]) if config.get("ffn_dim") is not None else 4 * D
        self.d_state = int(config.get("d_state", 32))
        self.d_conv = int(config.get("d_conv", 4))
        self.expand = int(config.get("expand", 2))
        rank = config.get("dt_rank", "auto")
        self.dt_rank = -(-D // 16) if rank == "auto" else int(rank)
        self.d_inner = self.expand * D
        if not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
        self.shape = _lib.Mamba4RecShape(self.item_num, D, self.maxlen, self.num_blocks, self.ffn_dim, self.d_state,
                                         self.d_conv, self.expand, self.dt_rank)
        lib = _lib.load()
        if lib.hiprec_mamba4rec_param_floats(ctypes.byref(self.shape)) < 0:
            raise ValueError((lib.hiprec_last_error() or b"beyond the library's limits").decode())
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, seq_len=None):
        need = lib.hiprec_mamba4rec_workspace_bytes(ctypes.byref(self.shape), int(batch))
        if need == 0:
            raise ValueError(f"unsupported batch {batch}: batch x maxlen {self.maxlen} must stay within 2^24")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def sequences(self, seqs):
        """``[B, L <= maxlen]`` ids as ``(flat int64 device tensor [B * maxlen], B, maxlen)``, left-padded with 0."""
        flat, B, L = super().sequences(seqs)
        T = self.maxlen
        if L < T:
            flat = torch.nn.functional.pad(flat.view(B, L), (T - L, 0)).reshape(-1).contiguous()
        return flat, B, T

    def feats(self, seqs):
        """The eval forward: ``f`` at the last slot of every sequence, ``[B, D]`` on the device."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, B, _ = self.sequences(seqs)
        stats = self._device_stats()
        out = torch.empty((B, self.hidden_units), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B)
        _lib.check(lib.hiprec_mamba4rec_feats(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(seq_t), B,
                                              _lib.ptr(out), _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def predict(self, seqs, item_indices):
        """``[B, K]`` scores of ``f`` against the rows of ``item_indices`` (1-D, ids in ``0 .. n_items``)."""
        f = self.feats(seqs)
        return self._predict_from_feats(f.view(f.shape[0], 1, -1), item_indices)


def selective_scan(u, dt_pre, z, A, Bm, Cm, D, start, dout=None):
    """The scan stage alone (``hiprec_mamba4rec_scan``) on device tensors ``u, dt_pre, z [B, T, d_inner]``,
    ``A [d_inner, N]``, ``Bm, Cm [B, T, N]``, ``D [d_inner]`` and ``start [B]`` (slots before ``start[b]`` are padding):
    ``out``, and with ``dout`` ``(out, du, d dt_pre, dz, dA, dBm, dCm, dD)``."""
    lib = _lib.load()
    dev = u.device
    B, T, Di = (int(n) for n in u.shape)
    N = int(A.shape[1])
    need = lib.hiprec_mamba4rec_scan_scratch_floats(B, T, Di, N)
    if need < 0 or tuple(A.shape) != (Di, N) or tuple(Bm.shape) != (B, T, N) or tuple(Cm.shape) != (B, T, N):
        raise ValueError("selective_scan: u [B, T <= 256, d_inner a multiple of 16 up to 256], A [d_inner, N <= 64], "
                         "Bm and Cm [B, T, N]")
    u, dt_pre, z, A, Bm, Cm, D = (t.contiguous().float() for t in (u, dt_pre, z, A, Bm, Cm, D))
    start = start.to(device=dev, dtype=torch.int32).contiguous()
    out = torch.empty_like(u)
    grads, scratch = [None] * 7, None
    if dout is not None:
        dout = dout.contiguous().float()
        grads = [torch.empty_like(t) for t in (u, dt_pre, z, A, Bm, Cm, D)]
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
    opt = lambda t: None if t is None else _lib.ptr(t)      # noqa: E731
    _lib.check(lib.hiprec_mamba4rec_scan(
        _lib.ptr(u), _lib.ptr(dt_pre), _lib.ptr(z), _lib.ptr(A), _lib.ptr(Bm), _lib.ptr(Cm), _lib.ptr(D), _lib.ptr(start),
        opt(dout), B, T, Di, N, _lib.ptr(out), *(opt(g) for g in grads), opt(scratch), need if dout is not None else 0,
        _lib.stream_ptr(dev)))
    return out if dout is None else (out, *grads)


class Mamba4RecEngine(_SeqEngine):
    """``train_single_batch((u, seq, pos, neg)) -> float``, ``backward_only``, ``train_an_epoch(sampler, epoch_id)``,
    ``predict``, ``recommend_next``; checkpoints through the flat-model base."""

    _N_FIXED_MASKS = 1
    _MASK_NAMES = "embedding, then per layer the Mamba output, the feed-forward's hidden and its output"

    def __init__(self, config):
        self.config = config
        m = config["model"]
        if m.setdefault("dropout_rng", "device") != "device":
            raise ValueError("Mamba4Rec draws its dropout masks on the device: dropout_rng must be 'device'")
        self.model = Mamba4Rec(m)
        self.num_batch = max(1, int(m["n_users"]) // int(m["batch_size"])) if "n_users" in m and "batch_size" in m else 1
        self._dropout_step = 0
        super(Mamba4RecEngine, self).__init__(config)

    def _mask_shapes(self, B, T):
        D, H = self.model.hidden_units, self.model.ffn_dim
        return [(B * T, D)] + [(B * T, D), (B * T, H), (B * T, D)] * self.model.num_blocks

    def _enqueue_grad(self, batch_data, keep_masks=None):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 4:
            raise ValueError("a Mamba4Rec batch is (u, seq [B, L], pos [B], neg [B]): u is ignored")
        _, seq, pos, neg = batch_data
        seq_t, B, T = m.sequences(seq)
        pos_t, neg_t = index_tensor(pos, dev), index_tensor(neg, dev)
        if pos_t.numel() != B or neg_t.numel() != B:
            raise ValueError(f"pos and neg must be [{B}]: one label pair for the last slot of every sequence")
        keep_arr = self._keep_array(B, T, keep_masks)
        ks = 1.0 / (1.0 - m.dropout_rate)
        ws = m.workspace(lib, B)
        _lib.check(lib.hiprec_mamba4rec_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), _lib.ptr(pos_t),
            _lib.ptr(neg_t), B, keep_arr, ks, None, _lib.ptr(self._stats), _lib.ptr(self._scratch), self._scratch.numel(),
            _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))

    def train_an_epoch(self, sampler, epoch_id):
        """``n_users // batch_size`` calls of ``sampler.next_batch()`` (``(u, seq, pos, neg)`` with ``pos`` / ``neg``
        ``[B, T]`` as ``data.SequenceSampler`` yields them, or ``[B]``): the last slot's pair is the label."""
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
        ``recommend.topk_factors``; the padding id is never returned.  ``seen`` as in ``FMLPRecEngine.recommend_next``.
        Returns ``(items [n, k] int64, scores [n, k] fp32)`` on the device, ``-1`` / ``-inf`` in a tail with nothing left."""
        self.model.eval()
        f = self.model.feats(seqs)
        return self._recommend_from_feats(f.view(f.shape[0], 1, -1), k, seen)
