"""``NextItNet`` / ``NextItNetEngine``: the dilated causal convolution sequence model (Yuan, Karatzoglou, Arapakis, Jose
and He, "A Simple Convolutional Generative Network for Next Item Recommendation", WSDM 2019) on libhiprec.so.

There is no counterpart in the reference; the paper and ``tests/nextitnet_torch.py`` (a restatement in plain torch ops)
are the specification, ``include/hiprec.h`` states the contract:

* items are ``1 .. n_items`` and 0 is padding (``item_emb.weight`` row 0 is zero and stays zero); sequences are
  ``[B, T]`` left-padded, the form ``data.SequenceSampler`` yields as ``(u, seq, pos, neg)`` -- ``neg`` is ignored;
* ``x_0 = item_emb[seq]``; ``R = len(dilations) * block_num`` residual blocks (the dilation list repeated ``block_num``
  times), each ``h = relu(LN(conv1(x)))`` at dilation ``d``, ``x' = relu(LN(conv2(h))) + x`` at ``2 d``, both causal with
  ``kernel_size`` taps; ``f = final_layer(x_R)``;
* the loss is the cross-entropy over items ``1 .. n_items`` against the tied table (no bias), the mean over the labelled
  rows: ``loss_positions = "all"`` (default, the paper's generative loss) labels every position with ``pos != 0``,
  ``"last"`` the last position of every sequence.  A batch without a label gives loss 0 and a zero gradient;
* ``l2`` is the optimizer's weight decay (``g += l2 * w`` on every element); it stands in for the published
  norm-regulariser on the convolution weights, which is not built.

Config keys under ``config["model"]``: ``n_items maxlen lr optimizer`` and, with defaults, ``emb_dim`` 64,
``kernel_size`` 3, ``dilations`` [1, 4], ``block_num`` 5, ``loss_positions`` "all", ``l2`` 0, ``n_users`` /
``batch_size`` (``train_an_epoch`` runs ``n_users // batch_size`` steps).  The constructor builds torch modules in
``state_dict()`` order (``Conv2d`` / ``Linear`` defaults, embedding normal(0, 0.01)), so one torch seed gives one model.

Forward, loss and backward run in ``csrc/nextitnet.hip`` (``final_layer`` through the grouped GEMM of ``csrc/ncf.hip``),
the optimizer is the shared dense sweep, ``recommend_next`` ranks the catalogue through ``csrc/topk.hip``.  There is no
CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor

MAX_DIM, MAX_LEN, MAX_KERNEL, MAX_BLOCKS = 128, 256, 4, 16      # kSeqMaxDim, kSeqMaxLen, kNinMax*
DEFAULTS = {"emb_dim": 64, "kernel_size": 3, "dilations": [1, 4], "block_num": 5, "loss_positions": "all", "l2": 0.0}
LOSS_POSITIONS = ("all", "last")


def _last_error(lib):
    return (lib.hiprec_last_error() or b"beyond the library's limits").decode()


def _get(cfg, key):
    return cfg[key] if key in cfg else DEFAULTS[key]


def _spec(n_items, D, k, R):
    spec = [("item_emb.weight", (n_items + 1, D))]
    for r in range(R):
        for c in ("1", "2"):
            spec += [(f"blocks.{r}.conv{c}.weight", (D, D, 1, k)), (f"blocks.{r}.conv{c}.bias", (D,)),
                     (f"blocks.{r}.ln{c}.weight", (D,)), (f"blocks.{r}.ln{c}.bias", (D,))]
    return spec + [("final_layer.weight", (D, D)), ("final_layer.bias", (D,))]


class _BlockParams(nn.Module):
    """One residual block's parameters as views of the flat buffer."""

    def __init__(self, v, r):
        super().__init__()
        for n in ("conv1", "ln1", "conv2", "ln2"):
            setattr(self, n, _ParamView(v[f"blocks.{r}.{n}.weight"], v[f"blocks.{r}.{n}.bias"]))


class NextItNet(_FlatModel):
    """The model: flat buffer in ``state_dict()`` order (``_spec``)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        m = config["model"]
        self.n_items, self.maxlen = int(m["n_items"]), int(m["maxlen"])
        self.emb_dim, self.kernel_size = int(_get(m, "emb_dim")), int(_get(m, "kernel_size"))
        self.block_dilations = [int(d) for d in _get(m, "dilations")] * int(_get(m, "block_num"))
        self.loss_positions, self.l2 = _get(m, "loss_positions"), float(_get(m, "l2"))
        if self.loss_positions not in LOSS_POSITIONS:
            raise ValueError(f"loss_positions must be one of {LOSS_POSITIONS}, got {self.loss_positions!r}")
        if self.l2 < 0.0:
            raise ValueError("l2 must be >= 0")
        D, k, R = self.emb_dim, self.kernel_size, len(self.block_dilations)
        if not 1 <= R <= MAX_BLOCKS:
            raise ValueError(f"len(dilations) * block_num must be in 1..{MAX_BLOCKS}, got {R}")
        if any(not 1 <= d < 2 ** 31 for d in self.block_dilations):
            raise ValueError("every dilation must be >= 1")
        self.shape = _lib.NextItNetShape(self.n_items, D, k, R, self.maxlen, LOSS_POSITIONS.index(self.loss_positions), 0,
                                         (ctypes.c_int32 * 16)(*self.block_dilations))
        lib = _lib.load()
        if lib.hiprec_nextitnet_param_floats(ctypes.byref(self.shape)) < 0:      # the limits live in csrc/nextitnet.hip
            raise ValueError(_last_error(lib))
        v = self._build(_spec(self.n_items, D, k, R))
        # torch modules in state_dict() order, for the RNG order: one torch seed gives one model
        mods = {"item_emb": nn.Embedding(self.n_items + 1, D, padding_idx=0)}
        with torch.no_grad():
            mods["item_emb"].weight.normal_(0, 0.01)
            mods["item_emb"].weight[0].zero_()
        for r in range(R):
            for c in ("1", "2"):
                mods[f"blocks.{r}.conv{c}"] = nn.Conv2d(D, D, (1, k))
                mods[f"blocks.{r}.ln{c}"] = nn.LayerNorm(D, eps=1e-8)
        mods["final_layer"] = nn.Linear(D, D)
        with torch.no_grad():
            for name, view in v.items():
                mod, attr = name.rsplit(".", 1)
                view.copy_(getattr(mods[mod], attr).data)
        self.item_emb = _ParamView(v["item_emb.weight"])
        self.blocks = nn.ModuleList(_BlockParams(v, r) for r in range(R))
        self.final_layer = _ParamView(v["final_layer.weight"], v["final_layer.bias"])
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, seq_len):
        need = lib.hiprec_nextitnet_workspace_bytes(ctypes.byref(self.shape), int(batch), int(seq_len))
        if need == 0:
            raise ValueError(f"unsupported batch {batch} x sequence length {seq_len} (maxlen {self.maxlen}, batch x "
                             "length below 2^24)")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def sequences(self, seqs):
        """``[B, T]`` ids (numpy, list or tensor) as ``(flat int64 device tensor, B, T)``."""
        shape = tuple(seqs.shape) if torch.is_tensor(seqs) else np.asarray(seqs).shape
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError("sequences must be [batch >= 1, length >= 1]")
        if shape[1] > self.maxlen:
            raise ValueError(f"sequence length {shape[1]} exceeds maxlen {self.maxlen}")
        return index_tensor(seqs, self._flat.device), int(shape[0]), int(shape[1])

    def feats(self, seqs):
        """The eval forward: ``f`` at the last position of every sequence, ``[B, D]`` on the device."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, B, T = self.sequences(seqs)
        stats = self._device_stats()
        out = torch.empty((B, self.emb_dim), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, T)
        _lib.check(lib.hiprec_nextitnet_feats(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(seq_t), B, T,
                                              _lib.ptr(out), _lib.ptr(stats), _lib.ptr(ws), ws.numel(),
                                              _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def predict(self, seqs, item_indices):
        """``[B, K]`` scores of the last position against the rows of ``item_indices`` (1-D, ids in ``0 .. n_items``)
        through the exact-fp32 MFMA GEMM."""
        if np.ndim(item_indices.cpu() if torch.is_tensor(item_indices) else item_indices) != 1:
            raise ValueError("item_indices must be 1-D: one list of candidate items for every sequence")
        f = self.feats(seqs)
        lib, dev = _lib.load(), self._flat.device
        idx = index_tensor(item_indices, dev)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) > self.n_items):
            raise IndexError(f"item id outside [0, {self.n_items}]")
        rows = self.item_emb.weight.data[idx].contiguous()
        B, D, K = f.shape[0], self.emb_dim, idx.numel()
        scores = torch.empty((B, K), dtype=torch.float32, device=dev)
        if K:
            _lib.check(lib.hiprec_gemm_f32(0, B, K, D, _lib.ptr(f), D, _lib.ptr(rows), D, _lib.ptr(scores), K, None, 0,
                                           None, 0, _lib.stream_ptr(dev)))
        return scores


class NextItNetEngine(FlatModelEngine):
    """Training and inference around ``NextItNet``."""

    def __init__(self, config):
        self.config = config
        self.model = NextItNet(config)
        m = config["model"]
        self.num_batch = max(1, int(m["n_users"]) // int(m["batch_size"])) if "n_users" in m and "batch_size" in m else 1
        super(NextItNetEngine, self).__init__(config)

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_nextitnet_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat NextItNet buffer is not laid out as libhiprec.so expects; rebuild the library")

    # ---- the step ----------------------------------------------------------------------------------------------
    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 4:
            raise ValueError("a NextItNet batch is (u, seq [B, T], pos [B, T], neg): u and neg are ignored")
        _, seq, pos, _ = batch_data
        seq_t, B, T = m.sequences(seq)
        pos_t = index_tensor(pos, dev)
        if pos_t.numel() != B * T:
            raise ValueError(f"pos must be [{B}, {T}] like seq")
        ws = m.workspace(lib, B, T)
        _lib.check(lib.hiprec_nextitnet_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), _lib.ptr(pos_t), B, T, m.l2,
            _lib.ptr(self._stats), _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)))

    def train_single_batch(self, batch_data, ratings=None):
        """One step on ``(u, seq, pos, neg)``: the loss (without the ``l2`` term)."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_grad(batch_data)
        self._enqueue_opt()
        return self._sync_stats().loss

    def train_an_epoch(self, sampler, epoch_id):
        """``n_users // batch_size`` calls of ``sampler.next_batch()``, the float losses summed (as ``SASRecEngine``)."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        total_loss = 0.0
        for _ in range(self.num_batch):
            u, seq, pos, neg = sampler.next_batch()
            total_loss += self.train_single_batch((np.array(u), np.array(seq), np.array(pos), np.array(neg)))
        print("[Training Epoch {}], Loss {}".format(epoch_id, total_loss))
        self.writer.add_scalar("model/loss", total_loss, epoch_id)
        return total_loss

    # ---- inference ---------------------------------------------------------------------------------------------
    def predict(self, seqs, item_indices):
        """Eval-mode scores ``[B, K]`` of the candidate list ``item_indices [K]`` for every sequence."""
        self.model.eval()
        return self.model.predict(seqs, item_indices)

    def recommend_next(self, seqs, k, seen=None):
        """The ``k`` best next items for every sequence of ``seqs [n, T]``: the last position's ``f`` against
        ``item_emb.weight[1:]`` through ``recommend.topk_factors``; ids are shifted back by one, so the padding id is
        never returned.  ``seen``: None, or a ``(rows, items)`` pair of equally long id columns -- row ``r`` is never
        recommended item ``i`` (0 entries are ignored).  Returns ``(items [n, k] int64, scores [n, k] fp32)`` on the
        device, ``-1`` / ``-inf`` in a tail with nothing left."""
        from .recommend import topk_factors

        self.model.eval()
        q = self.model.feats(seqs)
        n, dev = q.shape[0], q.device
        if seen is not None:
            rows, items = (index_tensor(x, dev) for x in seen)
            if rows.numel() != items.numel():
                raise ValueError("seen must be a (rows, items) pair of equally long id columns")
            keep = items != 0
            seen = (rows[keep], items[keep] - 1)
        items, scores = topk_factors(q, self.model.item_emb.weight.data[1:], 1.0, None, torch.arange(n, device=dev), k,
                                     seen)
        return torch.where(items >= 0, items + 1, items), scores
