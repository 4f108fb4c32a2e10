"""``Caser`` / ``CaserEngine``: the convolutional sequence embedding recommender (Tang and Wang, "Personalized Top-N
Sequential Recommendation via Convolutional Sequence Embedding", WSDM 2018) on libhiprec.so.

There is no counterpart in the reference; the paper and ``tests/caser_torch.py`` (a restatement in plain torch ops) are
the specification, ``include/hiprec.h`` states the contract:

* items are ``1 .. n_items`` and 0 is padding (``item_embeddings`` row 0 is zero and stays zero); users are
  ``0 .. n_users - 1``;
* the last ``L`` items of a user are an ``L x d`` image: ``n_v`` vertical filters (``[L, 1]``, no activation) and ``n_h``
  horizontal filters of every height ``1 .. L`` (``ac_conv``, max over time), dropout on their concatenation, ``fc1``
  with ``ac_fc``, and the user embedding next to it: ``x = [z | user]``; an item scores ``<x, W2[item]> + b2[item]``;
* the loss is binary cross-entropy on ``T`` next items against ``neg_samples`` sampled ones, each side its own mean over
  its real (non-zero) entries; ``l2`` is Adam's ``weight_decay``: ``g += l2 * w`` for every parameter element.

Config keys under ``config["model"]``: ``n_users n_items emb_dim L T neg_samples n_v n_h ac_conv ac_fc dropout_rate l2
lr optimizer batch_size``; ``ac_conv`` / ``ac_fc`` are each one of ``relu tanh sigm iden``.  Dropout follows the house
convention: ``dropout_rng`` is ``"torch_cpu"`` (default: ``torch.empty(B, n_v d + n_h L).bernoulli_(1 - p)``, so the torch
seed reproduces it) or ``"device"`` (``hiprec_edge_dropout_mask`` seeded by ``dropout_seed`` and the step count);
explicit ``keep_masks`` are accepted too.  The constructor builds torch modules in ``state_dict()`` order, so one torch
seed gives one model.

Forward, loss and backward run in ``csrc/caser.hip`` (``fc1`` through the grouped GEMM of ``csrc/ncf.hip``), the
optimizer is the shared dense sweep, ``recommend_next`` ranks the catalogue through ``csrc/topk.hip``.  There is no CPU
path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor

MAX_DIM, MAX_L, MAX_NV, MAX_NH, MAX_T, MAX_N = 128, 10, 16, 64, 16, 64
ACTIVATIONS = ("relu", "tanh", "sigm", "iden")      # HIPREC_CASER_AC_*


def _spec(n_users, n_items, d, L, n_v, n_h):
    spec = [("user_embeddings.weight", (n_users, d)), ("item_embeddings.weight", (n_items + 1, d)),
            ("conv_v.weight", (n_v, 1, L, 1)), ("conv_v.bias", (n_v,))]
    for i in range(L):
        spec += [(f"conv_h.{i}.weight", (n_h, 1, i + 1, d)), (f"conv_h.{i}.bias", (n_h,))]
    return spec + [("fc1.weight", (d, n_v * d + n_h * L)), ("fc1.bias", (d,)), ("W2.weight", (n_items + 1, 2 * d)),
                   ("b2.weight", (n_items + 1, 1))]


def _limit(name, value, hi):
    if not 1 <= value <= hi:
        raise ValueError(f"{name} must be in 1..{hi}, got {value}")


class Caser(_FlatModel):
    """The model: flat buffer in ``state_dict()`` order (``_spec``)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        m = config["model"]
        self.n_users, self.n_items = int(m["n_users"]), int(m["n_items"])
        self.emb_dim, self.L, self.T = int(m["emb_dim"]), int(m["L"]), int(m["T"])
        self.neg_samples, self.n_v, self.n_h = int(m["neg_samples"]), int(m["n_v"]), int(m["n_h"])
        self.dropout_rate, self.l2 = float(m["dropout_rate"]), float(m["l2"])
        if self.n_users < 1 or self.n_items < 1:
            raise ValueError("Caser needs n_users >= 1 and n_items >= 1")
        _limit("emb_dim", self.emb_dim, MAX_DIM)
        _limit("L", self.L, MAX_L)
        _limit("n_v", self.n_v, MAX_NV)
        _limit("n_h", self.n_h, MAX_NH)
        _limit("T", self.T, MAX_T)
        _limit("neg_samples", self.neg_samples, MAX_N)
        for key in ("ac_conv", "ac_fc"):
            if m[key] not in ACTIVATIONS:
                raise ValueError(f"{key} must be one of {ACTIVATIONS}, got {m[key]!r}")
        if not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
        if self.l2 < 0.0:
            raise ValueError("l2 must be >= 0")
        self.ac_conv, self.ac_fc = m["ac_conv"], m["ac_fc"]
        U, I, d, L, n_v, n_h = self.n_users, self.n_items, self.emb_dim, self.L, self.n_v, self.n_h
        self.n_features = n_v * d + n_h * L
        self.shape = _lib.CaserShape(U, I, d, L, self.T, self.neg_samples, n_v, n_h, ACTIVATIONS.index(self.ac_conv),
                                     ACTIVATIONS.index(self.ac_fc))
        v = self._build(_spec(U, I, d, L, n_v, n_h))
        # torch modules in state_dict() order, for the RNG order: one torch seed gives one model
        mods = {"user_embeddings": nn.Embedding(U, d), "item_embeddings": nn.Embedding(I + 1, d, padding_idx=0),
                "conv_v": nn.Conv2d(1, n_v, (L, 1))}
        for i in range(L):
            mods[f"conv_h.{i}"] = nn.Conv2d(1, n_h, (i + 1, d))
        mods["fc1"] = nn.Linear(self.n_features, d)
        mods["W2"] = nn.Embedding(I + 1, 2 * d, padding_idx=0)
        mods["b2"] = nn.Embedding(I + 1, 1, padding_idx=0)
        with torch.no_grad():
            mods["user_embeddings"].weight.normal_(0, 1.0 / d)
            mods["item_embeddings"].weight.normal_(0, 1.0 / d)
            mods["item_embeddings"].weight[0].zero_()
            mods["W2"].weight.normal_(0, 1.0 / (2 * d))
            mods["b2"].weight.zero_()
        for name, view in v.items():
            mod, attr = name.rsplit(".", 1)
            view.copy_(getattr(mods[mod], attr).data)
        self.user_embeddings = _ParamView(v["user_embeddings.weight"])
        self.item_embeddings = _ParamView(v["item_embeddings.weight"])
        self.conv_v = _ParamView(v["conv_v.weight"], v["conv_v.bias"])
        self.conv_h = nn.ModuleList(_ParamView(v[f"conv_h.{i}.weight"], v[f"conv_h.{i}.bias"]) for i in range(L))
        self.fc1 = _ParamView(v["fc1.weight"], v["fc1.bias"])
        self.W2 = _ParamView(v["W2.weight"])
        self.b2 = _ParamView(v["b2.weight"])
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch):
        need = lib.hiprec_caser_workspace_bytes(ctypes.byref(self.shape), int(batch))
        if need == 0:
            raise ValueError(f"unsupported batch of {batch} rows")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def batch_ids(self, seq, users):
        """``seq [B, L]`` and ``users [B]`` checked against each other: ``(seq_t, users_t, B)`` on the device."""
        shape = tuple(seq.shape) if torch.is_tensor(seq) else np.asarray(seq).shape
        if len(shape) != 2 or shape[0] < 1 or shape[1] != self.L:
            raise ValueError(f"seq must be [batch >= 1, L = {self.L}], got {shape}")
        dev = self._flat.device
        users_t = index_tensor(users, dev)
        if users_t.numel() != shape[0]:
            raise ValueError(f"{users_t.numel()} users for a batch of {shape[0]} sequences")
        return index_tensor(seq, dev), users_t, int(shape[0])

    def query(self, seq, users):
        """The eval-mode forward up to ``x = [z | user_embeddings[users]]``: ``[B, 2 d]`` on the device, with
        ``scores = x W2^T + b2``."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, users_t, B = self.batch_ids(seq, users)
        stats = self._device_stats()
        out = torch.empty((B, 2 * self.emb_dim), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B)
        _lib.check(lib.hiprec_caser_grad(
            ctypes.byref(self.shape), _lib.ptr(self._flat), None, _lib.ptr(seq_t), _lib.ptr(users_t), None, None, B, None,
            1.0, 0.0, _lib.ptr(out), _lib.ptr(stats), None, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def forward(self, seq, users, items, for_pred=False):
        """Scores of the candidate ``items`` (ids in ``1 .. n_items``) in eval mode (no dropout), without autograd:
        ``[B, K]`` for ``items [B, K]``; with ``for_pred`` one list ``items [K]`` serves every row."""
        x = self.query(seq, users)
        lib, dev = _lib.load(), self._flat.device
        B = x.shape[0]
        items_t = index_tensor(items, dev)
        if for_pred:
            items_t = items_t.repeat(B)
        if items_t.numel() == 0 or items_t.numel() % B:
            raise ValueError(f"{items_t.numel()} candidates do not fill a [batch = {B}, K] table")
        K = items_t.numel() // B
        stats = self._device_stats()
        scores = torch.empty((B, K), dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_caser_score(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(x), _lib.ptr(items_t),
                                          B, K, _lib.ptr(scores), _lib.ptr(stats), _lib.stream_ptr(dev)))
        self._check_status()
        return scores

    def item_factors(self):
        """``(W2[1:] [n_items, 2 d], b2[1:] [n_items])``: the item side of the score, without the padding row; views of
        the flat buffer."""
        return self.W2.weight.data[1:], self.b2.weight.data[1:, 0]


class CaserEngine(FlatModelEngine):
    """Training and inference around ``Caser``."""

    def __init__(self, config):
        self.config = config
        self.model = Caser(config)
        self._dropout_step = 0
        self.last_keep_masks = None
        super(CaserEngine, self).__init__(config)
        self._n_batches = 0

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_caser_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat Caser buffer is not laid out as libhiprec.so expects; rebuild the library")

    # ---- dropout ---------------------------------------------------------------------------------------------
    def _mask_shapes(self, B):
        return [(B, self.model.n_features)]

    def _keep_masks(self, B, keep_masks):
        """``[mask]``: the keep bytes of one step as a uint8 device tensor, or None (eval mode, rate 0)."""
        m = self.model
        p = m.dropout_rate
        if not m.training or p == 0.0:
            return None
        dev = m.flat.device
        shape = self._mask_shapes(B)[0]
        if keep_masks is not None:
            if len(keep_masks) != 1:
                raise ValueError(f"1 keep mask expected ([B, n_v d + n_h L]), got {len(keep_masks)}")
            k = keep_masks[0]
            t = torch.as_tensor(np.asarray(k.cpu() if torch.is_tensor(k) else k)).to(torch.uint8)
            if t.numel() != int(np.prod(shape)):
                raise ValueError(f"keep mask of {t.numel()} elements where {shape} is expected")
            return [t.reshape(-1).contiguous().to(dev)]
        cfg = self.config["model"]
        rng = cfg["dropout_rng"] if "dropout_rng" in cfg else "torch_cpu"
        self._dropout_step += 1
        if rng == "torch_cpu":
            return [torch.empty(shape).bernoulli_(1 - p).to(torch.uint8).reshape(-1).contiguous().to(dev)]
        if rng == "device":
            seed = int(cfg["dropout_seed"]) if "dropout_seed" in cfg else 0
            buf = torch.empty(int(np.prod(shape)), dtype=torch.uint8, device=dev)
            _lib.check(_lib.load().hiprec_edge_dropout_mask(_lib.ptr(buf), buf.numel(), 1.0 - p, seed * 64,
                                                            self._dropout_step, _lib.stream_ptr(dev)))
            return [buf]
        raise ValueError(f"unknown dropout_rng {rng!r}: 'torch_cpu' or 'device'")

    # ---- the step ----------------------------------------------------------------------------------------------
    def _enqueue_grad(self, batch_data, keep_masks=None):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 4:
            raise ValueError("a Caser batch is (users [B], seq [B, L], pos [B, T], neg [B, N])")
        users, seq, pos, neg = batch_data
        seq_t, users_t, B = m.batch_ids(seq, users)
        pos_t, neg_t = index_tensor(pos, dev), index_tensor(neg, dev)
        if pos_t.numel() != B * m.T or neg_t.numel() != B * m.neg_samples:
            raise ValueError(f"pos must be [{B}, T = {m.T}] and neg [{B}, N = {m.neg_samples}]")
        keep = self.last_keep_masks = self._keep_masks(B, keep_masks)
        ws = m.workspace(lib, B)
        _lib.check(lib.hiprec_caser_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), _lib.ptr(users_t),
            _lib.ptr(pos_t), _lib.ptr(neg_t), B, None if keep is None else _lib.ptr(keep[0]), 1.0 / (1.0 - m.dropout_rate),
            m.l2, None, _lib.ptr(self._stats), _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)))

    def backward_only(self, batch_data, keep_masks=None):
        """zero_grad + forward + loss + backward (with the ``l2`` term) without the optimizer step: ``(loss, grads)``."""
        self._enqueue_grad(batch_data, keep_masks)
        st, grads = self._finish_backward_only()
        return st.loss, grads

    def train_single_batch(self, batch_data, ratings=None, keep_masks=None):
        """One step on ``(users, seq, pos, neg)``: the loss (without the ``l2`` term)."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_grad(batch_data, keep_masks)
        self._enqueue_opt()
        return self._sync_stats().loss

    def _epoch_step(self, batch):
        self._n_batches += 1
        self._enqueue_step(batch)

    def train_an_epoch(self, train_loader, epoch_id):
        """Every batch of the loader (``data.WindowSampler``) enqueued back to back with ONE host sync at the end;
        returns the mean of the per-batch losses and writes it to the writer."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._n_batches = 0
        st = self._run_epoch(train_loader)
        mean_loss = st.loss_sum / max(self._n_batches, 1)
        print("[Training Epoch {}], Loss {:.6f}".format(epoch_id, mean_loss))
        self.writer.add_scalar("model/loss", mean_loss, epoch_id)
        return mean_loss

    # ---- inference ---------------------------------------------------------------------------------------------
    def predict(self, seq, users, item_indices):
        """Eval-mode scores ``[B, K]`` of ``item_indices`` (``[K]``: one list for every row, or ``[B, K]``)."""
        self.model.eval()
        one_list = np.ndim(item_indices.cpu() if torch.is_tensor(item_indices) else item_indices) == 1
        return self.model.forward(seq, users, item_indices, for_pred=one_list)

    def recommend_next(self, histories, users, k, seen=None):
        """The ``k`` best next items for every ``(history, user)`` pair, the whole catalogue ranked in one call:
        ``query`` against ``W2[1:]`` with ``b2[1:]`` as the item bias through ``recommend.topk_factors``; ids are shifted
        back by one, so the padding id is never returned.  ``histories``: a ragged list of id lists (the last ``L`` items
        count, shorter ones are left-padded) or a ``[n, L]`` array.  ``seen``: None, or a ``(rows, items)`` pair of
        equally long id columns -- row ``r`` is never recommended item ``i`` (ids as the model knows them; 0 entries are
        ignored).  Returns ``(items [n, k] int64, scores [n, k] fp32)`` on the device, ``-1`` / ``-inf`` in a tail with
        nothing left."""
        from .data import last_window
        from .recommend import topk_factors

        self.model.eval()
        if not (isinstance(histories, np.ndarray) and histories.ndim == 2) and not torch.is_tensor(histories):
            histories = last_window(histories, self.model.L)
        q = self.model.query(histories, users)
        n, dev = q.shape[0], q.device
        table, bias = self.model.item_factors()
        if seen is not None:
            rows, items = (index_tensor(x, dev) for x in seen)
            if rows.numel() != items.numel():
                raise ValueError("seen must be a (rows, items) pair of equally long id columns")
            if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
                raise ValueError(f"seen: a row outside [0, {n})")
            if items.numel() and (int(items.min()) < 0 or int(items.max()) > self.model.n_items):
                raise ValueError(f"seen: an item outside [0, {self.model.n_items}]")
            keep = items != 0
            seen = (rows[keep], items[keep] - 1)
        items, scores = topk_factors(q, table, 1.0, bias, torch.arange(n, device=dev), k, seen)
        return torch.where(items >= 0, items + 1, items), scores
