"""``ALS`` / ``ALSEngine``: implicit-feedback matrix factorisation solved by alternating least squares (WRMF / iALS; Hu,
Koren and Volinsky, "Collaborative Filtering for Implicit Feedback Datasets", ICDM 2008) on libhiprec.so
(``csrc/als.hip``).  The reference has no counterpart: this model is an addition.

``r_ui`` is the number of times the pair (u, i) occurs in the training frame::

    p_ui = [r_ui > 0]        c_ui = 1 + alpha * r_ui
    L(X, Y) = sum over ALL (u, i) of c_ui (p_ui - x_u . y_i)^2  +  reg (|X|_F^2 + |Y|_F^2)

A half-sweep is the closed-form minimiser of ``L`` over one table with the other fixed: per row one ``[D, D]`` normal
equation, ``A_u = Y^T Y + reg I + sum_{i in N(u)} alpha r_ui y_i y_i^T``, ``b_u = sum_{i in N(u)} (1 + alpha r_ui) y_i``,
solved by a Cholesky factorisation in LDS.  There is no learning rate, no negative sampling and no float atomic; the loss
can only go down; a user who was not in the training frame gets a row from one solve (``fold_in``).

Config keys (``config["model"]`` of the engine): ``n_users n_items emb_dim device_str`` and optionally ``alpha`` (40.0,
>= 0), ``reg`` (0.1, > 0), ``stddev`` (0.01: the tables start N(0, stddev^2)), ``als_blocks`` (0 = the library's choice
of grid; the result does not depend on it).  ``state_dict`` keys: ``user_factors.weight``, ``item_factors.weight``.
There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .flat_engine import _FlatModel, _ParamView, index_tensor
from .knn import _frame_columns, build_interaction_csr
from .torch_engine import ModelEngine, make_writer

MAX_DIM = 128         # HIPREC_ALS_MAX_DIM
MAX_BLOCKS = 1024     # HIPREC_ALS_MAX_BLOCKS
NONE = (1 << 64) - 1  # hiprec_als_workspace_bytes for a bad shape


def longest_first(ptr):
    """The row order a half-sweep walks: longest row first, ties to the lower id (device int64)."""
    return torch.argsort(ptr[1:] - ptr[:-1], descending=True, stable=True).contiguous()


class ALS(_FlatModel):
    """The two factor tables and everything that reads them; ``ALSEngine`` owns the training frame and the sweeps."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.n_users, self.n_items = int(config["n_users"]), int(config["n_items"])
        self.emb_dim = int(config["emb_dim"])
        self.alpha = float(config["alpha"]) if "alpha" in config else 40.0
        self.reg = float(config["reg"]) if "reg" in config else 0.1
        self.stddev = float(config["stddev"]) if "stddev" in config else 0.01
        self.als_blocks = int(config["als_blocks"]) if "als_blocks" in config else 0
        if self.n_users < 1 or self.n_items < 1:
            raise ValueError("n_users and n_items must be >= 1")
        if not 1 <= self.emb_dim <= MAX_DIM:
            raise ValueError(f"emb_dim {self.emb_dim}: 1 .. {MAX_DIM} are supported")
        if not (self.alpha >= 0 and np.isfinite(self.alpha)):
            raise ValueError(f"alpha {self.alpha}: must be finite and >= 0")
        if not (self.reg > 0 and np.isfinite(self.reg)):
            raise ValueError(f"reg {self.reg}: must be finite and > 0 (it keeps every normal equation positive definite)")
        if not (self.stddev >= 0 and np.isfinite(self.stddev)):
            raise ValueError(f"stddev {self.stddev}: must be finite and >= 0")
        if not 0 <= self.als_blocks <= MAX_BLOCKS:
            raise ValueError(f"als_blocks {self.als_blocks}: 0 (the library's choice) .. {MAX_BLOCKS}")
        D = self.emb_dim
        v = self._build([("user_factors.weight", (self.n_users, D)), ("item_factors.weight", (self.n_items, D))])
        nn.init.normal_(v["user_factors.weight"], mean=0.0, std=self.stddev)
        nn.init.normal_(v["item_factors.weight"], mean=0.0, std=self.stddev)
        self.user_factors = _ParamView(v["user_factors.weight"])
        self.item_factors = _ParamView(v["item_factors.weight"])
        self._ws = None
        self.device = torch.device(config["device_str"])
        if self.device.type == "cuda" and torch.cuda.is_available():
            self.to(self.device)           # (elsewhere the tables stay on the host and every call raises RuntimeError)

    # ---- device buffers ---------------------------------------------------------------------------
    def _als_buffers(self):
        """Workspace, the two ``[D, D]`` Gram matrices, the failed-pivot counter and the loss pair on the tables' device."""
        lib = self._require_hip()
        dev = self._flat.device
        if self._ws is None or self._ws["dev"] != dev:
            need = lib.hiprec_als_workspace_bytes(self.n_users, self.n_items, self.emb_dim)
            if need == NONE:
                raise ValueError(f"bad shape (n_users={self.n_users}, n_items={self.n_items}, emb_dim={self.emb_dim})")
            D = self.emb_dim
            self._ws = {"dev": dev, "bytes": need,
                        "ws": torch.empty(max(need // 8, 1), dtype=torch.int64, device=dev),
                        "G": torch.zeros((D, D), dtype=torch.float32, device=dev),
                        "G_reg": torch.zeros((D, D), dtype=torch.float32, device=dev),
                        "failed": torch.zeros(1, dtype=torch.int32, device=dev),
                        "loss": torch.zeros(2, dtype=torch.float64, device=dev)}
        return self._ws

    def gram(self, table):
        """``(G, G + reg I)`` of ``table [n, D]`` (views of the model's buffers: the next call overwrites them)."""
        lib = self._require_hip()
        b = self._als_buffers()
        dev = self._flat.device
        _lib.check(lib.hiprec_als_gram(_lib.ptr(table), table.shape[0], self.emb_dim, self.reg, _lib.ptr(b["G"]),
                                       _lib.ptr(b["G_reg"]), _lib.ptr(b["ws"]), b["bytes"], _lib.stream_ptr(dev)))
        return b["G"], b["G_reg"]

    def solve_rows(self, csr, order, other, out):
        """One half-sweep of the rows of ``csr`` against the table ``other`` into ``out``: a Gram launch and a solve
        launch.  Raises ``FloatingPointError`` when a pivot failed (those rows of ``out`` are left as they were)."""
        lib = self._require_hip()
        b = self._als_buffers()
        dev = self._flat.device
        stats = self._device_stats()
        ptr, idx, val = csr
        n_rows = ptr.numel() - 1
        if idx.numel() == 0:                    # no interaction at all: every row is the empty row
            return out.zero_()
        _, g_reg = self.gram(other)
        b["failed"].zero_()
        _lib.check(lib.hiprec_als_solve_rows(
            _lib.ptr(ptr), _lib.ptr(idx), _lib.ptr(val), _lib.ptr(order), n_rows, _lib.ptr(other), other.shape[0],
            self.emb_dim, _lib.ptr(g_reg), self.alpha, _lib.ptr(out), self.als_blocks, _lib.ptr(b["failed"]),
            _lib.ptr(stats), _lib.stream_ptr(dev)))
        failed = int(b["failed"].item())        # the half-sweep's one host sync
        self._check_status()
        if failed:
            raise FloatingPointError(
                f"ALS: {failed} of {n_rows} normal equations met a pivot that is not finite or <= 0 (a table holds a NaN "
                "or an Inf?); those rows were left unchanged")
        return out

    # ---- the interface of every factor model ----------------------------------------------------
    def forward(self, batch_data=None):
        """Nothing to do: the scores are dot products of the tables (``predict``)."""
        return 0.0

    def ranking_factors(self):
        """``(X, Y, 1.0, None)`` for full-catalogue ranking: the score is the plain dot product."""
        return self.user_factors.weight.data, self.item_factors.weight.data, 1.0, None

    def predict(self, users, items):
        """``x_u . y_i`` per pair, ``[n]`` fp32 (the two-table dot-product kernel CMN's ``predict`` uses)."""
        lib = self._require_hip()
        dev = self._flat.device
        users_t, items_t = index_tensor(users, dev), index_tensor(items, dev)
        if users_t.numel() != items_t.numel():
            raise ValueError("users and items differ in length")
        stats = self._device_stats()
        scores = torch.empty(users_t.numel(), dtype=torch.float32, device=dev)
        base = self._flat.data_ptr()
        w = _lib.UltraGcnTables(base, base + 4 * self.offset_of("item_factors.weight"), self.n_users, self.n_items,
                                self.emb_dim, 0)
        _lib.check(lib.hiprec_ultragcn_predict(ctypes.byref(w), _lib.ptr(users_t), _lib.ptr(items_t), users_t.numel(),
                                               _lib.ptr(scores), _lib.ptr(stats), _lib.stream_ptr(dev)))
        self._check_status()
        return scores

    def fold_in(self, user_ptr, item_idx, values=None):
        """Factor rows ``[n, D]`` for ``n`` users given as a CSR of item lists (``user_ptr [n + 1]``, ``item_idx``
        ascending and unique per user, ``values`` the multiplicities, ones when ``None``), solved against the current
        item table exactly as ``update_users`` solves a training row.  Neither table is touched; a user with an empty
        list gets zeros; an item id outside ``[0, n_items)`` raises ``IndexError``."""
        self._require_hip()
        dev = self._flat.device
        ptr, idx = index_tensor(user_ptr, dev), index_tensor(item_idx, dev)
        if ptr.numel() < 1 or int(ptr[0]) != 0 or int(ptr[-1]) != idx.numel() or bool((ptr[1:] < ptr[:-1]).any()):
            raise ValueError("user_ptr must start at 0, never decrease and end at len(item_idx)")
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= self.n_items):
            raise IndexError(f"fold_in: an item id lies outside [0, {self.n_items})")
        if values is None:
            val = torch.ones(idx.numel(), dtype=torch.float32, device=dev)
        else:
            val = torch.as_tensor(np.asarray(values) if not torch.is_tensor(values) else values).to(
                dev, torch.float32).reshape(-1).contiguous()
            if val.numel() != idx.numel():
                raise ValueError("values and item_idx differ in length")
        n = ptr.numel() - 1
        out = torch.zeros((n, self.emb_dim), dtype=torch.float32, device=dev)
        if n == 0:
            return out
        return self.solve_rows((ptr, idx, val), longest_first(ptr), self.item_factors.weight.data, out)


class ALSEngine(ModelEngine):
    """The trainer: ``prepare(data)`` once, then ``train_an_epoch`` = ``update_users`` + ``update_items`` + ``loss``.
    There is nothing to optimise step by step, so no optimizer is built."""

    _dp_world = 1     # data-parallel replicas (replicated.replicated_flat_engine) would set these
    _dp_rank = 0

    def __init__(self, config):
        self.config = config
        self.model = ALS(config["model"])
        self.set_device()
        self.model.to(self.device)
        print(self.model)
        self.writer = make_writer(config["system"]["run_dir"]) if "system" in config else None
        self._b = self._bt = None
        self._order_u = self._order_i = None
        self.last_loss = self.last_regularizer = None

    def _single(self):
        if self._dp_world != 1:
            raise NotImplementedError("ALS has no data-parallel form: a half-sweep is one exact solve over the whole frame, "
                                      "not a sum of per-sample gradients")

    def prepare(self, data):
        """Load the training frame -- a ``BaseData``-like object (``data.train[col_user] / [col_item]``) or a
        ``(users, items)`` pair -- as both CSRs with multiplicities and the two longest-first row orders."""
        self.require_hip()
        m = self.model
        dev = m.flat.device
        users, items = _frame_columns(data)
        users, items = index_tensor(users, dev), index_tensor(items, dev)
        self._b = build_interaction_csr(users, items, m.n_users, m.n_items)
        self._bt = build_interaction_csr(items, users, m.n_items, m.n_users)
        self._order_u, self._order_i = longest_first(self._b[0]), longest_first(self._bt[0])

    def _prepared(self):
        self._single()
        self.require_hip()
        if self._b is None:
            raise RuntimeError("ALSEngine: call prepare(data) first")
        return self.model

    def seen_csr(self):
        """``(user_ptr, pos_sorted)`` of the training frame, as ``recommend(..., seen=)`` takes it."""
        self._prepared()
        from .recommend import SeenCsr

        return SeenCsr((self._b[0], self._b[1]))

    def update_users(self):
        """The user half-sweep: every user's row from the current item table."""
        m = self._prepared()
        m.solve_rows(self._b, self._order_u, m.item_factors.weight.data, m.user_factors.weight.data)

    def update_items(self):
        """The item half-sweep: every item's row from the current user table."""
        m = self._prepared()
        m.solve_rows(self._bt, self._order_i, m.user_factors.weight.data, m.item_factors.weight.data)

    def loss(self):
        """``L(X, Y)`` of the current tables as a float (fp64 on the device; one host sync).  The regulariser's share is
        left in ``last_regularizer``."""
        m = self._prepared()
        lib = _lib.load()
        b = m._als_buffers()
        dev = m.flat.device
        stats = m._device_stats()
        X, Y = m.user_factors.weight.data, m.item_factors.weight.data
        G, _ = m.gram(Y)
        _lib.check(lib.hiprec_als_loss(
            _lib.ptr(self._b[0]), _lib.ptr(self._b[1]), _lib.ptr(self._b[2]), m.n_users, _lib.ptr(X), _lib.ptr(Y),
            m.n_items, m.emb_dim, _lib.ptr(G), m.alpha, m.reg, _lib.ptr(b["ws"]), b["bytes"], _lib.ptr(b["loss"]),
            _lib.ptr(stats), _lib.stream_ptr(dev)))
        total, reg = b["loss"].cpu().tolist()
        m._check_status()
        self.last_loss, self.last_regularizer = total, reg
        return total

    def train_single_batch(self, batch_data, ratings=None):
        raise NotImplementedError("ALS has no batch step: a half-sweep solves every row exactly from the whole training "
                                  "frame (prepare(data), then train_an_epoch / update_users / update_items)")

    def train_an_epoch(self, train_loader, epoch_id):
        """One full sweep; ``train_loader`` is ignored (the frame was handed to ``prepare``) and may be ``None``."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.update_users()
        self.update_items()
        total = self.loss()
        print("[Training Epoch {}], Loss {}".format(epoch_id, total))
        if self.writer is not None:
            self.writer.add_scalar("model/loss", total, epoch_id)
            self.writer.add_scalar("model/regularizer", self.last_regularizer, epoch_id)
        return total
