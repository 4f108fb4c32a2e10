"""SLIM: the sparse linear item model (Ning and Karypis, "SLIM: Sparse Linear Methods for Top-N Recommender Systems",
ICDM 2011) on the device (csrc/slim.hip).  The reference has no counterpart; the oracle is the restatement
tests/slim_numpy.py.

``X`` is the **binary** ``[n_users, n_items]`` matrix of the training frame, as in EASE.  With ``G = X^T X`` and
``A = G + l2 I`` (``hiprec_ease_gram`` with ``reg = l2``), column ``w = W[:, j]`` minimises

    1/2 w^T A w - G[:, j]^T w + l1 * sum |w_k|        subject to w_j = 0 and, with ``positive_only``, w >= 0

which is the paper's ``1/2 ||x_j - X w||^2 + l2/2 ||w||^2 + l1 ||w||_1``.  ``l2 > 0`` makes the problem strictly convex
and the solution unique.  The solver is cyclic coordinate descent with a soft threshold, one workgroup per column, from
``w = 0``: a sweep visits the coordinates in ascending order and a column stops after the first sweep whose largest move
is ``<= tol``, or after ``max_sweeps`` sweeps (then it counts as unconverged: a warning, not an error).

``score(u, j) = sum of W[i, j] over the distinct items i of u``: ItemKNN's score and top-K stage with ``W`` as the matrix,
shared with EASE.  There is no CPU fallback: the arithmetic runs in libhiprec.so on the GPU or not at all.
"""
import math
import warnings

import torch

from . import _lib
from ._stats import _new_stats, clear_status, read_stats
from .ease import MAX_ITEMS, MAX_USERS, _idx, _ItemWeightsBase
from .knn import _KNNEngine

DEFAULT_L1 = 1.0                   # the SLIM library's defaults, on the count scale of G
DEFAULT_L2 = 1.0
DEFAULT_TOL = 1e-5
DEFAULT_MAX_SWEEPS = 100
DEFAULT_MAX_SIM_BYTES = 4 << 30    # A and W: about 23 000 items
CHUNK = 64                         # HIPREC_SLIM_CHUNK
LDS_CAP = 8192                     # HIPREC_SLIM_LDS_CAP
MAX_SWEEPS = 1000000               # HIPREC_SLIM_MAX_SWEEPS


def _check_bytes(n_items, max_sim_bytes):
    need = 2 * int(n_items) * int(n_items) * 4
    if need > int(max_sim_bytes):
        raise ValueError(f"SLIM's [{n_items}, {n_items}] float32 matrices A and W take {need} bytes, more than "
                         f"max_sim_bytes={int(max_sim_bytes)}")
    return need


class SLIM(_ItemWeightsBase):
    """Config keys: ``n_users``, ``n_items``, ``l1_reg`` (>= 0, default 1.0), ``l2_reg`` (> 0, default 1.0),
    ``positive_only`` (default True), ``tol`` (>= 0, default 1e-5), ``max_sweeps`` (>= 1, default 100), ``device_str``,
    ``max_sim_bytes`` (default 4 GiB; bounds ``A`` plus ``W``, ``2 * n_items^2 * 4`` bytes).  ``lds_cap`` moves the Gram
    stage's accumulator and the solver's two vectors between LDS and the workspace; the result does not depend on it.

    After ``prepare_model``: ``item_weights`` (``W``), ``sweeps`` (int32 per column), ``n_unconverged``, ``nnz``."""

    def __init__(self, config):
        super().__init__(dict(config, neighbourhood_size=0))
        self.config = config
        self.l1_reg = float(config.get("l1_reg", DEFAULT_L1))
        self.l2_reg = float(config.get("l2_reg", DEFAULT_L2))
        self.tol = float(config.get("tol", DEFAULT_TOL))
        self.max_sweeps = int(config.get("max_sweeps", DEFAULT_MAX_SWEEPS))
        self.positive_only = bool(config.get("positive_only", True))
        if not (self.l1_reg >= 0.0 and math.isfinite(self.l1_reg)):
            raise ValueError(f"l1_reg must be finite and >= 0, got {self.l1_reg}")
        if not (self.l2_reg > 0.0 and math.isfinite(self.l2_reg)):
            raise ValueError(f"l2_reg must be finite and > 0, got {self.l2_reg}")
        if not (self.tol >= 0.0 and math.isfinite(self.tol)):
            raise ValueError(f"tol must be finite and >= 0, got {self.tol}")
        if not 1 <= self.max_sweeps <= MAX_SWEEPS:
            raise ValueError(f"max_sweeps must be in 1..{MAX_SWEEPS}, got {self.max_sweeps}")
        if self.n_users >= MAX_USERS or self.n_items > MAX_ITEMS:
            raise ValueError(f"n_users must be < {MAX_USERS} and n_items <= {MAX_ITEMS}")
        self.max_sim_bytes = int(config.get("max_sim_bytes", DEFAULT_MAX_SIM_BYTES))
        _check_bytes(self.n_items, self.max_sim_bytes)
        self.item_weights = None
        self.sweeps = None
        self.n_unconverged = None
        self.nnz = None

    # ---- the two stages ---------------------------------------------------------------------------------------------
    def gram(self):
        """``A = X^T X + l2 I`` of the loaded frame, ``[n_items, n_items]`` fp32 (integer counts off the diagonal)."""
        dev = self._prepared()
        lib = _lib.load()
        need = lib.hiprec_ease_workspace_bytes(self.n_users, self.n_items)
        if need == (1 << 64) - 1:
            raise ValueError(f"bad sizes (n_users={self.n_users}, n_items={self.n_items})")
        ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
        A = torch.empty((self.n_items, self.n_items), dtype=torch.float32, device=dev)
        b, bt = self._b, self._bt
        _lib.check(lib.hiprec_ease_gram(
            _lib.ptr(bt[0]), _lib.ptr(_idx(bt[1])), _lib.ptr(b[0]), _lib.ptr(_idx(b[1])), self.n_users, self.n_items,
            self.l2_reg, _lib.ptr(A), self.lds_cap, _lib.ptr(ws), need, _lib.ptr(self._stats), _lib.stream_ptr(dev)))
        return A

    def _solve(self, A):
        """``(W, sweeps, n_unconverged)`` of the device matrix ``A``; the status word says whether a step was not
        finite."""
        lib = _lib.load()
        dev = A.device
        n = A.shape[0]
        need = lib.hiprec_slim_workspace_bytes(n, self.lds_cap)
        if need == (1 << 64) - 1:
            raise ValueError(f"bad sizes (n={n}, lds_cap={self.lds_cap})")
        ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
        W = torch.empty((n, n), dtype=torch.float32, device=dev)
        raw = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(lib.hiprec_slim_fit(
            _lib.ptr(A), n, self.l1_reg, int(self.positive_only), self.tol, self.max_sweeps, _lib.ptr(W), _lib.ptr(raw),
            self.lds_cap, _lib.ptr(ws), need, _lib.ptr(self._stats), _lib.stream_ptr(dev)))
        st = read_stats(self._stats)                 # (synchronises: the workspace may go)
        if st.status & _lib.STATUS_NOT_FINITE:
            clear_status(self._stats)
            raise FloatingPointError("SLIM: a coordinate step was not finite (NaN or inf in A = X^T X + l2 I, or a zero "
                                     "on its diagonal)")
        if st.status:
            self._raise_status(None)
        return W, raw.abs(), int((raw < 0).sum())

    def _warn_unconverged(self, n_unconverged, n):
        if n_unconverged:
            warnings.warn(f"SLIM: {n_unconverged} of {n} columns did not meet tol={self.tol:g} within "
                          f"max_sweeps={self.max_sweeps}; their weights are the last sweep's", RuntimeWarning,
                          stacklevel=3)

    def fit_from_gram(self, A):
        """``(W, sweeps, n_unconverged)`` of a caller's symmetric matrix ``A`` (``[n, n]`` fp32; it is not changed): the
        solver on its own, with this model's parameters.  Raises FloatingPointError when a step is not finite.  (The
        tests plant a NaN through here.)"""
        dev = self._device()
        if A.dim() != 2 or A.shape[0] != A.shape[1] or A.dtype != torch.float32:
            raise ValueError("A must be a square float32 matrix")
        if self._stats is None:
            self._stats = _new_stats(dev)
        clear_status(self._stats)
        W, sweeps, n_unconverged = self._solve(A.to(dev).contiguous())
        self._warn_unconverged(n_unconverged, A.shape[0])
        return W, sweeps, n_unconverged

    def prepare_model(self, data):
        """Load the frame, form ``A``, solve every column and publish ``item_weights`` (``W``), ``sweeps``,
        ``n_unconverged`` and ``nnz``.  Unconverged columns give one warning and stay usable; a step that is not finite
        raises FloatingPointError and ``item_weights`` is ``None``."""
        self.item_weights = self.sweeps = self.n_unconverged = self.nnz = None
        self._load_matrix(data)
        _check_bytes(self.n_items, self.max_sim_bytes)
        clear_status(self._stats)
        W, sweeps, n_unconverged = self._solve(self.gram())
        self.item_weights, self.sweeps, self.n_unconverged = W, sweeps, n_unconverged
        self.nnz = int(torch.count_nonzero(W))
        self._warn_unconverged(n_unconverged, self.n_items)


class SLIMEngine(_KNNEngine):
    """Like ItemKNNEngine: nothing to optimise, ``train_single_batch`` returns 0 and ``train_an_epoch`` prints the
    "skipped" line; ``save_checkpoint`` / ``resume_checkpoint`` carry ``W`` (the frame is loaded by ``prepare_model``)."""

    MODEL = SLIM

    def __init__(self, config):
        super().__init__(config)
        self.device = self.model.device
