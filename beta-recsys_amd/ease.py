"""EASE: the closed-form item autoencoder (Steck, "Embarrassingly Shallow Autoencoders for Sparse Data", WWW 2019) on
the device (csrc/ease.hip).  The reference has no counterpart; the oracle is the fp64 restatement tests/ease_numpy.py.

``X`` is the **binary** ``[n_users, n_items]`` matrix of the training frame: a pair that occurs ``m`` times counts once,
as in the paper (ItemKNN and ALS keep the multiplicity; EASE does not).

* ``G = X^T X + reg I`` -- the item co-occurrence counts, ``reg`` (lambda, the one hyper-parameter) on the diagonal;
* ``P = G^-1`` by a blocked Cholesky factorisation in fp32 on the exact-fp32 MFMA;
* ``B[i, j] = -P[i, j] / P[j, j]`` for ``i != j`` and ``B[j, j] = 0``;
* ``score(u, j) = sum of B[i, j] over the distinct items i of u`` -- ItemKNN's score and top-K stage
  (``hiprec_knn_item_scores``) with ``B`` in the place of the similarity matrix.  That kernel adds the rows in ascending
  item order from ``+0`` and ranks through an order-preserving key of the fp32 bits, so a signed, asymmetric ``B`` is
  handled as it is; the one thing it assumes of ItemKNN's non-negative matrix is that ``0 + S[i, j]`` is ``S[i, j]`` to
  the bit, and with ``B`` that differs only in the sign of a zero, which the ranking treats as equal.

There is no learning rate, no sampling and no epoch: ``prepare_model`` is the whole training.  There is no CPU fallback:
the arithmetic runs in libhiprec.so on the GPU or not at all.
"""
import torch

from . import _lib
from ._stats import _new_stats, clear_status, read_stats
from .flat_engine import index_tensor
from .knn import MAX_K, OP_ITEM_SCORES, _KNNBase, _KNNEngine, build_interaction_csr

DEFAULT_REG = 500.0
DEFAULT_MAX_SIM_BYTES = 4 << 30    # G and the workspace: about 23 000 items
PANEL = 64                         # HIPREC_EASE_PANEL
LDS_CAP = 7168                     # HIPREC_EASE_LDS_CAP
MAX_USERS = 1 << 24                # HIPREC_EASE_MAX_USERS (exclusive): an fp32 count stays exact
MAX_ITEMS = 1 << 20                # HIPREC_EASE_MAX_ITEMS


def _idx(t):
    """A CSR's index array as the library takes it: an empty frame has no entries, and an empty tensor no address."""
    return t if t.numel() else torch.zeros(1, dtype=torch.int64, device=t.device)


def _check_bytes(n_items, max_sim_bytes):
    need = 2 * int(n_items) * int(n_items) * 4
    if need > int(max_sim_bytes):
        raise ValueError(f"EASE's [{n_items}, {n_items}] float32 matrix and its workspace take {need} bytes, more than "
                         f"max_sim_bytes={int(max_sim_bytes)}")
    return need


class _ItemWeightsBase(_KNNBase):
    """What the models with a dense ``[n_items, n_items]`` fp32 ``item_weights`` matrix share (EASE, SLIM): scoring and
    ranking through ItemKNN's stage with that matrix, ``recommend_for`` and the checkpoint."""

    SCORE_DTYPE = torch.float32

    # ---- scoring ----------------------------------------------------------------------------------------------------
    def _score_call(self, csr, n_rows, query, pair_ptr, pair_items, out_pick, topk, seen, out_items, out_scores):
        if self.item_weights is None:
            raise RuntimeError(f"{type(self).__name__}: call prepare_model(data) first")
        dev = query.device
        lib = _lib.load()
        need = lib.hiprec_knn_workspace_bytes(OP_ITEM_SCORES, n_rows, self.n_items, query.numel(), self.lds_cap)
        ws = torch.empty(max(need // 8, 1), dtype=torch.int64, device=dev)
        _lib.check(lib.hiprec_knn_item_scores(
            _lib.ptr(csr[0]), _lib.ptr(_idx(csr[1])), n_rows, self.n_items, _lib.ptr(self.item_weights), self.n_items,
            _lib.ptr(query), query.numel(), _lib.ptr(pair_ptr), _lib.ptr(pair_items), _lib.ptr(out_pick), topk,
            _lib.ptr(seen[0]) if seen else None, _lib.ptr(seen[1]) if seen else None, _lib.ptr(out_items),
            _lib.ptr(out_scores), self.lds_cap, _lib.ptr(ws), need, _lib.ptr(self._stats), _lib.stream_ptr(dev)))

    def _scores(self, query, pair_ptr, pair_items, out_pick, topk, seen, out_items, out_scores):
        self._score_call(self._b, self.n_users, query, pair_ptr, pair_items, out_pick, topk, seen, out_items, out_scores)

    def recommend_for(self, ptr, idx, k, exclude=True):
        """Top-``k`` for users outside the frame: row ``r`` of the CSR ``(ptr[n + 1], idx)`` is a user's item list (any
        order; an item listed twice counts once).  ``(items[n, k] int64, scores[n, k] float32)``, best first, ties to
        the lower id; ``exclude=True`` never returns an item of the user's own list.  A user with an empty list gets
        ``-1`` / ``-inf`` throughout (there is nothing to score from); an id outside ``[0, n_items)`` raises IndexError."""
        if self.item_weights is None:
            raise RuntimeError(f"{type(self).__name__}: call prepare_model(data) first")
        dev = self.item_weights.device
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in 1..{MAX_K}, got {k}")
        ptr_t, idx_t = index_tensor(ptr, dev).reshape(-1), index_tensor(idx, dev).reshape(-1)
        n = ptr_t.numel() - 1
        if n < 0 or (n >= 0 and (int(ptr_t[0]) != 0 or int(ptr_t[-1]) != idx_t.numel()
                                 or (n > 0 and bool((ptr_t[1:] < ptr_t[:-1]).any())))):
            raise ValueError("ptr must rise from 0 to len(idx)")
        out_items = torch.full((n, k), -1, dtype=torch.int64, device=dev)
        out_scores = torch.full((n, k), float("-inf"), dtype=torch.float32, device=dev)
        if n == 0 or idx_t.numel() == 0:
            return out_items, out_scores
        lengths = ptr_t[1:] - ptr_t[:-1]
        rows = torch.repeat_interleave(torch.arange(n, device=dev), lengths)
        csr = build_interaction_csr(rows, idx_t, n, self.n_items)[:2]      # IndexError for an id out of range
        if self._stats is None:
            self._stats = _new_stats(dev)
        query = torch.arange(n, dtype=torch.int64, device=dev)
        self._score_call(csr, n, query, None, None, None, k, csr if exclude else None, out_items, out_scores)
        self._raise_status((out_items, out_scores))
        empty = (lengths == 0).unsqueeze(1)
        return out_items.masked_fill_(empty, -1), out_scores.masked_fill_(empty, float("-inf"))

    # ---- checkpoint: the weights are the model ----------------------------------------------------------------------
    def state_dict(self, *args, **kwargs):
        sd = super().state_dict(*args, **kwargs)
        if self.item_weights is not None:
            sd["item_weights"] = self.item_weights
        return sd

    def load_state_dict(self, state_dict, strict=True):
        B = state_dict.get("item_weights")
        if B is None:
            self.item_weights = None
            return
        if tuple(B.shape) != (self.n_items, self.n_items):
            raise ValueError(f"item_weights is {tuple(B.shape)}, this model has n_items={self.n_items}")
        self.item_weights = B.to(device=self._device(), dtype=torch.float32).contiguous().clone()


class EASE(_ItemWeightsBase):
    """Config keys: ``n_users``, ``n_items``, ``reg`` (lambda > 0, default 500.0), ``device_str``, ``max_sim_bytes``
    (default 4 GiB; bounds ``G`` plus the workspace, ``2 * n_items^2 * 4`` bytes).  ``lds_cap`` moves the Gram stage's
    accumulator between LDS and the workspace (the result does not depend on it) and ``keep_inverse=True`` keeps
    ``P = G^-1`` as ``self.inverse`` -- both for the tests."""

    def __init__(self, config):
        super().__init__(dict(config, neighbourhood_size=0))
        self.config = config
        self.reg = float(config.get("reg", DEFAULT_REG))
        if not (self.reg > 0.0 and self.reg < float("inf")):
            raise ValueError(f"reg must be finite and > 0, got {self.reg}")
        if self.n_users >= MAX_USERS or self.n_items > MAX_ITEMS:
            raise ValueError(f"n_users must be < {MAX_USERS} and n_items <= {MAX_ITEMS}")
        self.max_sim_bytes = int(config.get("max_sim_bytes", DEFAULT_MAX_SIM_BYTES))
        _check_bytes(self.n_items, self.max_sim_bytes)
        self.keep_inverse = bool(config.get("keep_inverse", False))
        self.item_weights = None
        self.inverse = None

    # ---- the three stages -------------------------------------------------------------------------------------------
    def _ease_workspace(self, lib, dev):
        need = lib.hiprec_ease_workspace_bytes(self.n_users, self.n_items)
        if need == (1 << 64) - 1:
            raise ValueError(f"bad sizes (n_users={self.n_users}, n_items={self.n_items})")
        return torch.empty(need // 4, dtype=torch.float32, device=dev), need

    def gram(self, workspace=None):
        """``G = X^T X + reg I`` of the loaded frame, ``[n_items, n_items]`` fp32."""
        dev = self._prepared()
        lib = _lib.load()
        ws, ws_bytes = workspace if workspace is not None else self._ease_workspace(lib, dev)
        G = torch.empty((self.n_items, self.n_items), dtype=torch.float32, device=dev)
        b, bt = self._b, self._bt
        _lib.check(lib.hiprec_ease_gram(
            _lib.ptr(bt[0]), _lib.ptr(_idx(bt[1])), _lib.ptr(b[0]), _lib.ptr(_idx(b[1])), self.n_users, self.n_items,
            self.reg, _lib.ptr(G), self.lds_cap, _lib.ptr(ws), ws_bytes, _lib.ptr(self._stats), _lib.stream_ptr(dev)))
        return G

    def _invert(self, G, ws, ws_bytes):
        """``G`` -> the lower triangle of its inverse, in place; FloatingPointError on a pivot that is not positive."""
        lib = _lib.load()
        n = G.shape[0]
        _lib.check(lib.hiprec_ease_invert(_lib.ptr(G), n, _lib.ptr(ws), ws_bytes, _lib.ptr(self._stats),
                                          _lib.stream_ptr(G.device)))

    def _finish(self, P, B):
        lib = _lib.load()
        _lib.check(lib.hiprec_ease_finish(_lib.ptr(P), P.shape[0], _lib.ptr(B), _lib.ptr(self._stats),
                                          _lib.stream_ptr(P.device)))

    def _raise_not_spd(self):
        """After the three stages: the failed-pivot flag first (a numeric answer, not a fault), then the id flags."""
        st = read_stats(self._stats)
        if st.status & _lib.STATUS_NOT_SPD:
            clear_status(self._stats)
            raise FloatingPointError("EASE: a pivot of the Cholesky factorisation of G = X^T X + reg I was not positive "
                                     "and finite (NaN in the matrix, or reg too small for float32)")
        if st.status:
            self._raise_status(None)

    def weights_from_gram(self, G):
        """``(B, P)`` of a caller's symmetric matrix ``G`` (``[n, n]`` fp32 on the device; it is not changed): the
        inversion and the last stage on their own.  Raises FloatingPointError when ``G`` is not positive definite.
        (The tests plant a NaN and a negative pivot through here.)"""
        dev = self._device()
        if G.dim() != 2 or G.shape[0] != G.shape[1] or G.dtype != torch.float32:
            raise ValueError("G must be a square float32 matrix")
        if self._stats is None:
            self._stats = _new_stats(dev)
        P = G.to(dev).contiguous().clone()
        n = P.shape[0]
        W = torch.empty((n, n), dtype=torch.float32, device=dev)
        clear_status(self._stats)
        self._invert(P, W, n * n * 4)
        B = W                                   # L^-1 is no longer needed once P stands
        self._finish(P, B)
        self._raise_not_spd()
        return B, P

    def prepare_model(self, data):
        """Load the frame, run the three stages and publish ``item_weights`` (``B``).  On a failed pivot it raises
        FloatingPointError and ``item_weights`` is ``None``."""
        self.item_weights = self.inverse = None
        dev = self._load_matrix(data)
        _check_bytes(self.n_items, self.max_sim_bytes)
        lib = _lib.load()
        ws, ws_bytes = self._ease_workspace(lib, dev)
        clear_status(self._stats)
        G = self.gram((ws, ws_bytes))
        self._invert(G, ws, ws_bytes)
        B = ws[:self.n_items * self.n_items].view(self.n_items, self.n_items)
        self._finish(G, B)
        self._raise_not_spd()
        self.item_weights = B
        self.inverse = G if self.keep_inverse else None


class EASEEngine(_KNNEngine):
    """Like ItemKNNEngine: nothing to optimise, ``train_single_batch`` returns 0 and ``train_an_epoch`` prints the
    "skipped" line; ``save_checkpoint`` / ``resume_checkpoint`` carry ``B`` (the frame is loaded by ``prepare_model``)."""

    MODEL = EASE

    def __init__(self, config):
        super().__init__(config)
        self.device = self.model.device
