"""ItemKNN and UserKNN: the neighbourhood baselines of ``beta_rec/models/itemKNN.py`` and ``userKNN.py`` on the device
(csrc/knn.hip).

``B`` is the ``[n_users, n_items]`` interaction matrix of the training frame *with multiplicities* (the reference's
``coo_matrix((ones, (user, item))).tocsr()``: a pair that occurs ``m`` times has value ``m``).

* **ItemKNN**: ``S[i, j] = overlap_i[j] / sqrt(cnt[j])`` (float64, stored float32; ``overlap_i[j]`` sums ``B[v, j]`` over
  the distinct users of column ``i``); a user's score row is the float32 sum of ``S[i, :]`` over the user's distinct
  items, ascending.  Nothing is masked and ``neighbourhood_size`` is read but never used -- as in the reference.
* **UserKNN**: ``sim[v] = overlap[v] / sqrt(cu[v])`` in float64, the ``neighbourhood_size`` users with the largest
  ``sim`` (the query user is one of them; users with ``sim == 0`` fill the list), ``score[j] = sum sim[v] * B[v, j]``
  over them in float64, and ``-inf`` on the user's own items.

**The sequence.**  Both ``predict`` methods of the reference take the user's sequence as
``binary_user_item.getrow(u).nonzero()[0]``: the *row* coordinates of a one-row matrix, ``nnz(u)`` zeros, where the
user's items are ``nonzero()[1]``.  As written the reference scores every user as if they had interacted with item 0,
``nnz(u)`` times.  Its building blocks (``similarity_with_users``, ``similarity_with_items``, ``top_k``,
``get_sparse_vector``, ``generate_item_sim_matrix``) are right when handed the user's items, and that is what this
mirror computes; ``tests/test_oracle_golden_knn.py`` pins the defect reading against the reference's recorded output.

Where the reference has no defined answer: ties of ``sim`` at the cut go to the lower user id (``argpartition`` there);
ItemKNN's ``predict`` for a user without training rows returns zeros (a stale variable there); ``neighbourhood_size`` is
clamped to ``n_users`` (the reference raises).

There is no CPU fallback: the arithmetic runs in libhiprec.so on the GPU or not at all.  torch builds the two CSRs
(a sort and a few scans -- plumbing).
"""
import torch

from . import _lib
from ._stats import _new_stats, clear_status, raise_on_status, read_stats
from .flat_engine import index_tensor
from .torch_engine import ModelEngine

MAX_K = 128                        # HIPREC_KNN_MAX_K: neighbourhood_size and the length of a recommendation list
LDS_CAP = 7168                     # HIPREC_KNN_LDS_CAP: accumulator entries a block keeps in LDS
DEFAULT_MAX_SIM_BYTES = 4 << 30    # ItemKNN's [n_items, n_items] float32 matrix: about 32 700 items
OP_ITEM_SIMILARITY, OP_ITEM_SCORES, OP_USER_SCORES = 0, 1, 2
DEFAULT_USER_COL, DEFAULT_ITEM_COL = "col_user", "col_item"


def build_interaction_csr(users, items, n_users, n_items):
    """``(ptr[n_users + 1] int64, idx int64, val float32)`` of ``coo_matrix((ones, (users, items))).tocsr()`` with
    its duplicates summed: rows ascending and unique, ``val`` the number of times the pair occurs -- torch ops on the
    tensors' device (``data.build_positive_csr`` plus the counts)."""
    users, items = users.to(torch.int64).reshape(-1), items.to(torch.int64).reshape(-1)
    if users.numel() != items.numel():
        raise ValueError(f"users and items differ in length ({users.numel()}, {items.numel()})")
    if users.numel() and (int(users.min()) < 0 or int(users.max()) >= n_users
                          or int(items.min()) < 0 or int(items.max()) >= n_items):
        raise IndexError("training frame holds a user / item id outside [0, n_users) x [0, n_items)")
    key, counts = torch.unique(users * n_items + items, return_counts=True)          # sorted
    owner = torch.div(key, n_items, rounding_mode="floor")
    ptr = torch.zeros(n_users + 1, dtype=torch.int64, device=users.device)
    torch.cumsum(torch.bincount(owner, minlength=n_users), 0, out=ptr[1:])
    return ptr, (key - owner * n_items).contiguous(), counts.to(torch.float32).contiguous()


def _row_sums(csr):
    """float64 row sums of a CSR with multiplicities, by a scan and a difference at the row pointers (integers:
    exact) -- not an ``index_add_`` of the frame's rows, which is one contended fp64 atomic per interaction."""
    ptr, _, val = csr
    total = torch.zeros(val.numel() + 1, dtype=torch.float64, device=val.device)
    torch.cumsum(val.to(torch.float64), 0, out=total[1:])
    return (total[ptr[1:]] - total[ptr[:-1]]).contiguous()


def _frame_columns(data):
    """The ``(users, items)`` id columns of ``data``: an object with ``data.train[col_user] / [col_item]`` (the
    reference's ``BaseData``) or the pair itself."""
    if isinstance(data, (tuple, list)) and len(data) == 2:
        return data
    train = data.train
    cols = []
    for name in (DEFAULT_USER_COL, DEFAULT_ITEM_COL):
        col = train[name]
        cols.append(col.to_numpy() if hasattr(col, "to_numpy") else col)
    return tuple(cols)


def _check_sim_bytes(n_items, max_sim_bytes):
    need = int(n_items) * int(n_items) * 4
    if need > int(max_sim_bytes):
        raise ValueError(f"ItemKNN's [{n_items}, {n_items}] float32 similarity matrix takes {need} bytes, more than "
                         f"max_sim_bytes={int(max_sim_bytes)}")
    return need


class _KNNBase(torch.nn.Module):
    """What the two models share: the config keys of the reference, the two CSRs, the output stage's plumbing."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.device = self.config["device_str"]
        self.n_users = int(self.config["n_users"])
        self.n_items = int(self.config["n_items"])
        self.neighbourhood_size = int(self.config["neighbourhood_size"])
        if self.n_users < 1 or self.n_items < 1:
            raise ValueError("n_users and n_items must be >= 1")
        self.lds_cap = int(self.config.get("lds_cap", 0))    # 0 = chosen by the library; the result does not depend on it
        self._b = self._bt = None
        self._stats = None

    def forward(self, batch_data):
        """Redundant, as in the reference."""
        return 0.0

    def _device(self):
        dev = torch.device(self.device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"hiprec neighbourhood models run on an MI355X through libhiprec.so; device {dev} has no "
                               "HIP path and there is deliberately no CPU fallback")
        return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)

    def _load_matrix(self, data):
        dev = self._device()
        users, items = _frame_columns(data)
        users, items = index_tensor(users, dev), index_tensor(items, dev)
        self._b = build_interaction_csr(users, items, self.n_users, self.n_items)
        self._bt = build_interaction_csr(items, users, self.n_items, self.n_users)
        self.items_count_per_user = _row_sums(self._b)
        self.users_count_per_item = _row_sums(self._bt)
        self._stats = _new_stats(dev)
        return dev

    def _prepared(self):
        if self._b is None:
            raise RuntimeError(f"{type(self).__name__}: call prepare_model(data) first")
        return self._b[0].device

    def seen_csr(self):
        """``(user_ptr, pos_sorted)`` of the training frame, as ``recommend(..., seen=)`` takes it."""
        self._prepared()
        from .recommend import SeenCsr

        return SeenCsr((self._b[0], self._b[1]))

    def _workspace(self, lib, op, n_query, dev):
        need = lib.hiprec_knn_workspace_bytes(op, self.n_users, self.n_items, n_query, self.lds_cap)
        if need == (1 << 64) - 1:
            raise ValueError(f"bad sizes (n_users={self.n_users}, n_items={self.n_items}, lds_cap={self.lds_cap})")
        return torch.empty(max(need // 8, 1), dtype=torch.int64, device=dev), need

    def _raise_status(self, partial):
        st = read_stats(self._stats)
        if st.status:
            clear_status(self._stats)
            err = None
            try:
                raise_on_status(st.status)
            except IndexError as exc:
                err = exc
            err.partial = partial           # the rows of the in-range queries are complete
            raise err

    def _scores(self, query, pair_ptr, pair_items, out_pick, topk, seen, out_items, out_scores):
        raise NotImplementedError

    def predict(self, users, items):
        """One score per (user, item) pair: float32 for ItemKNN, float64 for UserKNN, as the reference returns.  The
        pairs are grouped by user, so a user's score row is formed once however many of its pairs are asked for."""
        dev = self._prepared()
        users_t, items_t = index_tensor(users, dev), index_tensor(items, dev)
        if users_t.numel() != items_t.numel():
            raise ValueError("users and items differ in length")
        out = torch.zeros(users_t.numel(), dtype=self.SCORE_DTYPE, device=dev)
        if users_t.numel() == 0:
            return out
        order = torch.argsort(users_t, stable=True)
        query, counts = torch.unique_consecutive(users_t[order], return_counts=True)
        pair_ptr = torch.zeros(query.numel() + 1, dtype=torch.int64, device=dev)
        torch.cumsum(counts, 0, out=pair_ptr[1:])
        picked = torch.zeros_like(out)
        self._scores(query.contiguous(), pair_ptr, items_t[order].contiguous(), picked, 0, None, None, None)
        out[order] = picked
        self._raise_status(out)
        return out

    def topk_items(self, users, k, seen=None, item_splits=0):
        """``(items[n, k] int64, scores[n, k] float32)``: the hook ``recommend.recommend`` and ``eval.evaluate_full``
        rank this model through (``item_splits`` belongs to the factor models' kernel and is ignored)."""
        from .recommend import normalise_seen

        dev = self._prepared()
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in 1..{MAX_K}, got {k}")
        csr = normalise_seen(seen, self.n_users, self.n_items, dev)
        query = index_tensor(users, dev)
        out_items = torch.empty((query.numel(), k), dtype=torch.int64, device=dev)
        out_scores = torch.empty((query.numel(), k), dtype=torch.float32, device=dev)
        if query.numel() == 0:
            return out_items, out_scores
        self._scores(query, None, None, None, k, csr, out_items, out_scores)
        self._raise_status((out_items, out_scores))
        return out_items, out_scores

    def recommend(self, users, k, seen=None):
        """The ``k`` best items per query user, best first (ties to the lower id), never an item of the user's ``seen``
        row (``None`` masks nothing; ``model.seen_csr()`` is the training frame); ``-1`` / ``-inf`` in the tail."""
        return self.topk_items(users, k, seen)


class ItemKNN(_KNNBase):
    """models/itemKNN.py:39-124.  ``config["max_sim_bytes"]`` (default 4 GiB) bounds the similarity matrix."""

    SCORE_DTYPE = torch.float32

    def __init__(self, config):
        super().__init__(config)
        self.max_sim_bytes = int(self.config.get("max_sim_bytes", DEFAULT_MAX_SIM_BYTES))
        _check_sim_bytes(self.n_items, self.max_sim_bytes)
        self.item_sim_matrix = None

    def prepare_model(self, data):
        """Load the frame and build ``item_sim_matrix`` (``generate_item_sim_matrix``) on the device."""
        self._load_matrix(data)
        self.item_sim_matrix = self.generate_item_sim_matrix()

    def generate_item_sim_matrix(self):
        dev = self._prepared()
        _check_sim_bytes(self.n_items, self.max_sim_bytes)
        lib = _lib.load()
        S = torch.empty((self.n_items, self.n_items), dtype=torch.float32, device=dev)
        ws, ws_bytes = self._workspace(lib, OP_ITEM_SIMILARITY, 0, dev)
        b, bt = self._b, self._bt
        _lib.check(lib.hiprec_knn_item_similarity(
            _lib.ptr(bt[0]), _lib.ptr(bt[1]), _lib.ptr(b[0]), _lib.ptr(b[1]), _lib.ptr(b[2]),
            _lib.ptr(self.users_count_per_item), self.n_users, self.n_items, _lib.ptr(S), self.n_items, self.lds_cap,
            _lib.ptr(ws), ws_bytes, _lib.stream_ptr(dev)))
        return S

    def _scores(self, query, pair_ptr, pair_items, out_pick, topk, seen, out_items, out_scores):
        if self.item_sim_matrix is None:
            raise RuntimeError("ItemKNN: call prepare_model(data) first")
        dev = query.device
        lib = _lib.load()
        ws, ws_bytes = self._workspace(lib, OP_ITEM_SCORES, query.numel(), dev)
        _lib.check(lib.hiprec_knn_item_scores(
            _lib.ptr(self._b[0]), _lib.ptr(self._b[1]), self.n_users, self.n_items, _lib.ptr(self.item_sim_matrix),
            self.n_items, _lib.ptr(query), query.numel(), _lib.ptr(pair_ptr), _lib.ptr(pair_items), _lib.ptr(out_pick),
            topk, _lib.ptr(seen[0]) if seen else None, _lib.ptr(seen[1]) if seen else None, _lib.ptr(out_items),
            _lib.ptr(out_scores), self.lds_cap, _lib.ptr(ws), ws_bytes, _lib.ptr(self._stats), _lib.stream_ptr(dev)))


class UserKNN(_KNNBase):
    """models/userKNN.py:31-109.  ``1 <= neighbourhood_size <= 128``; it is clamped to ``n_users``."""

    SCORE_DTYPE = torch.float64

    def __init__(self, config):
        super().__init__(config)
        if not 1 <= self.neighbourhood_size <= MAX_K:
            raise ValueError(f"neighbourhood_size must be in 1..{MAX_K}, got {self.neighbourhood_size}")
        self.k = min(self.neighbourhood_size, self.n_users)

    def prepare_model(self, data):
        self._load_matrix(data)

    def _scores(self, query, pair_ptr, pair_items, out_pick, topk, seen, out_items, out_scores, nb=None):
        dev = query.device
        lib = _lib.load()
        ws, ws_bytes = self._workspace(lib, OP_USER_SCORES, query.numel(), dev)
        b, bt = self._b, self._bt
        _lib.check(lib.hiprec_knn_user_scores(
            _lib.ptr(b[0]), _lib.ptr(b[1]), _lib.ptr(b[2]), _lib.ptr(bt[0]), _lib.ptr(bt[1]), _lib.ptr(bt[2]),
            _lib.ptr(self.items_count_per_user), self.n_users, self.n_items, self.k, _lib.ptr(query), query.numel(),
            _lib.ptr(nb[0]) if nb else None, _lib.ptr(nb[1]) if nb else None, _lib.ptr(pair_ptr), _lib.ptr(pair_items),
            _lib.ptr(out_pick), topk, _lib.ptr(seen[0]) if seen else None, _lib.ptr(seen[1]) if seen else None,
            _lib.ptr(out_items), _lib.ptr(out_scores), self.lds_cap, _lib.ptr(ws), ws_bytes, _lib.ptr(self._stats),
            _lib.stream_ptr(dev)))

    def neighbours(self, users):
        """``(ids[n, k] int64, sims[n, k] float64)``: every query user's neighbours, best first (``k`` is
        ``neighbourhood_size`` clamped to ``n_users``)."""
        dev = self._prepared()
        query = index_tensor(users, dev)
        ids = torch.empty((query.numel(), self.k), dtype=torch.int64, device=dev)
        sims = torch.empty((query.numel(), self.k), dtype=torch.float64, device=dev)
        if query.numel() == 0:
            return ids, sims
        self._scores(query, None, None, None, 0, None, None, None, nb=(ids, sims))
        self._raise_status((ids, sims))
        return ids, sims


class _KNNEngine(ModelEngine):
    """The engines of the two models: like the reference's they do not call the base constructor (there is nothing to
    optimise), ``train_single_batch`` returns 0 and ``train_an_epoch`` prints the reference's line."""

    MODEL = None

    def __init__(self, config):
        self.config = config
        self.model = self.MODEL(config["model"])

    def train_single_batch(self, batch_data):
        assert hasattr(self, "model"), "Please specify the exact model !"
        return 0

    def train_an_epoch(self, train_loader, epoch_id):
        assert hasattr(self, "model"), "Please specify the exact model !"
        print(f"[Training Epoch {epoch_id}] skipped")
        writer = getattr(self, "writer", None)      # (the reference's engines never make one)
        if writer is not None:
            writer.add_scalar("model/loss", 0.0, epoch_id)
            writer.add_scalar("model/regularizer", 0.0, epoch_id)

    def recommend(self, users, k, seen=None, item_splits=0):
        return self.model.recommend(users, k, seen)


class ItemKNNEngine(_KNNEngine):
    """models/itemKNN.py:127-163."""

    MODEL = ItemKNN


class UserKNNEngine(_KNNEngine):
    """models/userKNN.py:112-149."""

    MODEL = UserKNN

    def __init__(self, config):
        print("userKNNEngine init")
        super().__init__(config)
