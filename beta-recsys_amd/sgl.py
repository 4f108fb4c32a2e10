"""Drop-in ``SGL`` / ``SGLEngine`` for beta_rec/models/sgl.py on libhiprec.so.

Interface parity (file:line = beta_rec/models/sgl.py): ``SGL(config)`` :229-405 (bare parameters ``user_embedding`` /
``item_embedding``, xavier-uniform, in that order; ``predict``), ``SGLEngine(config)`` :408-585
(``train_single_batch(sub_mat, batch_data) -> float``, ``train_an_epoch``, ``sub_mat_refresher``, ``create_sgl_mat``,
``randint_choice``).  Same config keys (``n_users n_items emb_dim n_layers regs ssl_reg ssl_temp ssl_mode ssl_ratio
aug_type is_subgraph pretrain norm_adj optimizer lr device_str``), same ``state_dict`` keys, same initial weights for the
same torch seed.

The step: three LightGCN propagations (``norm_adj``, sub-graph 1, sub-graph 2), each mean-pooled over ``L + 1`` hops;
loss = BPR **sum** on the main view + ``regs / 2`` x squares of the batch's hop-0 rows + ``ssl_reg`` x InfoNCE of the
batch's view-1 rows against **every** view-2 row of their side.  ``csrc/sgl.hip`` never forms the ``[B, n]`` score
matrices.  There is no CPU path.

Not kept:
* ``predict`` propagates from the CURRENT weights (cached until they change); the reference reads the tables its last
  training forward left behind -- the weights from before that step -- and fails before any step (sgl.py:396-405);
* ``ssl_mode = "merge"`` raises ``ValueError``; the reference always crashes there (sgl.py:168: ``batch_items, _ =
  torch.unique(pos_items)`` unpacks a tensor);
* ``aug_type = 0`` works, with ``int(n * ssl_ratio)`` dropped nodes per side; the reference passes the float
  ``n * ssl_ratio`` as ``size`` and ``np.random.choice`` raises ``TypeError`` for it, integral or not (sgl.py:477-482);
* the BPR term and the InfoNCE term are computed in their shifted, stable forms;
* ``pretrain`` truthy skips the sub-graph views entirely, not just the loss (sgl.py:361-362).
An all-zero pooled row divides by zero in both (no clamp).

Extensions: ``sub_rng = "numpy"`` (default) replays the reference's ``np.random.choice`` calls on the host, in its order
(the same ``np.random.seed`` gives the same kept set); ``"device"`` takes the first ``k`` of
``hiprec_random_permutation`` from ``sub_seed``.  ``last_losses()`` returns ``(bpr, emb, ssl)``.
"""
import ctypes

import numpy as np
import torch
from torch.nn import Parameter

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, index_tensor
from .lightgcn import _csr_from_coo, _slice_rows
from .mixgcf import coo_to_csr_maps

SSL_MODES = {"user_side": 1, "item_side": 2, "both_side": 3}
MAX_LAYERS = _lib.SGL_MAX_LAYERS


def randint_choice(high, size=None, replace=True, p=None, exclusion=None):
    """sgl.py:9-22, draw for draw."""
    a = np.arange(high)
    if exclusion is not None:
        p = np.ones_like(a) if p is None else np.array(p, copy=True)
        p = p.flatten()
        p[exclusion] = 0
    if p is not None:
        p = p / np.sum(p)
    return np.random.choice(a, size=size, replace=replace, p=p)


def l2_norm(x):
    """sgl.py:25-27."""
    return (x.T / torch.norm(x, 2, 1)).T


class create_bpr_loss:
    """sgl.py:188-226 as a name: the loss itself is the BPR stage of ``csrc/sgl.hip``."""

    def __init__(self, reg):
        self.reg = reg


class calc_ssl_loss_v2:
    """sgl.py:82-145 as a name: the loss itself is the InfoNCE kernels of ``csrc/sgl.hip``."""

    def __init__(self, ssl_reg, ssl_temp, ssl_mode):
        self.ssl_reg, self.ssl_temp, self.ssl_mode = ssl_reg, ssl_temp, ssl_mode


def _coo_of(adj):
    """``(rows, cols, vals, shape)`` as CPU tensors of a scipy sparse matrix or a torch sparse tensor."""
    if torch.is_tensor(adj):
        a = adj.cpu()
        idx = a._indices()
        return idx[0].to(torch.int64), idx[1].to(torch.int64), a._values().to(torch.float32), tuple(a.shape)
    coo = adj.tocoo()
    return (torch.from_numpy(np.asarray(coo.row, dtype=np.int64)), torch.from_numpy(np.asarray(coo.col, dtype=np.int64)),
            torch.from_numpy(np.asarray(coo.data, dtype=np.float32)), tuple(coo.shape))


def symmetric_structure(users, items, n_users, n_items):
    """The symmetric bipartite CSR of a list of interactions: ``(rowptr, col, edge_inter)`` (int64, int32, int32 CPU
    tensors), ``edge_inter[e]`` = the interaction both directions of an edge came from.  Raises ``ValueError`` for
    repeated (user, item) pairs: the reference would sum them into one entry of value 2 while dropping them one by one;
    a CSR edge has one keep byte."""
    u = torch.as_tensor(np.asarray(users), dtype=torch.int64).reshape(-1)
    i = torch.as_tensor(np.asarray(items), dtype=torch.int64).reshape(-1)
    if u.numel() != i.numel():
        raise ValueError("users and items differ in length")
    if u.numel() and (int(u.min()) < 0 or int(u.max()) >= n_users or int(i.min()) < 0 or int(i.max()) >= n_items):
        raise ValueError("an interaction lies outside n_users x n_items")
    key = torch.sort(u * n_items + i).values
    if key.numel() > 1 and bool((key[1:] == key[:-1]).any()):
        raise ValueError("the loader holds repeated (user, item) pairs; pass every interaction once")
    N, n = n_users + n_items, u.numel()
    rows, cols = torch.cat([u, n_users + i]), torch.cat([n_users + i, u])
    inter = torch.cat([torch.arange(n), torch.arange(n)])
    order = torch.argsort(rows * N + cols, stable=True)
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=N), 0)
    return rowptr, cols[order].to(torch.int32), inter[order].to(torch.int32)


class SubMats:
    """What ``sub_mat_refresher`` hands out: the sub-graphs' shared CSR structure on the device and per view and layer
    a value array over its edges (``vals[view][layer]``; node / edge dropout hold one array per view L times)."""

    def __init__(self, rowptr, col, vals, n_rows, keep=None):
        self.rowptr, self.col, self.vals, self.n_rows = rowptr, col, vals, n_rows
        self.nnz = int(col.numel())
        self.keep = keep            # [view][layer] keep bytes per interaction (edge dropout / random walk), or None
        on_gpu = rowptr.device.type == "cuda" and self.nnz > 0
        self.slice_row = _slice_rows(rowptr, col, col, n_rows, self.nnz) if on_gpu else None   # (col: any edge array)

    def csr(self):
        return _lib.Csr(self.rowptr.data_ptr(), self.col.data_ptr() if self.nnz else None, None, None, self.n_rows,
                        self.nnz, _lib.ptr(self.slice_row))


class SGL(_FlatModel):
    """sgl.py:229-405."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.n_users, self.n_items = int(config["n_users"]), int(config["n_items"])
        self.emb_dim = self.embe_dim = int(config["emb_dim"])
        self.n_layers = int(config["n_layers"])
        if not 1 <= self.emb_dim <= 256:
            raise ValueError(f"emb_dim {self.emb_dim}: 1 .. 256 are supported")
        if not 0 <= self.n_layers <= MAX_LAYERS:
            raise ValueError(f"n_layers {self.n_layers}: 0 .. {MAX_LAYERS} are supported")
        self.ssl_mode = config["ssl_mode"]
        if self.ssl_mode == "merge":
            raise ValueError("ssl_mode 'merge' is not supported: the reference itself always raises there (sgl.py:168, "
                             "`batch_items, _ = torch.unique(pos_items)` unpacks a tensor)")
        if self.ssl_mode not in SSL_MODES:
            raise ValueError("Invalid ssl_mode!")
        self.pretrain = config["pretrain"]
        self.aug_type = int(config["aug_type"])
        self.regs, self.ssl_reg, self.ssl_temp = float(config["regs"]), float(config["ssl_reg"]), float(config["ssl_temp"])
        if not self.ssl_temp > 0:
            raise ValueError(f"ssl_temp {self.ssl_temp}: must be positive")
        self.norm_adj = config["norm_adj"]
        self.create_bpr_loss = create_bpr_loss(self.regs)
        self.calc_ssl_loss_v2 = calc_ssl_loss_v2(self.ssl_reg, self.ssl_temp, self.ssl_mode)
        v = self._build([("user_embedding", (self.n_users, self.emb_dim)), ("item_embedding", (self.n_items, self.emb_dim))])
        # RNG order of sgl.py:257-264
        torch.nn.init.xavier_uniform_(v["user_embedding"])
        torch.nn.init.xavier_uniform_(v["item_embedding"])
        self.user_embedding = Parameter(v["user_embedding"], requires_grad=False)
        self.item_embedding = Parameter(v["item_embedding"], requires_grad=False)
        self.n_splits = int(config["ssl_splits"]) if "ssl_splits" in config else 0   # 0: chosen from the shape
        self._graph = None
        self._ws = None
        self._weights_clock = 0      # bumped by the engine with every optimizer step
        self._pool_key = None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._weights_clock += 1         # predict's cached propagation is stale
        return out

    @property
    def ssl_sides(self):
        return 0 if self.pretrain else SSL_MODES[self.ssl_mode]

    # ---- graph + workspace ------------------------------------------------------------------------
    def graph(self):
        """CSR and transposed CSR of norm_adj on the parameters' device (built once)."""
        dev = self._flat.device
        if self._graph is not None and self._graph["dev"] == dev:
            return self._graph
        rows, cols, vals, shape = _coo_of(self.norm_adj)
        N = self.n_users + self.n_items
        if shape != (N, N):
            raise ValueError(f"norm_adj is {shape}, expected ({N}, {N})")
        coo_to_csr_maps(rows, cols, N)           # repeated coordinates raise
        rp, c, v, _ = _csr_from_coo(rows, cols, vals, N, dev)
        rpt, ct, vt, _ = _csr_from_coo(cols, rows, vals, N, dev)
        nnz = int(vals.numel())
        self._graph = {"dev": dev, "nnz": nnz, "rowptr": rp, "col": c, "val": v, "rowptr_t": rpt, "col_t": ct, "val_t": vt}
        if dev.type == "cuda":
            self._graph["slice_row"] = _slice_rows(rp, c, v, N, nnz)
            self._graph["slice_row_t"] = _slice_rows(rpt, ct, vt, N, nnz)
        return self._graph

    def workspace(self, batch=0):
        dev = self._flat.device
        lib = _lib.load()
        N = self.n_users + self.n_items
        if self._ws is None or self._ws["dev"] != dev:
            self._ws = {"dev": dev, "batch_ws": None,
                        "ws": torch.zeros(int(lib.hiprec_sgl_ws_floats(N, self.emb_dim)), dtype=torch.float32, device=dev)}
        if batch:
            self._ws["batch_ws"] = _lib.grow(self._ws["batch_ws"], int(lib.hiprec_sgl_batch_ws_floats(batch, self.emb_dim)),
                                             torch.float32, dev)
        return self._ws

    def plan(self, g_flat=None, sub=None, batch=0):
        gr, ws = self.graph(), self.workspace(batch)
        N = self.n_users + self.n_items
        p = _lib.SglPlan()
        p.a = _lib.Csr(gr["rowptr"].data_ptr(), gr["col"].data_ptr(), gr["val"].data_ptr(), None, N, gr["nnz"],
                       _lib.ptr(gr.get("slice_row")))
        p.at = _lib.Csr(gr["rowptr_t"].data_ptr(), gr["col_t"].data_ptr(), gr["val_t"].data_ptr(), None, N, gr["nnz"],
                        _lib.ptr(gr.get("slice_row_t")))
        p.n_users, p.n_items, p.dim, p.n_layers = self.n_users, self.n_items, self.emb_dim, self.n_layers
        p.ssl_sides, p.n_splits = (self.ssl_sides if sub is not None else 0), self.n_splits
        p.regs, p.ssl_reg, p.ssl_temp = self.regs, self.ssl_reg, self.ssl_temp
        p.e0 = self._flat.data_ptr()
        p.g = None if g_flat is None else g_flat.data_ptr()
        p.ws, p.ws_floats = ws["ws"].data_ptr(), ws["ws"].numel()
        if batch:
            p.batch_ws, p.batch_ws_floats = ws["batch_ws"].data_ptr(), ws["batch_ws"].numel()
        if sub is not None and p.ssl_sides:
            if sub.n_rows != N or sub.rowptr.device != self._flat.device:
                raise ValueError("the sub-graphs belong to another graph size or device")
            p.s = sub.csr()
            for v in range(2):
                for l in range(self.n_layers):
                    p.sub_val[v][l] = sub.vals[v][l].data_ptr() if sub.nnz else None
        return p

    # ---- reference API ----------------------------------------------------------------------------
    def _pooled(self):
        """The main view's hop sum from the current weights (cached until they change): ``[N, D]`` view of the
        workspace; the layer mean is this over ``L + 1``."""
        lib = self._require_hip()
        key = (self._flat.data_ptr(), self._flat._version, self._weights_clock)
        N, D = self.n_users + self.n_items, self.emb_dim
        if key != self._pool_key:
            plan = self.plan()
            _lib.check(lib.hiprec_sgl_propagate(ctypes.byref(plan), _lib.stream_ptr(self._flat.device)))
            self._pool_key = key
        return self._ws["ws"][: N * D].view(N, D)

    def ranking_factors(self):
        """``(U, I, alpha, None)`` for full-catalogue ranking: eval propagation over ``norm_adj`` only; the two halves
        of the hop sum, ``alpha = 1 / (L + 1)^2`` (the mean on both sides of the dot product)."""
        pool = self._pooled()
        return pool[: self.n_users], pool[self.n_users:], 1.0 / float(self.n_layers + 1) ** 2, None

    def predict(self, users, items):
        """sgl.py:396-405 on the CURRENT weights: dot product of the mean-pooled rows, no sigmoid."""
        lib = self._require_hip()
        dev = self._flat.device
        users_t, items_t = index_tensor(users, dev), index_tensor(items, dev)
        if users_t.numel() != items_t.numel():
            raise ValueError("users and items differ in length")
        self._pooled()
        stats = self._device_stats()
        plan = self.plan()
        scores = torch.empty(users_t.numel(), dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_sgl_predict(ctypes.byref(plan), _lib.ptr(users_t), _lib.ptr(items_t), users_t.numel(),
                                          _lib.ptr(scores), _lib.ptr(stats), _lib.stream_ptr(dev)))
        self._check_status()
        return scores

    def last_allnodes(self):
        """What the all-nodes side of the last training step wrote: ``(d2 [N, D], logsum [2, B])`` -- the gradient
        with respect to view 2's hop sum (every row stored once, no atomics) and the per-row log-sums of both sides."""
        N, D = self.n_users + self.n_items, self.emb_dim
        ws = self._ws
        B = self._last_batch
        return ws["ws"][5 * N * D: 6 * N * D].view(N, D), ws["batch_ws"][: 2 * B].view(2, B)


class SGLEngine(FlatModelEngine):
    """sgl.py:408-585."""

    def __init__(self, config):
        self.config = config
        m = config["model"]
        self.norm_adj = m["norm_adj"]
        self.n_layers = int(m["n_layers"])
        self.aug_type = int(m["aug_type"])
        if self.aug_type not in (0, 1, 2):
            raise ValueError(f"aug_type {self.aug_type}: 0 (node dropout), 1 (edge dropout) or 2 (random walk)")
        self.sub_rng = m["sub_rng"] if "sub_rng" in m else "numpy"
        if self.sub_rng not in ("numpy", "device"):
            raise ValueError(f"unknown sub_rng {self.sub_rng!r}: 'numpy' or 'device'")
        self.sub_seed = int(m["sub_seed"]) if "sub_seed" in m else 0
        self.model = SGL(m)
        super(SGLEngine, self).__init__(config)
        self.model.to(self.device)
        self._sub = None
        self._structure = None
        self._refreshes = 0

    def _alloc_extra(self, lib, device):
        self._parts = torch.zeros(4, dtype=torch.float32, device=device)

    # ---- sub-graphs -------------------------------------------------------------------------------
    def randint_choice(self, high, size=None, replace=True, p=None, exclusion=None):
        """sgl.py:529-543."""
        return randint_choice(high, size, replace, p, exclusion)

    def _interactions(self, train_loader):
        user_np = train_loader.dataset.user_tensor.cpu().numpy()
        item_np = train_loader.dataset.pos_item_tensor.cpu().numpy()
        return user_np, item_np

    def _loader_structure(self, train_loader):
        """The symmetric CSR of the loader's interactions on the device, built once per loader content."""
        m = self.model
        dev = m.flat.device
        ut, it = train_loader.dataset.user_tensor, train_loader.dataset.pos_item_tensor
        key = (ut.data_ptr(), ut._version, it.data_ptr(), it._version, ut.numel(), str(dev))
        if self._structure is None or self._structure["key"] != key:
            user_np, item_np = self._interactions(train_loader)
            rowptr, col, inter = symmetric_structure(user_np, item_np, m.n_users, m.n_items)
            self._structure = {"key": key, "rowptr": rowptr.to(dev), "col": col.to(dev), "inter": inter.to(dev),
                               "n": int(user_np.size)}
        return self._structure

    def _augments(self):
        m = self.config["model"]
        return bool(m["is_subgraph"]) and self.aug_type in (0, 1, 2) and float(m["ssl_ratio"]) > 0

    def draw_keep(self, n_inter):
        """The keep sets of one refresh, in the reference's call order (sgl.py:545-580: view 1 then view 2, per layer for
        the random walk): per (view, layer) a uint8 keep array over the interactions (edge dropout / random walk), a
        pair of node keep arrays (node dropout) or None (nothing dropped)."""
        self._refreshes += 1
        calls = [(v, l) for l in range(self.n_layers if self.aug_type == 2 else 1) for v in range(2)]
        out = [[None] * max(self.n_layers, 1) for _ in range(2)]
        for n_call, (v, l) in enumerate(calls):
            drawn = self._draw_one(n_inter, n_call)
            for ll in (range(max(self.n_layers, 1)) if self.aug_type != 2 else (l,)):
                out[v][ll] = drawn
        return out

    def _draw_one(self, n_inter, n_call):
        """The keep set of ONE create_sgl_mat call (sgl.py:474-512), the ``n_call``-th of its refresh."""
        m = self.model
        ratio = float(self.config["model"]["ssl_ratio"])
        dev = m.flat.device
        if not self._augments():
            return None
        if self.aug_type == 0:
            drawn = []
            for side, n in enumerate((m.n_users, m.n_items)):
                keep = torch.ones(n, dtype=torch.uint8)
                k = int(n * ratio)
                if self.sub_rng == "numpy":
                    drop = torch.from_numpy(np.asarray(self.randint_choice(n, size=k, replace=False), dtype=np.int64))
                else:
                    drop = self._device_perm(n, 2 * n_call + side)[:k].cpu()
                keep[drop] = 0
                drawn.append(keep.to(dev))
            return tuple(drawn)
        k = int(n_inter * (1 - ratio))
        if self.sub_rng == "numpy":
            idx = torch.from_numpy(np.asarray(self.randint_choice(n_inter, size=k, replace=False), dtype=np.int64))
        else:
            idx = self._device_perm(n_inter, n_call)[:k]
        drawn = torch.zeros(n_inter, dtype=torch.uint8, device=dev)
        drawn[idx.to(dev)] = 1
        return drawn

    def _device_perm(self, n, call):
        lib = self.require_hip()
        dev = self.model.flat.device
        out = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        seed = (self.sub_seed * 0x9E3779B97F4A7C15 + self._refreshes * 1000003 + call) % (1 << 64)
        _lib.check(lib.hiprec_random_permutation(_lib.ptr(out), n, seed, _lib.stream_ptr(dev)))
        return out[:n]

    def sub_values(self, rowptr, col, inter, keep):
        """``hiprec_sgl_sub_values`` for one keep set (see ``draw_keep``): ``(val [nnz], deg [N])`` on the device."""
        lib = self.require_hip()
        m = self.model
        dev = m.flat.device
        N, nnz = m.n_users + m.n_items, int(col.numel())
        val = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
        deg = torch.empty(N, dtype=torch.float32, device=dev)
        csr = _lib.Csr(rowptr.data_ptr(), col.data_ptr() if nnz else None, None, None, N, nnz, None)
        k_e, k_u, k_i = (None, keep[0], keep[1]) if isinstance(keep, tuple) else (keep, None, None)
        _lib.check(lib.hiprec_sgl_sub_values(ctypes.byref(csr), _lib.ptr(inter), _lib.ptr(k_e), _lib.ptr(k_u), _lib.ptr(k_i),
                                             m.n_users, _lib.ptr(deg), _lib.ptr(val), _lib.stream_ptr(dev)))
        return val, deg

    def sub_mat_refresher(self, train_loader):
        """sgl.py:545-580: a fresh pair of sub-graphs (one pair per layer for the random walk), as a ``SubMats`` handle
        whose value arrays live on the device."""
        self._setup()
        m = self.model
        s = self._loader_structure(train_loader)
        keeps = self.draw_keep(s["n"])
        vals = [[None] * max(self.n_layers, 1) for _ in range(2)]
        made = {}                    # one value array per keep set (None -- nothing dropped -- is one set)
        for v in range(2):
            for l in range(max(self.n_layers, 1)):
                k = keeps[v][l]
                if id(k) not in made:
                    made[id(k)] = self.sub_values(s["rowptr"], s["col"], s["inter"], k)[0]
                vals[v][l] = made[id(k)]
        return SubMats(s["rowptr"], s["col"], vals, m.n_users + m.n_items, keeps)

    def create_sgl_mat(self, train_loader):
        """sgl.py:464-527: ONE augmented, normalised adjacency as a scipy CSR matrix (one set of draws)."""
        import scipy.sparse as sp

        m = self.model
        s = self._loader_structure(train_loader)
        self._refreshes += 1
        keep = self._draw_one(s["n"], 0)
        val, _ = self.sub_values(s["rowptr"], s["col"], s["inter"], keep)
        N = m.n_users + m.n_items
        mat = sp.csr_matrix((val[: s["col"].numel()].cpu().numpy(), s["col"].cpu().numpy(), s["rowptr"].cpu().numpy()),
                            shape=(N, N))
        mat.eliminate_zeros()
        return mat

    def from_reference_dict(self, sub_mat):
        """The reference's own ``sub_mat`` dict (``adj_indices_sub1`` ... or the per-layer keys) as a ``SubMats`` handle:
        one CSR structure over the union of all its coordinates, every view's values scattered into it."""
        m = self.model
        dev = m.flat.device
        N, L = m.n_users + m.n_items, max(self.n_layers, 1)
        names = [[("sub%d" % (v + 1)) + ("%d" % (l + 1) if self.aug_type == 2 else "") for l in range(L)] for v in range(2)]
        coords = {}
        for v in range(2):
            for l in range(L):
                if names[v][l] in coords:
                    continue
                idx = np.asarray(sub_mat["adj_indices_" + names[v][l]], dtype=np.int64).reshape(2, -1)
                shape = tuple(sub_mat["adj_shape_" + names[v][l]])
                if shape != (N, N):
                    raise ValueError(f"sub-matrix {names[v][l]} is {shape}, expected ({N}, {N})")
                coords[names[v][l]] = (idx[0] * N + idx[1], np.asarray(sub_mat["adj_values_" + names[v][l]], dtype=np.float32))
        keys = np.unique(np.concatenate([k for k, _ in coords.values()]))
        rows, cols = keys // N, keys % N
        rowptr = torch.zeros(N + 1, dtype=torch.int64)
        rowptr[1:] = torch.cumsum(torch.bincount(torch.from_numpy(rows), minlength=N), 0)
        dense = {}
        for name, (k, v) in coords.items():
            if np.unique(k).size != k.size:
                raise ValueError(f"sub-matrix {name} holds repeated coordinates")
            val = np.zeros(max(keys.size, 1), dtype=np.float32)
            val[np.searchsorted(keys, k)] = v
            dense[name] = torch.from_numpy(val).to(dev)
        vals = [[dense[names[v][l]] for l in range(L)] for v in range(2)]
        return SubMats(rowptr.to(dev), torch.from_numpy(cols.astype(np.int32)).to(dev), vals, N)

    def _as_handle(self, sub_mat):
        if isinstance(sub_mat, SubMats) or sub_mat is None:
            return sub_mat
        if not isinstance(sub_mat, dict):
            raise TypeError("sub_mat: what sub_mat_refresher returned, or the reference's dict")
        if self.model.pretrain:
            return None
        dev = self.model.flat.device
        cached = sub_mat.get("_hiprec")          # converted once per dict (the reference adds its own tensors to it too)
        if cached is None or cached.rowptr.device != dev:
            cached = sub_mat["_hiprec"] = self.from_reference_dict(sub_mat)
        return cached

    # ---- the step ---------------------------------------------------------------------------------
    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 3:
            raise ValueError("SGL batches are (users, pos_items, neg_items)")
        users, pos, neg = (index_tensor(x, dev) for x in batch_data)
        B = users.numel()
        if not (pos.numel() == B and neg.numel() == B):
            raise ValueError("batch tensors differ in length")
        if B == 0:
            raise ValueError("empty batch")
        sub = None if m.pretrain else self._sub
        if sub is None and not m.pretrain:
            raise ValueError("no sub-graphs: pass what sub_mat_refresher returned (or the reference's dict)")
        plan = m.plan(self._g_flat, sub, B)
        m._last_batch = B
        m._pool_key = None                   # the training forward overwrites the pooled main view
        _lib.check(lib.hiprec_sgl_grad(ctypes.byref(plan), _lib.ptr(users), _lib.ptr(pos), _lib.ptr(neg), B,
                                       _lib.ptr(self._parts), _lib.ptr(self._stats), _lib.ptr(self._scratch),
                                       self._scratch.numel(), _lib.stream_ptr(dev)))

    def _enqueue_opt(self, *a, **k):
        super()._enqueue_opt(*a, **k)
        self.model._weights_clock += 1

    def last_losses(self):
        """``(bpr, emb, ssl)`` of the last step (one host sync)."""
        p = self._parts.cpu().numpy()
        return float(p[0]), float(p[1]), float(p[2])

    def backward_only(self, sub_mat, batch_data):
        """zero_grad + forward + loss + backward without the optimizer step: ``(loss, grads)``."""
        self._setup()
        self._sub = self._as_handle(sub_mat)
        return super().backward_only(batch_data)

    def train_single_batch(self, sub_mat, batch_data):
        """sgl.py:423-445: one step, returns ``sl_loss + emb_loss + ssl_loss`` as a float."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._setup()
        self._sub = self._as_handle(sub_mat)
        self._enqueue_step(batch_data)
        return self._sync_stats().loss

    def train_an_epoch(self, train_loader, epoch_id):
        """sgl.py:447-462: one refresh, then every batch; prints the last batch's loss, logs the epoch sum."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        self._sub = None if self.model.pretrain else self.sub_mat_refresher(train_loader)
        st = self._run_epoch(train_loader)
        print("[Training Epoch {}], Loss {}".format(epoch_id, st.loss))
        self.writer.add_scalar("model/loss", st.loss_sum, epoch_id)
