"""Drop-in ``LightGCN`` / ``LightGCNEngine`` / ``GraphConv`` for beta_rec/models/mixgcf.py on libhiprec.so, exported by
the package as ``MixGCF`` / ``MixGCFEngine``.

Interface parity (file:line = beta_rec/models/mixgcf.py): ``LightGCN(config, norm_adj)`` :70-157 (``forward() -> (user,
item)`` hop stacks ``[*, L + 1, D]``, ``pooling``, ``predict``), ``LightGCNEngine(config)`` :160-286
(``train_single_batch``, ``train_an_epoch``).  Same config keys (``n_users n_items emb_dim pool context_hops mess_dropout
mess_dropout_rate edge_dropout edge_dropout_rate norm_adj l2 n_negs ns K optimizer lr device_str``), same ``state_dict``
keys, same initial weights for the same torch seed.

Kept from the reference on purpose:
* edge dropout keeps edge ``e`` iff ``floor(rate + r_e) == 1``: a share ``rate`` of the edges SURVIVES and is scaled by
  ``1 / (1 - rate)``; ``r`` is drawn in the order of ``norm_adj._indices()`` as passed (the reference never coalesces);
* one mixing seed per (row, hop), shared by all candidates and channels, a fresh draw for every ``k``;
* the L2 term acts on the MIXED hop-0 negative.
Not kept:
* the reference's ``train_single_batch`` returns the loss tensor and never calls ``backward()`` or
  ``optimizer.step()``, so no weight ever moves; the mirror takes the gradient of exactly that loss and runs the engine's
  optimizer, and returns the loss as a float;
* an unknown ``pool`` is treated as ``final`` by the reference; the mirror raises ``ValueError``;
* ``log(1 + sum exp(x))`` is computed shifted by its largest argument (the reference's form overflows beyond x ~ 88).

Extensions: ``dropout_rng`` / ``seed_rng`` = ``"torch_cpu"`` (default) replay the reference's CPU draws (per hop the
edge ``rand(nnz)`` then the message ``bernoulli_``, then per ``k`` the seed ``rand(B, 1, L + 1, 1)``); ``"device"`` draws
on the GPU from ``dropout_seed``.  ``last_choice()``, ``last_seeds()``, ``last_edge_keep(l)`` and ``last_mess_keep(l)``
hand out what the last step used.

Propagation, sampler, loss and backward are ``csrc/mixgcf.hip``.  There is no CPU path.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor
from .lightgcn import _csr_from_coo, _slice_rows

POOLS = ("concat", "mean", "sum", "final")
MAX_HOPS = _lib.MIXGCF_MAX_HOPS


def coo_to_csr_maps(rows, cols, n):
    """For a COO edge list in ANY order without repeated coordinates: ``(order, order_t, eid_t)`` -- the COO position of
    every forward-CSR edge, of every transposed-CSR edge, and the forward-CSR edge number of every transposed-CSR edge.
    Raises ``ValueError`` for repeated coordinates (the reference would sum them inside ``torch.sparse.mm`` while
    dropping them one by one; a CSR edge has one keep byte)."""
    rows, cols = rows.to(torch.int64), cols.to(torch.int64)
    key = rows * n + cols
    order = torch.argsort(key, stable=True)
    sk = key[order]
    if sk.numel() > 1 and bool((sk[1:] == sk[:-1]).any()):
        raise ValueError("norm_adj holds repeated coordinates; pass a tensor with one value per (row, col)")
    order_t = torch.argsort(cols * n + rows, stable=True)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel())
    return order, order_t, inv[order_t]


class GraphConv(nn.Module):
    """mixgcf.py:7-67: a handle on the owning model's propagation (``model.gcn``)."""

    def __init__(self, model):
        super().__init__()
        object.__setattr__(self, "_model", model)   # (not a submodule: the model owns this handle)
        self.n_hops, self.n_users = model.context_hops, model.n_users
        self.edge_dropout_rate, self.mess_dropout_rate = model.edge_dropout_rate, model.mess_dropout_rate

    def forward(self, user_embed=None, item_embed=None, mess_dropout=True, edge_dropout=True):
        """The hop stacks of the model's own tables (the reference always passes those)."""
        return self._model._stacks(bool(mess_dropout), bool(edge_dropout))


class LightGCN(_FlatModel):
    """mixgcf.py:70-157."""

    def __init__(self, config, norm_adj):
        super().__init__()
        self.config = config
        self.n_users, self.n_items = int(config["n_users"]), int(config["n_items"])
        self.emb_dim = int(config["emb_dim"])
        self.pool = config["pool"]
        if self.pool not in POOLS:
            raise ValueError(f"pool {self.pool!r}: one of {POOLS} (the reference silently treats anything else as 'final')")
        self.context_hops = int(config["context_hops"])
        if not 0 <= self.context_hops <= MAX_HOPS:
            raise ValueError(f"context_hops {self.context_hops}: 0 .. {MAX_HOPS} are supported")
        if not 1 <= self.emb_dim <= 256:
            raise ValueError(f"emb_dim {self.emb_dim}: 1 .. 256 are supported")
        self.mess_dropout = bool(config["mess_dropout"])
        self.mess_dropout_rate = float(config["mess_dropout_rate"])
        self.edge_dropout = bool(config["edge_dropout"])
        self.edge_dropout_rate = float(config["edge_dropout_rate"])
        if self.mess_dropout and not 0.0 <= self.mess_dropout_rate < 1.0:
            raise ValueError(f"mess_dropout_rate {self.mess_dropout_rate}: must lie in [0, 1)")
        if self.edge_dropout and not 0.0 <= self.edge_dropout_rate < 1.0:
            raise ValueError(f"edge_dropout_rate {self.edge_dropout_rate}: must lie in [0, 1)")
        self.norm_adj = norm_adj
        v = self._build([("user_embedding.weight", (self.n_users, self.emb_dim)),
                         ("item_embedding.weight", (self.n_items, self.emb_dim))])
        # RNG order of mixgcf.py:90-99: two nn.Embedding (N(0,1)) then xavier_uniform_ x2
        v["user_embedding.weight"].normal_(0, 1)
        v["item_embedding.weight"].normal_(0, 1)
        nn.init.xavier_uniform_(v["user_embedding.weight"])
        nn.init.xavier_uniform_(v["item_embedding.weight"])
        self.user_embedding = _ParamView(v["user_embedding.weight"])
        self.item_embedding = _ParamView(v["item_embedding.weight"])
        self.dropout_rng = config["dropout_rng"] if "dropout_rng" in config else "torch_cpu"
        self.seed_rng = config["seed_rng"] if "seed_rng" in config else "torch_cpu"
        for name, val in (("dropout_rng", self.dropout_rng), ("seed_rng", self.seed_rng)):
            if val not in ("torch_cpu", "device"):
                raise ValueError(f"unknown {name} {val!r}: 'torch_cpu' or 'device'")
        self.dropout_seed = int(config["dropout_seed"]) if "dropout_seed" in config else 0
        self._graph = None
        self._ws = None
        self._step = 0
        self._masks = ([None] * MAX_HOPS, [None] * MAX_HOPS)
        self._given = None
        self.gcn = GraphConv(self)

    # ---- graph + workspace ------------------------------------------------------------------------
    def graph(self):
        """CSR and transposed CSR of norm_adj on the parameters' device (built once), and ``order``: the position in
        ``norm_adj._indices()`` of every CSR edge -- the order the reference draws its edge mask in."""
        dev = self._flat.device
        if self._graph is not None and self._graph["dev"] == dev:
            return self._graph
        adj = self.norm_adj.cpu()
        N = self.n_users + self.n_items
        if tuple(adj.shape) != (N, N):
            raise ValueError(f"norm_adj is {tuple(adj.shape)}, expected ({N}, {N})")
        idx, vals = adj._indices(), adj._values().to(torch.float32)
        rows, cols = idx[0], idx[1]
        order, _, eid_t = coo_to_csr_maps(rows, cols, N)
        rp, c, v, _ = _csr_from_coo(rows, cols, vals, N, dev)
        rpt, ct, vt, _ = _csr_from_coo(cols, rows, vals, N, dev)
        nnz = int(vals.numel())
        self._graph = {"dev": dev, "nnz": nnz, "rowptr": rp, "col": c, "val": v, "rowptr_t": rpt, "col_t": ct,
                       "val_t": vt, "eid_t": eid_t.to(torch.int32).to(dev), "order": order}
        if dev.type == "cuda":
            self._graph["slice_row"] = _slice_rows(rp, c, v, N, nnz)
            self._graph["slice_row_t"] = _slice_rows(rpt, ct, vt, N, nnz)
        return self._graph

    def workspace(self):
        dev = self._flat.device
        if self._ws is not None and self._ws["dev"] == dev:
            return self._ws
        N, D, L = self.n_users + self.n_items, self.emb_dim, self.context_hops
        g = self.graph()
        self._ws = {"dev": dev,
                    # hop tables 1 .. L, then their gradient tables: one fill per step
                    "zero_ws": torch.zeros(max(2 * L * N * D, 1), dtype=torch.float32, device=dev),
                    "edge_keep": [torch.ones(max(g["nnz"], 1), dtype=torch.uint8, device=dev) for _ in range(L)],
                    "mess_keep": [torch.ones(N * D, dtype=torch.uint8, device=dev) for _ in range(L)]}
        return self._ws

    def plan(self, g_flat=None, l2=0.0, n_negs=1, k_neg=1, rns=False, masks=None):
        gr, ws = self.graph(), self.workspace()
        N = self.n_users + self.n_items
        p = _lib.MixGcfPlan()
        p.a = _lib.Csr(gr["rowptr"].data_ptr(), gr["col"].data_ptr(), gr["val"].data_ptr(), None, N, gr["nnz"],
                       _lib.ptr(gr.get("slice_row")))
        p.at = _lib.Csr(gr["rowptr_t"].data_ptr(), gr["col_t"].data_ptr(), gr["val_t"].data_ptr(),
                        gr["eid_t"].data_ptr(), N, gr["nnz"], _lib.ptr(gr.get("slice_row_t")))
        p.n_users, p.n_items, p.dim, p.n_hops = self.n_users, self.n_items, self.emb_dim, self.context_hops
        p.pool, p.rns, p.n_negs, p.k_neg = _lib.MIXGCF_POOLS[self.pool], int(bool(rns)), int(n_negs), int(k_neg)
        p.l2 = float(l2)
        p.edge_scale = 1.0 / (1.0 - self.edge_dropout_rate) if self.edge_dropout else 1.0
        p.mess_scale = 1.0 / (1.0 - self.mess_dropout_rate) if self.mess_dropout else 1.0
        p.e0 = self._flat.data_ptr()
        p.g = None if g_flat is None else g_flat.data_ptr()
        p.zero_ws, p.zero_ws_floats = ws["zero_ws"].data_ptr(), ws["zero_ws"].numel()
        edge, mess = masks if masks is not None else ([None] * MAX_HOPS, [None] * MAX_HOPS)
        for l in range(self.context_hops):
            p.edge_keep[l] = None if edge[l] is None else edge[l].data_ptr()
            p.mess_keep[l] = None if mess[l] is None else mess[l].data_ptr()
        return p

    def draw_masks(self, mess_dropout=None, edge_dropout=None):
        """Per hop the edge and message keep bytes of one training propagation, ``(edge[l], mess[l])`` with None where a
        hop has no such dropout.  ``torch_cpu``: the reference's draws in the reference's order (mixgcf.py:31-44, :52-63)."""
        lib = self._require_hip()
        ws, gr = self.workspace(), self.graph()
        mess_on = self.mess_dropout if mess_dropout is None else mess_dropout
        edge_on = self.edge_dropout if edge_dropout is None else edge_dropout
        mess_on = mess_on and self.mess_dropout_rate > 0      # at::dropout with p == 0 returns its input: no draw
        N, D, L = self.n_users + self.n_items, self.emb_dim, self.context_hops
        self._step += 1
        st = _lib.stream_ptr(self._flat.device)
        edge, mess = [None] * MAX_HOPS, [None] * MAX_HOPS
        given, self._given = self._given, None
        for l in range(L):
            if given is not None:         # the caller's masks for this one propagation (LightGCNEngine.give_draws)
                if given[0] is not None:
                    edge[l] = ws["edge_keep"][l]
                    mask = torch.as_tensor(given[0][l]).reshape(-1)
                    edge[l][: gr["nnz"]].copy_(mask[gr["order"]].to(torch.uint8))
                if given[1] is not None:
                    mess[l] = ws["mess_keep"][l]
                    mess[l].copy_(torch.as_tensor(given[1][l]).reshape(-1).to(torch.uint8))
                continue
            if edge_on:
                buf = ws["edge_keep"][l]
                if self.dropout_rng == "torch_cpu":
                    random_tensor = self.edge_dropout_rate + torch.rand(gr["nnz"])
                    mask = torch.floor(random_tensor).type(torch.bool)          # in COO order
                    buf[: gr["nnz"]].copy_(mask[gr["order"]].to(torch.uint8))
                else:
                    _lib.check(lib.hiprec_edge_dropout_mask(_lib.ptr(buf), gr["nnz"], self.edge_dropout_rate,
                                                            self.dropout_seed, 2 * (self._step * MAX_HOPS + l), st))
                edge[l] = buf
            if mess_on:
                buf = ws["mess_keep"][l]
                if self.dropout_rng == "torch_cpu":
                    buf.copy_(torch.empty(N, D).bernoulli_(1 - self.mess_dropout_rate).to(torch.uint8).reshape(-1))
                else:
                    _lib.check(lib.hiprec_edge_dropout_mask(_lib.ptr(buf), N * D, 1.0 - self.mess_dropout_rate,
                                                            self.dropout_seed, 2 * (self._step * MAX_HOPS + l) + 1, st))
                mess[l] = buf
        self._masks = (edge, mess)
        return self._masks

    def last_edge_keep(self, hop):
        """Keep bytes (uint8 [nnz], forward CSR order) of hop ``hop -> hop + 1`` of the last training propagation, or
        None when that hop dropped no edges."""
        m = self._masks[0][hop]
        return None if m is None else m[: self.graph()["nnz"]]

    def last_mess_keep(self, hop):
        """Keep bytes (uint8 [N, D]) of hop ``hop + 1``'s message dropout in the last training propagation, or None."""
        m = self._masks[1][hop]
        return None if m is None else m.view(self.n_users + self.n_items, self.emb_dim)

    # ---- reference API ----------------------------------------------------------------------------
    def _propagate(self, mess_dropout, edge_dropout):
        lib = self._require_hip()
        train = self.training and (mess_dropout or edge_dropout)
        masks = self.draw_masks(mess_dropout, edge_dropout) if train else None
        plan = self.plan(masks=masks)
        _lib.check(lib.hiprec_mixgcf_propagate(ctypes.byref(plan), 1 if train else 0, _lib.stream_ptr(self._flat.device)))

    def _stacks(self, mess_dropout, edge_dropout):
        self._propagate(mess_dropout, edge_dropout)
        N, D, L = self.n_users + self.n_items, self.emb_dim, self.context_hops
        hops = [self._flat[: N * D].view(N, D)] + [self._ws["zero_ws"][l * N * D:(l + 1) * N * D].view(N, D)
                                                   for l in range(L)]
        embs = torch.stack(hops, dim=1)
        return embs[: self.n_users], embs[self.n_users:]

    def forward(self):
        """mixgcf.py:112-121 without autograd: the two ``[*, L + 1, D]`` hop stacks; dropout follows the config in
        training mode, as ``nn.Dropout`` and the reference's flags do."""
        return self._stacks(self.mess_dropout, self.edge_dropout)

    def pooling(self, embeddings):
        """mixgcf.py:123-133."""
        if self.pool == "mean":
            return embeddings.mean(dim=1)
        if self.pool == "sum":
            return embeddings.sum(dim=1)
        if self.pool == "concat":
            return embeddings.reshape(embeddings.shape[0], -1)
        return embeddings[:, -1, :]

    def ranking_factors(self):
        """``(U, I, 1.0, None)`` for full-catalogue ranking (``recommend.recommend``): eval-mode propagation and the
        pooled tables (``[*, (L + 1) D]`` for concat), whose dot product is ``predict``."""
        users, items = self._stacks(False, False)
        return self.pooling(users).contiguous(), self.pooling(items).contiguous(), 1.0, None

    def predict(self, users, items):
        """mixgcf.py:135-157: propagation without dropout, pooled rows, plain dot product (no sigmoid, no draws)."""
        lib = self._require_hip()
        dev = self._flat.device
        users_t, items_t = index_tensor(users, dev), index_tensor(items, dev)
        if users_t.numel() != items_t.numel():
            raise ValueError("users and items differ in length")
        stats = self._device_stats()
        plan = self.plan()
        st = _lib.stream_ptr(dev)
        _lib.check(lib.hiprec_mixgcf_propagate(ctypes.byref(plan), 0, st))
        scores = torch.empty(users_t.numel(), dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_mixgcf_predict(ctypes.byref(plan), _lib.ptr(users_t), _lib.ptr(items_t),
                                             users_t.numel(), _lib.ptr(scores), _lib.ptr(stats), st))
        self._check_status()
        return scores


class LightGCNEngine(FlatModelEngine):
    """mixgcf.py:160-286, with the backward pass and the optimizer step the reference leaves out."""

    def __init__(self, config):
        self.config = config
        m = config["model"]
        self.norm_adj = m["norm_adj"]
        self.decay = float(m["l2"])
        self.pool = m["pool"]
        self.n_negs, self.ns, self.K = int(m["n_negs"]), m["ns"], int(m["K"])
        if self.ns not in ("rns", "mixgcf"):
            raise ValueError(f"ns {self.ns!r}: 'mixgcf' or 'rns'")
        if self.K < 1:
            raise ValueError(f"K = {self.K}: at least one negative per sample")
        if self.ns != "rns" and self.n_negs < 1:
            raise ValueError(f"n_negs = {self.n_negs}: at least one candidate per negative")
        self.model = LightGCN(m, self.norm_adj)
        if self.K * (self.model.context_hops + 1) > 64:
            raise ValueError(f"K * (context_hops + 1) = {self.K * (self.model.context_hops + 1)} > 64 is not supported")
        super(LightGCNEngine, self).__init__(config)
        self.model.to(self.device)
        self._choice = None
        self._seeds = None
        self._given_seeds = None
        self._gen = None

    def give_draws(self, seeds=None, edge_keep=None, mess_keep=None):
        """Use these numbers instead of drawing for the NEXT training step only: ``seeds [B, K, L + 1]``, and -- with the
        model in training mode -- per hop the edge keep mask ``[L, nnz]`` in the order of ``norm_adj._indices()`` and
        the message keep mask ``[L, N, D]`` (None: that dropout is off for the step).  No generator is touched."""
        self._given_seeds = seeds
        self.model._given = (edge_keep, mess_keep)

    def _batch(self, batch_data):
        if len(batch_data) != 3:
            raise ValueError("MixGCF batches are (users, pos_items, neg_items[B, n])")
        dev = self.model.flat.device
        users, pos = index_tensor(batch_data[0], dev), index_tensor(batch_data[1], dev)
        neg = batch_data[2] if torch.is_tensor(batch_data[2]) else torch.as_tensor(batch_data[2])
        B = users.numel()
        if B == 0:
            raise ValueError("empty batch")
        if pos.numel() != B:
            raise ValueError("users and pos_items differ in length")
        need = self.K if self.ns == "rns" else self.K * self.n_negs
        if neg.dim() != 2 or neg.shape[0] != B or neg.shape[1] < need:
            raise ValueError(f"neg_items must be [batch, n] with n >= {need} "
                             f"({'K' if self.ns == 'rns' else 'K * n_negs'})")
        return users, pos, neg.to(dev, torch.int64).contiguous(), B

    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        users, pos, neg, B = self._batch(batch_data)
        H = m.context_hops + 1
        masks = m.draw_masks() if m.training else None
        seeds = None
        given, self._given_seeds = self._given_seeds, None
        if self.ns != "rns":
            if given is not None:
                seeds = torch.as_tensor(given, dtype=torch.float32).reshape(B, self.K, H).to(dev)
            elif m.seed_rng == "torch_cpu":        # mixgcf.py:235, one draw per k
                seeds = torch.stack([torch.rand(B, 1, H, 1).view(B, H) for _ in range(self.K)], dim=1).to(dev)
            else:
                if self._gen is None or self._gen.device != dev:   # seeded once: the stream continues from step to step
                    self._gen = torch.Generator(device=dev)
                    self._gen.manual_seed(m.dropout_seed)
                seeds = torch.rand(B, self.K, H, device=dev, generator=self._gen)
            seeds = seeds.contiguous()
        self._seeds = seeds
        self._choice = torch.zeros(B, self.K, H, dtype=torch.int32, device=dev)
        plan = m.plan(self._g_flat, self.decay, self.n_negs, self.K, self.ns == "rns", masks)
        _lib.check(lib.hiprec_mixgcf_grad(
            ctypes.byref(plan), _lib.ptr(users), _lib.ptr(pos), _lib.ptr(neg), neg.shape[1], B, _lib.ptr(seeds),
            _lib.ptr(self._choice), self._batch_share() / B, _lib.ptr(self._stats), _lib.ptr(self._scratch),
            self._scratch.numel(), _lib.stream_ptr(dev)))

    def last_choice(self):
        """``int32 [B, K, L + 1]``: per row, negative and hop the index (inside its ``n_negs`` candidates) of the
        candidate the last step's sampler chose; all zeros for ``ns == "rns"``."""
        return self._choice

    def last_seeds(self):
        """``float32 [B, K, L + 1]`` mixing seeds of the last step (None for ``ns == "rns"``)."""
        return self._seeds

    def train_single_batch(self, batch_data):
        """mixgcf.py:176-203 plus ``backward()`` and ``optimizer.step()``: one step, returns the loss as a float."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_step(batch_data)
        return self._sync_stats().loss

    def train_an_epoch(self, train_loader, epoch_id):
        """mixgcf.py:205-220: prints the last batch's loss, logs the epoch sum."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        st = self._run_epoch(train_loader)
        print("[Training Epoch {}], Loss {}".format(epoch_id, st.loss))
        self.writer.add_scalar("model/loss", st.loss_sum, epoch_id)


MixGCF, MixGCFEngine = LightGCN, LightGCNEngine
