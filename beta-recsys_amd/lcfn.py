"""Drop-in ``LCFN`` / ``LCFNEngine`` for beta_rec/models/lcfn.py on libhiprec.so.

Interface parity (file:line = beta_rec/models/lcfn.py): ``LCFN(config, graph_embeddings)`` :8-99 (``user_embeddings`` /
``item_embeddings``, attributes ``P Q frequence_user frequence_item layer lamda``, the plain-tensor lists
``user_filters`` / ``item_filters`` / ``transformers``, ``predict``), ``LCFNEngine(config)`` :102-205
(``train_single_batch(batch) -> float``, ``train_an_epoch``; ``config["model"]["graph_embeddings"]`` = ``[P, Q]``).  Same
config keys (``n_users n_items emb_dim layer lamda optimizer lr device_str``), the same two ``state_dict`` keys, and the
reference's order of RNG draws (:24-48: ``nn.Embedding`` users, items; ``normal_(0.01, 0.02)`` users, items; ``layer``
torch draws for the user filters, then for the item filters; per layer two numpy draws for the transformer), so the same
torch and numpy seeds give the same tables, filters and transformers.

The step (``csrc/lcfn.hip``): per layer and side ``T = P^T X`` (row tiles reduced on the fp32 MFMA into per-block slots),
``M = (f (.) T) W`` (slots summed in a fixed order), ``X' = sigmoid(P M)`` into the ``[n, (L + 1) D]`` all-embeddings
table; BPR mean over the gathered all-rows + ``lamda`` x unsquared norms; the backward by hand.  ``diag(f)``,
``P diag(f)`` and anything ``[n, n]`` are never formed.  There is no CPU path.

Not kept:
* ``layer >= 2`` works, each layer feeding on the previous one's output; the reference raises ``AttributeError`` there
  (lcfn.py:68 and :81 read ``.weight`` of what has become a tensor);
* ``predict`` propagates from the CURRENT weights (cached until they change); the reference reads the tables its last
  training forward left behind -- the weights from before that step -- and fails before any step (lcfn.py:89-99);
* a gathered batch matrix whose norm is exactly 0 contributes gradient 0; the reference's ``x / 0`` writes NaN into the
  tables.

Extension: ``train_filters`` (default ``False``: the reference's behaviour, where filters and transformers never move
because they are neither parameters nor in the optimizer, lcfn.py:28-48).  When true the tail joins the optimizer sweep
with ``df``, ``dW`` and the gradients of its three norm terms; ``filter_state()`` / ``load_filter_state()`` hand it in
and out.  ``last_losses()`` returns ``(bpr, reg)``.  Data-parallel replicas are not offered: the regulariser is a norm
of the whole batch, not a sum over samples.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor

MAX_LAYERS = _lib.LCFN_MAX_LAYERS
MAX_DIM = _lib.LCFN_MAX_DIM
MAX_FREQ = _lib.LCFN_MAX_FREQ
MAX_WIDTH = _lib.LCFN_MAX_WIDTH
TAIL = ("user_filters", "item_filters", "transformers")


class LCFN(_FlatModel):
    """lcfn.py:8-99."""

    def __init__(self, config, graph_embeddings):
        super().__init__()
        self.config = config
        self.n_users, self.n_items = int(config["n_users"]), int(config["n_items"])
        self.emb_dim = int(config["emb_dim"])
        self.layer = int(config["layer"])
        self.lamda = float(config["lamda"])
        self.train_filters = bool(config["train_filters"]) if "train_filters" in config else False
        self.n_slots = int(config["project_slots"]) if "project_slots" in config else 0   # 0: the library's default
        P, Q = graph_embeddings
        self.P = torch.as_tensor(np.asarray(P), dtype=torch.float32).contiguous()
        self.Q = torch.as_tensor(np.asarray(Q), dtype=torch.float32).contiguous()
        if self.P.dim() != 2 or self.Q.dim() != 2 or self.P.shape[0] != self.n_users or self.Q.shape[0] != self.n_items:
            raise ValueError(f"graph_embeddings are {tuple(self.P.shape)} and {tuple(self.Q.shape)}, expected "
                             f"[{self.n_users}, F_u] and [{self.n_items}, F_i]")
        self.frequence_user, self.frequence_item = int(self.P.shape[1]), int(self.Q.shape[1])
        if not 1 <= self.emb_dim <= MAX_DIM:
            raise ValueError(f"emb_dim {self.emb_dim}: 1 .. {MAX_DIM} are supported")
        for name, f in (("frequence_user", self.frequence_user), ("frequence_item", self.frequence_item)):
            if not 1 <= f <= MAX_FREQ:
                raise ValueError(f"{name} {f}: 1 .. {MAX_FREQ} are supported")
        if not 1 <= self.layer <= MAX_LAYERS:
            raise ValueError(f"layer {self.layer}: 1 .. {MAX_LAYERS} are supported")
        if (self.layer + 1) * self.emb_dim > MAX_WIDTH:
            raise ValueError(f"(layer + 1) * emb_dim = {(self.layer + 1) * self.emb_dim}: at most {MAX_WIDTH} (the top-K "
                             "path's widest row)")
        if self.n_slots < 0:
            raise ValueError(f"project_slots {self.n_slots}: must not be negative")
        D, L = self.emb_dim, self.layer
        shapes = {"user_filters": (self.frequence_user,), "item_filters": (self.frequence_item,), "transformers": (D, D)}
        v = self._build([("user_embeddings.weight", (self.n_users, D)), ("item_embeddings.weight", (self.n_items, D))]
                        + [(f"{name}.{k}", shapes[name]) for name in TAIL for k in range(L)])
        # RNG order of lcfn.py:24-48
        for n in (self.n_users, self.n_items):
            nn.Embedding(n, D)                                   # the constructor's own N(0, 1) draw, overwritten below
        nn.init.normal_(v["user_embeddings.weight"], mean=0.01, std=0.02)
        nn.init.normal_(v["item_embeddings.weight"], mean=0.01, std=0.02)
        for k in range(L):
            v[f"user_filters.{k}"].copy_(torch.normal(mean=1, std=0.001, size=(1, self.frequence_user))[0])
        for k in range(L):
            v[f"item_filters.{k}"].copy_(torch.normal(size=(1, self.frequence_item), mean=1, std=0.001)[0])
        for k in range(L):
            v[f"transformers.{k}"].copy_(torch.tensor(
                (np.random.normal(0, 0.001, (D, D)) + np.diag(np.random.normal(1, 0.001, D))).astype(np.float32)))
        self.user_embeddings = _ParamView(v["user_embeddings.weight"])
        self.item_embeddings = _ParamView(v["item_embeddings.weight"])
        self._bind_tail(v)
        self._ws = None
        self._weights_clock = 0      # bumped by the engine with every optimizer step
        self._pool_key = None

    @property
    def table_floats(self):
        """The leading floats of the flat buffer the two tables take; the tail follows."""
        return (self.n_users + self.n_items) * self.emb_dim

    def _bind_tail(self, views):
        """The tail as plain tensors in Python lists (views of the flat buffer): no parameters, no buffers -- the
        ``state_dict`` keys stay the reference's two."""
        for name in TAIL:
            object.__setattr__(self, name, [views[f"{name}.{k}"] for k in range(self.layer)])

    def _rebind(self, flat):
        self._flat = flat
        views = self.views(flat)
        self.user_embeddings.weight.data = views["user_embeddings.weight"]
        self.item_embeddings.weight.data = views["item_embeddings.weight"]
        self._bind_tail(views)
        self.P, self.Q = self.P.to(flat.device), self.Q.to(flat.device)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self._weights_clock += 1         # predict's cached propagation is stale
        return out

    def filter_state(self):
        """The tail as a dict of CPU copies: ``user_filters.k`` / ``item_filters.k`` / ``transformers.k``."""
        return {f"{name}.{k}": t.detach().cpu().clone() for name in TAIL for k, t in enumerate(getattr(self, name))}

    def load_filter_state(self, state):
        for name in TAIL:
            for k, t in enumerate(getattr(self, name)):
                t.copy_(torch.as_tensor(np.asarray(state[f"{name}.{k}"]), dtype=torch.float32).reshape(t.shape))
        self._weights_clock += 1

    # ---- workspace + plan -------------------------------------------------------------------------
    def workspace(self, batch=0):
        dev = self._flat.device
        lib = _lib.load()
        if self._ws is None or self._ws["dev"] != dev:
            n = int(lib.hiprec_lcfn_ws_floats(self.n_users, self.n_items, self.frequence_user, self.frequence_item,
                                              self.emb_dim, self.layer, self.n_slots))
            self._ws = {"dev": dev, "batch_ws": None, "ws": torch.zeros(n, dtype=torch.float32, device=dev)}
            self._pool_key = None
        if batch:
            self._ws["batch_ws"] = _lib.grow(self._ws["batch_ws"], int(lib.hiprec_lcfn_batch_ws_floats(batch)),
                                             torch.float32, dev)
        return self._ws

    def plan(self, g_flat=None, batch=0):
        ws = self.workspace(batch)
        if self.P.device != self._flat.device:
            self.P, self.Q = self.P.to(self._flat.device), self.Q.to(self._flat.device)
        p = _lib.LcfnPlan()
        p.P, p.Q = self.P.data_ptr(), self.Q.data_ptr()
        p.n_users, p.n_items = self.n_users, self.n_items
        p.f_user, p.f_item, p.dim, p.layer = self.frequence_user, self.frequence_item, self.emb_dim, self.layer
        p.train_filters, p.n_slots, p.lamda = int(self.train_filters), self.n_slots, self.lamda
        p.w = self._flat.data_ptr()
        p.g = None if g_flat is None else g_flat.data_ptr()
        p.ws, p.ws_floats = ws["ws"].data_ptr(), ws["ws"].numel()
        if batch:
            p.batch_ws, p.batch_ws_floats = ws["batch_ws"].data_ptr(), ws["batch_ws"].numel()
        return p

    # ---- reference API ----------------------------------------------------------------------------
    def _all_embeddings(self):
        """``(U_all [n_users, (L + 1) D], I_all)`` from the current weights (cached until they change): views of the
        workspace (lcfn.py:74, :87)."""
        lib = self._require_hip()
        key = (self._flat.data_ptr(), self._flat._version, self._weights_clock)
        if self._ws is None or self._ws["dev"] != self._flat.device or key != self._pool_key:
            plan = self.plan()
            _lib.check(lib.hiprec_lcfn_propagate(ctypes.byref(plan), _lib.stream_ptr(self._flat.device)))
            self._pool_key = key
        W = (self.layer + 1) * self.emb_dim
        ws = self._ws["ws"]
        return ws[: self.n_users * W].view(self.n_users, W), ws[self.n_users * W: (self.n_users + self.n_items) * W].view(
            self.n_items, W)

    def forward(self):
        """lcfn.py:55-87: leaves ``user_all_embeddings`` / ``item_all_embeddings`` behind."""
        self.user_all_embeddings, self.item_all_embeddings = self._all_embeddings()

    def ranking_factors(self):
        """``(U_all, I_all, 1.0, None)`` for full-catalogue ranking: the score is the plain dot product of all-rows."""
        ua, ia = self._all_embeddings()
        return ua, ia, 1.0, None

    def predict(self, users, items):
        """lcfn.py:89-99 on the CURRENT weights: dot product of the all-rows."""
        lib = self._require_hip()
        dev = self._flat.device
        users_t, items_t = index_tensor(users, dev), index_tensor(items, dev)
        if users_t.numel() != items_t.numel():
            raise ValueError("users and items differ in length")
        self._all_embeddings()
        stats = self._device_stats()
        plan = self.plan()
        scores = torch.empty(users_t.numel(), dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_lcfn_predict(ctypes.byref(plan), _lib.ptr(users_t), _lib.ptr(items_t), users_t.numel(),
                                           _lib.ptr(scores), _lib.ptr(stats), _lib.stream_ptr(dev)))
        self._check_status()
        return scores


class LCFNEngine(FlatModelEngine):
    """lcfn.py:102-205."""

    def __init__(self, config):
        self.config = config
        self.graph_embeddings = config["model"]["graph_embeddings"]
        self.model = LCFN(config["model"], self.graph_embeddings)
        super(LCFNEngine, self).__init__(config)
        self.model.to(self.device)

    def _alloc_extra(self, lib, device):
        self._parts = torch.zeros(4, dtype=torch.float32, device=device)

    def _sweep_floats(self):
        """The two tables; the tail only when the filters are trained."""
        return self.model.flat.numel() if self.model.train_filters else self.model.table_floats

    def _enqueue_grad(self, batch_data):
        if self._dp_world != 1:
            raise NotImplementedError("LCFN has no data-parallel form: its regulariser is a norm of the whole batch")
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 3:
            raise ValueError("LCFN batches are (users, pos_items, neg_items)")
        users, pos, neg = (index_tensor(x, dev) for x in batch_data)
        B = users.numel()
        if not (pos.numel() == B and neg.numel() == B):
            raise ValueError("batch tensors differ in length")
        if B == 0:
            raise ValueError("empty batch")
        plan = m.plan(self._g_flat, B)
        m._pool_key = None                   # the training forward overwrites the all-embeddings tables
        _lib.check(lib.hiprec_lcfn_grad(ctypes.byref(plan), _lib.ptr(users), _lib.ptr(pos), _lib.ptr(neg), B,
                                        _lib.ptr(self._parts), _lib.ptr(self._stats), _lib.ptr(self._scratch),
                                        self._scratch.numel(), _lib.stream_ptr(dev)))

    def _enqueue_opt(self, *a, **k):
        super()._enqueue_opt(*a, **k)
        self.model._weights_clock += 1

    def load_optimizer_state(self, step, exp_avg=None, exp_avg_sq=None):
        """As the base's, with the tail's moments zero where the dicts hold only the reference's two keys."""
        m = self.model

        def full(src):
            if src is None:
                return None
            return {name: (src[name] if name in src else np.zeros(shape, dtype=np.float32)) for name, shape in m._spec}

        super().load_optimizer_state(step, full(exp_avg), full(exp_avg_sq))

    def last_losses(self):
        """``(bpr, reg)`` of the last step (one host sync)."""
        p = self._parts.cpu().numpy()
        return float(p[0]), float(p[1])

    def train_single_batch(self, batch_data):
        """lcfn.py:115-152: one step, returns ``bpr_loss + regularizer`` as a float."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._setup()
        self._enqueue_step(batch_data)
        return self._sync_stats().loss

    def train_an_epoch(self, train_loader, epoch_id):
        """lcfn.py:154-169: every batch; prints the last batch's loss, logs the epoch sum."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        st = self._run_epoch(train_loader)
        print("[Training Epoch {}], Loss {}".format(epoch_id, st.loss))
        self.writer.add_scalar("model/loss", st.loss_sum, epoch_id)
