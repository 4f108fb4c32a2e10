"""Drop-in ``BUIR_NB`` / ``BUIREngine`` for beta_rec/models/buir.py on libhiprec.so.

Interface parity (file:line = beta_rec/models/buir.py): ``BUIR_NB(config)`` :9-100 (two ``LGCN_Encoder`` with
``embedding_dict.user_emb`` / ``item_emb``, xavier-uniform, the target's own draws consumed and then overwritten by the
online tables, ``predictor = nn.Linear(D, D)`` built after both), ``BUIREngine(config)`` :202-250
(``train_single_batch(batch_data) -> float``, ``train_an_epoch(train_loader, epoch_id)``).  Same config keys (``n_users
n_items emb_dim momentum norm_adj optimizer lr batch_size device_str``), same ``state_dict`` keys in the same order, same
initial weights for the same torch seed.

The step (``csrc/buir.hip``): ``P = mean(E_0, A E_0, .., A^L E_0)`` of the online tables (hop 0 is in the mean), one fused
kernel per batch tile -- gather, ``y = x W^T + b`` for the stacked user and item rows on the exact-fp32 MFMA, ``loss =
mean[(2 - 2 n(y_u).n(t_i)) + (2 - 2 n(y_i).n(t_u))]``, its backward --, and the backward chain over ``A^T``.  The reference
never calls ``_update_target``, so its target encoder is the frozen initial online encoder: the pooled target table is a
constant of the workspace and a step runs L SpMMs forward and L backward where the reference runs 3 L.  The negatives of a
batch are accepted and ignored, as buir.py:226-228 does.  There is no CPU path.

The target tables are checkpointed, so they live in the flat buffer -- behind the trained parameters, outside the range
the dense optimizer sweeps (``BUIREngine._sweep_floats``): the sweep never reads or writes them.

Not kept:
* ``emb_dim`` is limited to 1 .. 256;
* ``n_layers`` is an optional config key (default 3, the reference's hard-coded value; 1 .. 4): the reference ignores it;
* a one-element ``predict`` returns one score (the reference's ``.squeeze()`` makes that call raise);
* ``norm_adj`` is used on the parameters' device (the reference leaves it on the host, and fails there on a GPU);
* ``layer_size``, ``keep_pro``, ``drop_flag`` and ``sparse_dropout`` are dead in the reference and have no mirror.

Extension, the moving target: ``update_target`` (config key, default ``False`` = the reference).  When set, every optimizer
step is followed by what ``_update_target`` (buir.py:48-54) would do, ``T <- m T + (1 - m) O``, on the raw tables at once
(``state_dict`` never needs a flush) and -- the pool being linear -- on the pooled target at the NEXT step's forward, ``P_tg
<- m P_tg + (1 - m) P_on``, in the pass that writes the pooled online rows; the target is never propagated.  The workspace's
``pending`` flag marks a step whose pooled update is still due.  ``load_state_dict`` / ``resume_checkpoint``,
``.to(device)`` and ``invalidate_target()`` have the pooled target rebuilt from the raw tables; ``pooled_target()`` returns it.
"""
import ctypes

import torch
import torch.nn as nn
from torch.nn import Parameter

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor
from .lightgcn import _csr_from_coo, _slice_rows
from .mixgcf import coo_to_csr_maps
from .sgl import _coo_of

MAX_LAYERS = _lib.BUIR_MAX_LAYERS
MAX_DIM = _lib.BUIR_MAX_DIM
TILE_B = _lib.BUIR_TILE_B
ONLINE = ("online_encoder.embedding_dict.user_emb", "online_encoder.embedding_dict.item_emb")
TARGET = ("target_encoder.embedding_dict.user_emb", "target_encoder.embedding_dict.item_emb")
PREDICTOR = ("predictor.weight", "predictor.bias")
TRAINABLE = ONLINE + PREDICTOR


class _Encoder(nn.Module):
    """buir.py:103-134: the parameter holder of one ``LGCN_Encoder`` (the propagation is the model's)."""

    def __init__(self, user_emb, item_emb):
        super().__init__()
        self.embedding_dict = nn.ParameterDict({"user_emb": Parameter(user_emb, requires_grad=False),
                                                "item_emb": Parameter(item_emb, requires_grad=False)})


class BUIR_NB(_FlatModel):
    """buir.py:9-100."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.user_count = self.n_users = int(config["n_users"])
        self.item_count = self.n_items = int(config["n_items"])
        self.latent_size = self.emb_dim = int(config["emb_dim"])
        self.momentum = float(config["momentum"])
        self.norm_adj = config["norm_adj"]
        self.n_layers = int(config["n_layers"]) if "n_layers" in config else 3
        self.update_target = bool(config["update_target"]) if "update_target" in config else False
        if not 1 <= self.emb_dim <= MAX_DIM:
            raise ValueError(f"emb_dim {self.emb_dim}: 1 .. {MAX_DIM} are supported")
        if not 1 <= self.n_layers <= MAX_LAYERS:
            raise ValueError(f"n_layers {self.n_layers}: 1 .. {MAX_LAYERS} are supported")
        U, I, D = self.n_users, self.n_items, self.emb_dim
        # flat order: what trains first, the checkpointed-only target tables behind it
        v = self._build([(ONLINE[0], (U, D)), (ONLINE[1], (I, D)), (PREDICTOR[0], (D, D)), (PREDICTOR[1], (D,)),
                         (TARGET[0], (U, D)), (TARGET[1], (I, D))])
        self.n_trainable = self.offset_of(TARGET[0])
        # RNG order of buir.py:20-39: online user, online item, the target's own two draws (discarded by _init_target),
        # then nn.Linear's own init
        nn.init.xavier_uniform_(v[ONLINE[0]])
        nn.init.xavier_uniform_(v[ONLINE[1]])
        nn.init.xavier_uniform_(v[TARGET[0]])
        nn.init.xavier_uniform_(v[TARGET[1]])
        lin = nn.Linear(D, D)
        v[PREDICTOR[0]].copy_(lin.weight.data)
        v[PREDICTOR[1]].copy_(lin.bias.data)
        v[TARGET[0]].copy_(v[ONLINE[0]])
        v[TARGET[1]].copy_(v[ONLINE[1]])
        # module order = the reference's state_dict order
        self.online_encoder = _Encoder(v[ONLINE[0]], v[ONLINE[1]])
        self.target_encoder = _Encoder(v[TARGET[0]], v[TARGET[1]])
        self.predictor = _ParamView(v[PREDICTOR[0]], v[PREDICTOR[1]])
        self._graph = None
        self._ws = None

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
        """The five ``[n, D]`` tables of a step (pooled online, pooled target, gradient table, two hop buffers), the
        ``stale`` / ``pending`` flags of the pooled target, and the batch-sized partial sums."""
        dev = self._flat.device
        lib = _lib.load()
        N = self.n_users + self.n_items
        if self._ws is None or self._ws["dev"] != dev:
            self._ws = {"dev": dev, "batch_ws": None, "stale": True, "pending": False,
                        "ws": torch.zeros(int(lib.hiprec_buir_ws_floats(N, self.emb_dim)), dtype=torch.float32, device=dev)}
        if batch:
            self._ws["batch_ws"] = _lib.grow(self._ws["batch_ws"], int(lib.hiprec_buir_batch_ws_floats(batch, self.emb_dim)),
                                             torch.float32, dev)
        return self._ws

    def plan(self, g_flat=None, batch=0, graph=True):
        p = _lib.BuirPlan()
        N = self.n_users + self.n_items
        p.n_users, p.n_items, p.dim, p.n_layers = self.n_users, self.n_items, self.emb_dim, self.n_layers
        p.momentum, p.one_minus_momentum = self.momentum, 1.0 - self.momentum
        base, fs = self._flat.data_ptr(), 4
        p.online = base + fs * self.offset_of(ONLINE[0])
        p.target = base + fs * self.offset_of(TARGET[0])
        p.w = base + fs * self.offset_of(PREDICTOR[0])
        p.b = base + fs * self.offset_of(PREDICTOR[1])
        if not graph:
            return p
        gr, ws = self.graph(), self.workspace(batch)
        p.a = _lib.Csr(gr["rowptr"].data_ptr(), gr["col"].data_ptr(), gr["val"].data_ptr(), None, N, gr["nnz"],
                       _lib.ptr(gr.get("slice_row")))
        p.at = _lib.Csr(gr["rowptr_t"].data_ptr(), gr["col_t"].data_ptr(), gr["val_t"].data_ptr(), None, N, gr["nnz"],
                        _lib.ptr(gr.get("slice_row_t")))
        if g_flat is not None:
            g = g_flat.data_ptr()
            p.g_online = g + fs * self.offset_of(ONLINE[0])
            p.g_w = g + fs * self.offset_of(PREDICTOR[0])
            p.g_b = g + fs * self.offset_of(PREDICTOR[1])
        p.ws, p.ws_floats = ws["ws"].data_ptr(), ws["ws"].numel()
        if batch:
            p.batch_ws, p.batch_ws_floats = ws["batch_ws"].data_ptr(), ws["batch_ws"].numel()
        return p

    # ---- the pooled target --------------------------------------------------------------------------
    def invalidate_target(self):
        """The raw target tables were written from outside a step: the pooled target is rebuilt from them at its next
        use, and a pooled update that was still due is dropped with it (the raw tables already carry it)."""
        if getattr(self, "_ws", None) is not None:
            self._ws["stale"], self._ws["pending"] = True, False

    def _pooled_target_view(self):
        N, D = self.n_users + self.n_items, self.emb_dim
        return self.workspace()["ws"][N * D:2 * N * D].view(N, D)

    def _ensure_target(self):
        lib = self._require_hip()
        ws = self.workspace()
        if ws["stale"]:
            plan = self.plan()
            _lib.check(lib.hiprec_buir_pool(ctypes.byref(plan), plan.target, _lib.ptr(self._pooled_target_view()), None,
                                            _lib.stream_ptr(self._flat.device)))
            ws["stale"], ws["pending"] = False, False

    def pooled_target(self):
        """``[n, D]``: the pooled target table the next step's loss reads (a pending moving-average update applied)."""
        self._ensure_target()
        out = self._pooled_target_view().clone()
        if self._ws["pending"]:
            out.mul_(self.momentum).add_(self._pooled(self.views()[ONLINE[0]].data_ptr())[0], alpha=1.0 - self.momentum)
        return out

    def _pooled(self, table_ptr, project=False):
        lib = self._require_hip()
        dev = self._flat.device
        N, D = self.n_users + self.n_items, self.emb_dim
        plan = self.plan()
        P = torch.empty(N, D, dtype=torch.float32, device=dev)
        PW = torch.empty(N, D, dtype=torch.float32, device=dev) if project else None
        _lib.check(lib.hiprec_buir_pool(ctypes.byref(plan), table_ptr, _lib.ptr(P), _lib.ptr(PW), _lib.stream_ptr(dev)))
        return P, PW

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_target()
        return out

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self.invalidate_target()
        return self

    # ---- reference API ----------------------------------------------------------------------------
    def ranking_factors(self):
        """``(cat[p(P_u), P_u], cat[P_i, p(P_i)], 1.0, None)`` for full-catalogue ranking: width 2 D, whose dot product
        is ``predict``.  P is the ONLINE pool (buir.py:61-64)."""
        P, PW = self._pooled(self.views()[ONLINE[0]].data_ptr(), project=True)
        U = self.n_users
        return torch.cat([PW[:U], P[:U]], dim=1), torch.cat([P[U:], PW[U:]], dim=1), 1.0, None

    def predict(self, users, items):
        """buir.py:79-100: ``p(P[u]).P[U + i] + P[u].p(P[U + i])`` on the online pool."""
        lib = self._require_hip()
        dev = self._flat.device
        users_t, items_t = index_tensor(users, dev), index_tensor(items, dev)
        if users_t.numel() != items_t.numel():
            raise ValueError("users and items differ in length")
        stats = self._device_stats()
        plan = self.plan()
        scores = torch.empty(users_t.numel(), dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_buir_predict(ctypes.byref(plan), _lib.ptr(users_t), _lib.ptr(items_t), users_t.numel(),
                                           _lib.ptr(scores), _lib.ptr(stats), _lib.stream_ptr(dev)))
        self._check_status()
        return scores


class BUIREngine(FlatModelEngine):
    """buir.py:202-250."""

    def __init__(self, config):
        self.config = config
        self.norm_adj = config["model"]["norm_adj"]
        self.model = BUIR_NB(config["model"])
        super(BUIREngine, self).__init__(config)
        self.model.to(self.device)

    def _sweep_floats(self):
        """The trained parameters only: the target tables sit behind them in the flat buffer and are never swept."""
        return self.model.n_trainable

    def invalidate_target(self):
        self.model.invalidate_target()

    def pooled_target(self):
        return self.model.pooled_target()

    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if self._dp_world != 1:
            raise NotImplementedError("BUIR's data-parallel form is not built")
        if len(batch_data) != 3:
            raise ValueError("BUIR batches are (users, pos_items, neg_items)")
        users, pos, neg = (index_tensor(x, dev) for x in batch_data)
        B = users.numel()
        if not (pos.numel() == B and neg.numel() == B):
            raise ValueError("batch tensors differ in length")
        if B == 0:
            raise ValueError("empty batch")
        m._ensure_target()
        plan = m.plan(self._g_flat, B)
        plan.apply_pending = 1 if m._ws["pending"] else 0
        _lib.check(lib.hiprec_buir_grad(ctypes.byref(plan), _lib.ptr(users), _lib.ptr(pos), _lib.ptr(neg), B,
                                        _lib.ptr(self._stats), _lib.ptr(self._scratch), self._scratch.numel(),
                                        _lib.stream_ptr(dev)))
        m._ws["pending"] = False             # the forward's finishing pass applied it

    def _enqueue_step(self, batch_data):
        self._enqueue_grad(batch_data)
        self._enqueue_opt()
        m = self.model
        if m.update_target:                  # buir.py:48-54, which the reference defines and never calls
            plan = m.plan(graph=False)
            _lib.check(_lib.load().hiprec_buir_ema(ctypes.byref(plan), _lib.stream_ptr(m.flat.device)))
            m._ws["pending"] = True

    def backward_only(self, batch_data):
        """zero_grad + forward + loss + backward without the optimizer step: ``(loss, grads)`` of the four trained
        tensors (nothing reaches the target)."""
        loss, grads = super().backward_only(batch_data)
        return loss, {k: grads[k] for k in TRAINABLE}

    def load_optimizer_state(self, step, exp_avg=None, exp_avg_sq=None):
        """As the base's; the target tables have no moments in the reference's optimizer state and keep zeros."""
        def padded(src):
            if src is None:
                return None
            src = dict(src)
            for name, shape in self.model._spec:
                if name in TARGET:
                    src.setdefault(name, torch.zeros(shape))
            return src

        super().load_optimizer_state(step, padded(exp_avg), padded(exp_avg_sq))

    def train_single_batch(self, batch_data):
        """buir.py:215-233: one step, returns the batch loss as a float."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._setup()
        self._enqueue_step(batch_data)
        return self._sync_stats().loss

    def train_an_epoch(self, train_loader, epoch_id):
        """buir.py:235-250: every batch; prints the last batch's loss, logs the epoch sum."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        st = self._run_epoch(train_loader)
        print("[Training Epoch {}], Loss {}".format(epoch_id, st.loss))
        self.writer.add_scalar("model/loss", st.loss_sum, epoch_id)
