"""Drop-in ``SimGCL`` / ``SimGCLEngine`` for beta_rec/models/simgcl.py on libhiprec.so.

Interface parity (file:line = beta_rec/models/simgcl.py): ``SimGCL(config, norm_adj)`` :9-82 (``nn.Embedding`` tables
``user_embedding`` / ``item_embedding``, N(0, 1), in that order; ``predict`` on the RAW tables), ``SimGCLEngine(config)``
:85-163 (``train_single_batch(batch_data) -> float``, ``train_an_epoch(train_loader, epoch_id)``).  Same config keys
(``n_users n_items emb_dim n_layer eps reg lambda batch_size norm_adj optimizer lr device_str``), same ``state_dict`` keys,
same initial weights for the same torch seed.

The step (``csrc/simgcl.hip``): three propagations over ``norm_adj`` -- a clean one and two whose every hop is perturbed,
``X_k = Y_k + sign(Y_k) * normalize(u) * eps`` --, each mean-pooled over hops 1 .. L; loss = BPR **sum** of
``-log(1e-7 + sigmoid(pos - neg))`` on the clean pool + ``reg`` x the unsquared Frobenius norms of the three batch matrices
+ ``lambda`` x InfoNCE among the batch's **unique** users and unique positive items at temperature 0.2.  ``sign`` has no
derivative, so the three views share one backward chain; the noise is drawn in registers and never stored; the unique ids
never visit the host.  There is no CPU path.

Not kept:
* the uniforms come from a counter-based device draw keyed by (``noise_seed``, step, view, hop, row, column), not from
  torch's generator: the same distribution, other numbers;
* a batch matrix of Frobenius norm exactly 0 contributes gradient 0 (the reference writes NaN);
* ``n_layer < 1`` raises ``ValueError`` (the reference fails in ``torch.stack``); ``emb_dim`` is limited to 1 .. 256 and
  ``n_layer`` to 1 .. 4.

Extensions: ``noise=`` on ``backward_only`` / ``train_single_batch`` supplies the ``[2, L, n, D]`` uniforms explicitly;
``noise_seed`` (default: the torch seed) and ``draw_noise(step)`` give the uniforms the device draw uses at a step;
``last_losses()`` returns ``(bpr, reg, cl_user, cl_item)``; ``cl_temp`` (default 0.2); ``user_view = "reference"``
(default) contrasts the users' view 1 with itself as simgcl.py:65 does, ``"two_views"`` with view 2 as the paper does.
"""
import ctypes

import torch

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor
from .lightgcn import _csr_from_coo, _slice_rows
from .mixgcf import coo_to_csr_maps
from .sgl import _coo_of

MAX_LAYERS = _lib.SIMGCL_MAX_LAYERS
MAX_DIM = _lib.SIMGCL_MAX_DIM
USER_VIEWS = {"reference": 1, "two_views": 2}


class SimGCL(_FlatModel):
    """simgcl.py:9-82."""

    def __init__(self, config, norm_adj=None):
        super().__init__()
        self.config = config
        self.eps = float(config["eps"])
        self.n_layers = int(config["n_layer"])
        self.n_users, self.n_items = int(config["n_users"]), int(config["n_items"])
        self.emb_dim = int(config["emb_dim"])
        if not 1 <= self.emb_dim <= MAX_DIM:
            raise ValueError(f"emb_dim {self.emb_dim}: 1 .. {MAX_DIM} are supported")
        if not 1 <= self.n_layers <= MAX_LAYERS:
            raise ValueError(f"n_layer {self.n_layers}: 1 .. {MAX_LAYERS} are supported")
        self.reg = float(config["reg"]) if "reg" in config else 0.0
        self.cl_rate = float(config["lambda"]) if "lambda" in config else 0.0
        self.cl_temp = float(config["cl_temp"]) if "cl_temp" in config else 0.2
        if not self.cl_temp > 0:
            raise ValueError(f"cl_temp {self.cl_temp}: must be positive")
        self.user_view = config["user_view"] if "user_view" in config else "reference"
        if self.user_view not in USER_VIEWS:
            raise ValueError(f"unknown user_view {self.user_view!r}: 'reference' or 'two_views'")
        self.norm_adj = norm_adj if norm_adj is not None else config["norm_adj"]
        v = self._build([("user_embedding.weight", (self.n_users, self.emb_dim)),
                         ("item_embedding.weight", (self.n_items, self.emb_dim))])
        # RNG order of simgcl.py:21-23: two nn.Embedding, N(0, 1) each
        v["user_embedding.weight"].normal_(0, 1)
        v["item_embedding.weight"].normal_(0, 1)
        self.user_embedding = _ParamView(v["user_embedding.weight"])
        self.item_embedding = _ParamView(v["item_embedding.weight"])
        self.noise_seed = (int(config["noise_seed"]) if "noise_seed" in config else torch.initial_seed()) % (1 << 64)
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
        """The ``[n, D]`` tables of a step (one of them the gradient table; no noise), the stamp table with the step
        clock in front of it, and the batch-sized buffers."""
        dev = self._flat.device
        lib = _lib.load()
        N = self.n_users + self.n_items
        if self._ws is None or self._ws["dev"] != dev:
            self._ws = {"dev": dev, "batch_ws": None, "clock": 0,
                        "ws": torch.zeros(int(lib.hiprec_simgcl_ws_floats(N, self.emb_dim)), dtype=torch.float32, device=dev),
                        "stamps": torch.zeros(int(lib.hiprec_simgcl_stamp_ints(N)), dtype=torch.int32, device=dev)}
        if batch:
            self._ws["batch_ws"] = _lib.grow(self._ws["batch_ws"], int(lib.hiprec_simgcl_batch_ws_floats(batch, self.emb_dim)),
                                             torch.float32, dev)
        return self._ws

    @property
    def noise_step(self):
        """The step the next training call draws its noise at: the workspace's clock, mirrored on the host."""
        return self.workspace()["clock"]

    def plan(self, g_flat=None, batch=0, noise=None, graph=True):
        p = _lib.SimgclPlan()
        N = self.n_users + self.n_items
        p.n_users, p.n_items, p.dim, p.n_layers = self.n_users, self.n_items, self.emb_dim, self.n_layers
        p.user_view = USER_VIEWS[self.user_view]
        p.eps, p.reg, p.lambda_, p.cl_temp, p.noise_seed = self.eps, self.reg, self.cl_rate, self.cl_temp, self.noise_seed
        p.e0 = self._flat.data_ptr()
        if not graph:
            return p
        gr, ws = self.graph(), self.workspace(batch)
        p.a = _lib.Csr(gr["rowptr"].data_ptr(), gr["col"].data_ptr(), gr["val"].data_ptr(), None, N, gr["nnz"],
                       _lib.ptr(gr.get("slice_row")))
        p.at = _lib.Csr(gr["rowptr_t"].data_ptr(), gr["col_t"].data_ptr(), gr["val_t"].data_ptr(), None, N, gr["nnz"],
                        _lib.ptr(gr.get("slice_row_t")))
        p.g = None if g_flat is None else g_flat.data_ptr()
        p.ws, p.ws_floats, p.stamps = ws["ws"].data_ptr(), ws["ws"].numel(), ws["stamps"].data_ptr()
        p.noise = None if noise is None else noise.data_ptr()
        if batch:
            p.batch_ws, p.batch_ws_floats = ws["batch_ws"].data_ptr(), ws["batch_ws"].numel()
        return p

    def draw_noise(self, step):
        """The ``[2, L, n, D]`` uniforms (view, hop, row, column) the device draw of ``(noise_seed, step)`` uses."""
        lib = self._require_hip()
        dev = self._flat.device
        N = self.n_users + self.n_items
        out = torch.empty(2, self.n_layers, N, self.emb_dim, dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_simgcl_noise(self.noise_seed, int(step), self.n_layers, N, self.emb_dim, _lib.ptr(out),
                                           _lib.stream_ptr(dev)))
        return out

    # ---- reference API ----------------------------------------------------------------------------
    def ranking_factors(self):
        """``(U, I, 1.0, None)`` for full-catalogue ranking: the two raw tables, whose dot product is ``predict``."""
        self._require_hip()
        v = self.views()
        return v["user_embedding.weight"], v["item_embedding.weight"], 1.0, None

    def predict(self, users, items):
        """simgcl.py:72-82: dot product of the RAW table rows (no propagation)."""
        lib = self._require_hip()
        dev = self._flat.device
        users_t, items_t = index_tensor(users, dev), index_tensor(items, dev)
        if users_t.numel() != items_t.numel():
            raise ValueError("users and items differ in length")
        stats = self._device_stats()
        plan = self.plan(graph=False)
        scores = torch.empty(users_t.numel(), dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_simgcl_predict(ctypes.byref(plan), _lib.ptr(users_t), _lib.ptr(items_t), users_t.numel(),
                                             _lib.ptr(scores), _lib.ptr(stats), _lib.stream_ptr(dev)))
        self._check_status()
        return scores


class SimGCLEngine(FlatModelEngine):
    """simgcl.py:85-163."""

    def __init__(self, config):
        self.config = config
        m = config["model"]
        self.reg = float(m["reg"])
        self.batch_size = m["batch_size"] if "batch_size" in m else None
        self.cl_rate = float(m["lambda"])
        self.norm_adj = m["norm_adj"]
        self.model = SimGCL(m, self.norm_adj)
        super(SimGCLEngine, self).__init__(config)
        self.model.to(self.device)
        self._noise = None

    def _alloc_extra(self, lib, device):
        self._parts = torch.zeros(8, dtype=torch.float32, device=device)

    def draw_noise(self, step):
        return self.model.draw_noise(step)

    @property
    def noise_step(self):
        return self.model.noise_step

    def _checked_noise(self, noise):
        if noise is None:
            return None
        m = self.model
        shape = (2, m.n_layers, m.n_users + m.n_items, m.emb_dim)
        noise = torch.as_tensor(noise, dtype=torch.float32).to(m.flat.device).contiguous()
        if tuple(noise.shape) != shape:
            raise ValueError(f"noise is {tuple(noise.shape)}, expected {shape}: [view, hop, row, column]")
        return noise

    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if self._dp_world != 1:
            raise NotImplementedError("SimGCL's loss is no sum over samples (norms of the whole batch, InfoNCE among its "
                                      "unique ids): there is no data-parallel form")
        if len(batch_data) != 3:
            raise ValueError("SimGCL batches are (users, pos_items, neg_items)")
        users, pos, neg = (index_tensor(x, dev) for x in batch_data)
        B = users.numel()
        if not (pos.numel() == B and neg.numel() == B):
            raise ValueError("batch tensors differ in length")
        if B == 0:
            raise ValueError("empty batch")
        plan = m.plan(self._g_flat, B, self._noise)
        _lib.check(lib.hiprec_simgcl_grad(ctypes.byref(plan), _lib.ptr(users), _lib.ptr(pos), _lib.ptr(neg), B,
                                          _lib.ptr(self._parts), _lib.ptr(self._stats), _lib.ptr(self._scratch),
                                          self._scratch.numel(), _lib.stream_ptr(dev)))
        m._ws["clock"] += 1                  # the finishing kernel advanced the device's

    def last_losses(self):
        """``(bpr, reg, cl_user, cl_item)`` of the last step (one host sync); the loss is ``bpr + reg + lambda *
        (cl_user + cl_item)``."""
        p = self._parts.cpu().numpy()
        return float(p[0]), float(p[1]), float(p[2]), float(p[3])

    def backward_only(self, batch_data, noise=None):
        """zero_grad + forward + loss + backward without the optimizer step: ``(loss, grads)``."""
        self._setup()
        self._noise = self._checked_noise(noise)
        try:
            return super().backward_only(batch_data)
        finally:
            self._noise = None

    def train_single_batch(self, batch_data, noise=None):
        """simgcl.py:101-133: one step, returns the batch loss as a float."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._setup()
        self._noise = self._checked_noise(noise)
        try:
            self._enqueue_step(batch_data)
            return self._sync_stats().loss
        finally:
            self._noise = None

    def train_an_epoch(self, train_loader, epoch_id):
        """simgcl.py:135-151: every batch; prints the last batch's loss, logs the epoch sum."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        st = self._run_epoch(train_loader)
        print(f"[Training Epoch {epoch_id}], Loss {st.loss}")
        self.writer.add_scalar("model/loss", st.loss_sum, epoch_id)
        self.writer.add_scalar("model/regularizer", 0.0, epoch_id)
