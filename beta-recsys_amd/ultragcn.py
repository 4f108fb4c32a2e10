"""Drop-in ``UltraGCN`` / ``UltraGCNEngine`` for beta_rec/models/ultragcn.py on libhiprec.so.

The one graph-CF model of the reference that needs no propagation: two embedding tables, a weighted BCE over one
positive and N sampled negatives per sample, and an item-item constraint over K precomputed neighbours -- the consumer
of ``data.instance_mul_neg_loader``'s ``(user, pos_item, neg_items[N])`` batches.  Interface parity (file:line =
beta_rec/...): ``get_ii_constraint_mat`` models/ultragcn.py:9-33, ``UltraGCN(config)`` :36-179 (``forward(users, pos,
neg) -> loss``, ``predict(users, items)``), ``UltraGCNEngine(config)`` :182-236 (``train_single_batch(batch) -> float``,
``train_an_epoch(loader, epoch_id)``).  Same config keys (``n_users n_items emb_dim w1 w2 w3 w4 negative_weight gamma
lambda train_mat constraint_mat ii_neighbor_num`` under ``config["model"]`` next to ``regs optimizer lr device_str``),
same ``state_dict`` keys, same initial weights for the same torch seed.

Kept from the reference on purpose:
* the loss is a SUM over the batch; only the negatives are averaged (over N);
* ``gamma * norm_loss`` covers every row of both tables in every step, so all three optimizers move every element;
* ``config["model"]["regs"]`` is read and never used;
* ``w4 <= 0`` makes every negative weight the constant ``w3``.
Not kept: with ``w2 <= 0`` the reference dies with ``NameError`` (``pow_weight`` is never bound, ultragcn.py:73-81); the
mirror raises a ``ValueError`` that says so at construction.

Extension: ``config["model"]`` may carry precomputed ``ii_neighbor_mat`` / ``ii_constraint_mat`` ([n_items, K] each);
``train_mat`` is then not needed.

Forward, loss, backward and predict run in ``csrc/ultragcn.hip``; the gamma term's gradient rides in the optimizer sweep
(``hiprec_opt_dense_step_decay``, optim.hip's arithmetic in a sweep of its own).  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .data import DeviceTensorBatcher
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor


def get_ii_constraint_mat(train_mat, num_neighbors, ii_diagonal_zero=False):
    """models/ultragcn.py:9-33: per item the ``num_neighbors`` largest entries of ``Omega = (beta_u' beta_i'^T) o A``,
    ``A = M^T M``, as ``(ii_neighbor_mat int64 [I, K], ii_constraint_mat float32 [I, K])``.

    The reference multiplies a DENSE I x I outer product row by row; here only the stored entries of ``A`` are ever
    formed (the same three fp32 operations per entry, so the same bits).  ``torch.topk`` breaks ties in an unspecified
    order, and a row with fewer than K co-occurring items is padded with ``sim = 0`` entries whose ids are arbitrary
    there (zero loss, zero gradient); here ties go to the smaller item id and the padding carries the row's own id."""
    import scipy.sparse as sp

    print("Computing \\Omega for the item-item graph... ")
    M = sp.csr_matrix(train_mat)
    A = sp.csr_matrix(M.T.dot(M))
    n_items, K = A.shape[0], int(num_neighbors)
    if ii_diagonal_zero:
        A.setdiag(0)
    A.eliminate_zeros()
    A.sort_indices()
    items_D = np.asarray(A.sum(axis=0)).reshape(-1)
    users_D = np.asarray(A.sum(axis=1)).reshape(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        beta_uD = np.sqrt(users_D + 1) / users_D
        beta_iD = 1 / np.sqrt(items_D + 1)
    rows = np.repeat(np.arange(n_items), np.diff(A.indptr))
    vals = (beta_uD[rows] * beta_iD[A.indices]) * A.data
    order = np.lexsort((A.indices, -vals, rows))
    rank = np.arange(rows.size) - A.indptr[rows]          # position inside the row, rows being contiguous in `order`
    keep = rank < K
    res_mat = np.repeat(np.arange(n_items, dtype=np.int64)[:, None], K, axis=1)
    res_sim_mat = np.zeros((n_items, K), dtype=np.float32)
    res_mat[rows[keep], rank[keep]] = A.indices[order][keep]
    res_sim_mat[rows[keep], rank[keep]] = vals[order][keep]
    print("Computation \\Omega OK!")
    return torch.from_numpy(res_mat).long(), torch.from_numpy(res_sim_mat).float()


class UltraGCN(_FlatModel):
    """models/ultragcn.py:36-179.  Flat buffer: [user_embeds | item_embeds]."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.user_num = int(config["n_users"])
        self.item_num = int(config["n_items"])
        self.emb_dim = int(config["emb_dim"])
        self.w1, self.w2, self.w3, self.w4 = (float(config[k]) for k in ("w1", "w2", "w3", "w4"))
        if not self.w2 > 0:
            raise ValueError(
                f"w2 = {self.w2!r}: the reference has no meaning for w2 <= 0 (get_omegas never binds pow_weight and "
                "raises NameError, models/ultragcn.py:73-81)")
        self.negative_weight = float(config["negative_weight"])
        self.gamma = float(config["gamma"])
        self.lambda_ = float(config["lambda"])
        U, I, D = self.user_num, self.item_num, self.emb_dim
        v = self._build([("user_embeds.weight", (U, D)), ("item_embeds.weight", (I, D))])
        # RNG order of ultragcn.py:50-51,68-70: two nn.Embedding (N(0,1) each), then normal_(std=1e-3) twice
        v["user_embeds.weight"].normal_(0, 1)
        v["item_embeds.weight"].normal_(0, 1)
        self.user_embeds = _ParamView(v["user_embeds.weight"])
        self.item_embeds = _ParamView(v["item_embeds.weight"])

        cm = config["constraint_mat"]
        self.constraint_mat = {
            "beta_uD": torch.from_numpy(np.asarray(cm["beta_uD"], dtype=np.float32).reshape(-1).copy()),
            "beta_iD": torch.from_numpy(np.asarray(cm["beta_iD"], dtype=np.float32).reshape(-1).copy())}
        if self.constraint_mat["beta_uD"].numel() != U or self.constraint_mat["beta_iD"].numel() != I:
            raise ValueError("constraint_mat: beta_uD / beta_iD must hold one value per user / item")
        self.train_mat = config["train_mat"] if "train_mat" in config else None
        self.ii_neighbor_num = int(config["ii_neighbor_num"])
        if "ii_neighbor_mat" in config and "ii_constraint_mat" in config:
            nbr = torch.as_tensor(np.asarray(config["ii_neighbor_mat"])).long()
            sim = torch.as_tensor(np.asarray(config["ii_constraint_mat"])).float()
        else:
            nbr, sim = get_ii_constraint_mat(self.train_mat, self.ii_neighbor_num)
        if tuple(nbr.shape) != (I, self.ii_neighbor_num) or tuple(sim.shape) != (I, self.ii_neighbor_num):
            raise ValueError(f"ii_neighbor_mat / ii_constraint_mat must be [{I}, {self.ii_neighbor_num}]")
        if self.ii_neighbor_num and (int(nbr.min()) < 0 or int(nbr.max()) >= I):
            raise ValueError("ii_neighbor_mat holds ids outside [0, n_items)")
        self.ii_neighbor_mat, self.ii_constraint_mat = nbr.contiguous(), sim.contiguous()
        self.initial_weights()
        self._consts = None

    def initial_weights(self):
        """ultragcn.py:68-70."""
        v = self.views()
        v["user_embeds.weight"].normal_(0, 1e-3)
        v["item_embeds.weight"].normal_(0, 1e-3)

    # ---- device-side constants and argument blocks -------------------------------------------------------
    def tables(self, flat=None):
        """hiprec_ultragcn_tables over the weight buffer (or a same-shaped gradient buffer)."""
        flat = self._flat if flat is None else flat
        base = flat.data_ptr()
        return _lib.UltraGcnTables(base, base + 4 * self.user_num * self.emb_dim, self.user_num, self.item_num,
                                   self.emb_dim, 0)

    def params(self):
        """hiprec_ultragcn_params; beta vectors and neighbour tables are copied to the weights' device once."""
        dev = self._flat.device
        if self._consts is None or self._consts[0].device != dev:
            self._consts = tuple(t.to(dev).contiguous() for t in (
                self.constraint_mat["beta_uD"], self.constraint_mat["beta_iD"], self.ii_neighbor_mat,
                self.ii_constraint_mat))
        bu, bi, nbr, sim = self._consts
        K = self.ii_neighbor_num
        return _lib.UltraGcnParams(bu.data_ptr(), bi.data_ptr(), nbr.data_ptr() if K else None,
                                   sim.data_ptr() if K else None, K, self.w1, self.w2, self.w3, self.w4,
                                   self.negative_weight, self.gamma, self.lambda_)

    def batch_tensors(self, users, pos_items, neg_items):
        """``(users[B], pos[B], neg[B, N])`` as contiguous int64 tensors on the weights' device, and ``N``."""
        dev = self._flat.device
        users_t, pos_t = index_tensor(users, dev), index_tensor(pos_items, dev)
        neg = neg_items if torch.is_tensor(neg_items) else np.asarray(neg_items)
        B = users_t.numel()
        if B == 0:
            raise ValueError("empty batch")
        if pos_t.numel() != B:
            raise ValueError("users and pos_items differ in length")
        if neg.ndim != 2 or neg.shape[0] != B or neg.shape[1] < 1:
            raise ValueError("neg_items must be [batch, n_neg] with n_neg >= 1")
        return users_t, pos_t, index_tensor(neg, dev).view(neg.shape), int(neg.shape[1])

    # ---- reference API -----------------------------------------------------------------------------------
    def get_omegas(self, users, pos_items, neg_items):
        """ultragcn.py:72-100 on caller-supplied ids (utility, fp32 on the CPU copies of beta; the training kernel
        forms the same weights from ``beta_uD[u]`` / ``beta_iD[i]`` itself): ``cat(pos_weight[B], neg_weight[B*N])``."""
        bu, bi = self.constraint_mat["beta_uD"], self.constraint_mat["beta_iD"]
        users, pos_items, neg_items = (torch.as_tensor(x).long().cpu() for x in (users, pos_items, neg_items))
        pos_weight = self.w1 + self.w2 * (bu[users] * bi[pos_items])
        if self.w4 > 0:
            neg_weight = self.w3 + self.w4 * (torch.repeat_interleave(bu[users], neg_items.size(1)) * bi[neg_items.flatten()])
        else:
            neg_weight = self.w3 * torch.ones(neg_items.numel())
        return torch.cat((pos_weight, neg_weight))

    def forward(self, users, pos_items, neg_items):
        """ultragcn.py:159-165: the batch loss as a 0-dim tensor (no autograd graph: training goes through
        ``UltraGCNEngine.train_single_batch``, which keeps the gradient this call discards)."""
        lib = self._require_hip()
        dev = self._flat.device
        stats = self._device_stats()
        g = torch.zeros_like(self._flat)
        scratch = torch.zeros(lib.hiprec_scratch_bytes(0), dtype=torch.uint8, device=dev)
        sumsq = torch.zeros(lib.hiprec_sumsq_workspace_bytes() // 8, dtype=torch.float64, device=dev)
        enqueue_grad(lib, self, g, (users, pos_items, neg_items), sumsq, stats, scratch)
        _lib.check(lib.hiprec_finalize_stats(_lib.ptr(stats), _lib.ptr(scratch), None, None, _lib.stream_ptr(dev)))
        return torch.tensor(self._check_status().loss, device=dev)

    def ranking_factors(self):
        """``(U, I, 1.0, None)`` for full-catalogue ranking (``recommend.recommend``): the two tables; ``predict`` is
        their dot product."""
        self._require_hip()
        return self.user_embeds.weight.data, self.item_embeds.weight.data, 1.0, None

    def predict(self, users, items):
        """ultragcn.py:167-179."""
        lib = self._require_hip()
        dev = self._flat.device
        users_t, items_t = index_tensor(users, dev), index_tensor(items, dev)
        if users_t.numel() != items_t.numel():
            raise ValueError("users and items differ in length")
        stats = self._device_stats()
        scores = torch.empty(users_t.numel(), dtype=torch.float32, device=dev)
        w = self.tables()
        _lib.check(lib.hiprec_ultragcn_predict(ctypes.byref(w), _lib.ptr(users_t), _lib.ptr(items_t), users_t.numel(),
                                               _lib.ptr(scores), _lib.ptr(stats), _lib.stream_ptr(dev)))
        self._check_status()
        return scores


def enqueue_grad(lib, model, g_flat, batch_data, sumsq_ws, stats, scratch):
    """Sum of squares of the current weights (they may have been replaced since the last sweep), then forward + loss +
    backward of one batch into ``g_flat`` -- everything but the gamma term's gradient."""
    users, pos, neg, n_neg = model.batch_tensors(*batch_data)
    w, g, p = model.tables(), model.tables(g_flat), model.params()
    st = _lib.stream_ptr(model.flat.device)
    _lib.check(lib.hiprec_sumsq(_lib.ptr(model.flat), model.flat.numel(), _lib.ptr(sumsq_ws), sumsq_ws.numel() * 8, st))
    _lib.check(lib.hiprec_ultragcn_grad(
        ctypes.byref(w), ctypes.byref(g), ctypes.byref(p), _lib.ptr(users), _lib.ptr(pos), _lib.ptr(neg), users.numel(),
        n_neg, _lib.ptr(sumsq_ws), _lib.ptr(stats), _lib.ptr(scratch), scratch.numel(), st))


class UltraGCNEngine(FlatModelEngine):
    """models/ultragcn.py:182-236."""

    def __init__(self, config):
        self.config = config
        self.regs = config["model"]["regs"]  # read and never used, as in the reference
        self.decay = self.regs[0]
        self.model = UltraGCN(config["model"])
        super(UltraGCNEngine, self).__init__(config)

    def _alloc_extra(self, lib, dev):
        self._sumsq_ws = torch.zeros(lib.hiprec_sumsq_workspace_bytes() // 8, dtype=torch.float64, device=dev)

    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        if len(batch_data) != 3:
            raise ValueError("UltraGCN batches are (users, pos_items, neg_items[B, N])")
        enqueue_grad(lib, self.model, self._g_flat, batch_data, self._sumsq_ws, self._stats, self._scratch)

    def _enqueue_opt(self, fold_partials=True):
        """optimizer.step() with gamma * w added to every element's gradient inside the sweep."""
        lib, m, opt = _lib.load(), self.model, self.optimizer
        _lib.check(lib.hiprec_opt_dense_step_decay(
            opt.kind, _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(opt.exp_avg), _lib.ptr(opt.exp_avg_sq),
            m.flat.numel(), opt.lr, opt.beta1, opt.beta2, opt.eps, _lib.ptr(self._stats),
            _lib.ptr(self._scratch) if fold_partials else None, m.gamma, _lib.ptr(self._sumsq_ws),
            self._sumsq_ws.numel() * 8, _lib.stream_ptr(m.flat.device)))

    def backward_only(self, batch_data):
        """zero_grad + forward + loss + backward without the optimizer step: ``(loss, grads)``, the gradients
        INCLUDING the gamma term (which a training step never writes out: its sweep adds it on the fly)."""
        self._enqueue_grad(batch_data)
        m = self.model
        _lib.check(_lib.load().hiprec_decay_grad(_lib.ptr(self._g_flat), _lib.ptr(m.flat), m.flat.numel(), m.gamma,
                                                 _lib.stream_ptr(m.flat.device)))
        st, grads = self._finish_backward_only()
        return st.loss, grads

    def train_single_batch(self, batch_data):
        """ultragcn.py:196-216: one step on ``(users, pos_items, neg_items[B, N])``, returns ``batch_loss.item()``.
        Out-of-range ids raise IndexError and leave the tables as they were."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_step(batch_data)
        return self._sync_stats().loss

    def enqueue_epoch(self, users, pos, neg, batch_size):
        """One epoch over resident device arrays in visiting order (``users[n]``, ``pos[n]``, ``neg[n, N]``; batches of
        ``batch_size``, the last one short), enqueued by ``hiprec_ultragcn_epoch`` with no host work between steps and
        no sync."""
        lib = self._setup()
        m, opt = self.model, self.optimizer
        users, pos, neg, n_neg = m.batch_tensors(users, pos, neg)
        w, g, p = m.tables(), m.tables(self._g_flat), m.params()
        _lib.check(lib.hiprec_ultragcn_epoch(
            ctypes.byref(w), ctypes.byref(g), ctypes.byref(p), _lib.ptr(users), _lib.ptr(pos), _lib.ptr(neg),
            users.numel(), int(batch_size), n_neg, opt.kind, opt.lr, opt.beta1, opt.beta2, opt.eps, _lib.ptr(m.flat),
            _lib.ptr(self._g_flat), _lib.ptr(opt.exp_avg), _lib.ptr(opt.exp_avg_sq), m.flat.numel(),
            _lib.ptr(self._sumsq_ws), self._sumsq_ws.numel() * 8, _lib.ptr(self._stats), _lib.ptr(self._scratch),
            self._scratch.numel(), _lib.stream_ptr(m.flat.device)))

    def train_an_epoch(self, train_loader, epoch_id):
        """ultragcn.py:218-236: ``train_loader`` yields ``(users, pos_items, neg_items)`` batches; prints the LAST
        batch's loss and logs the epoch sum.  A ``DeviceTensorBatcher`` (``data.instance_mul_neg_loader``) is run
        resident: one device-side permutation, one gather, the whole epoch enqueued from C, one host sync.  Any other
        iterable is collected first (every batch but the last of one size)."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        self._setup()
        dev = self.model.flat.device
        if isinstance(train_loader, DeviceTensorBatcher) and len(train_loader.tensors) == 3:
            perm = train_loader.permutation()
            cols = [t.to(dev) if perm is None else t.to(dev)[perm] for t in train_loader.tensors]
            batch_size = train_loader.batch_size
        else:
            blocks = [self.model.batch_tensors(*b)[:3] for b in train_loader]
            if not blocks:
                raise ValueError("empty epoch")
            batch_size = blocks[0][0].numel()
            self._check_blocks([b[0].numel() for b in blocks], batch_size, "the same number of samples")
            if len({b[2].shape[1] for b in blocks}) != 1:
                raise ValueError("batches differ in the number of negatives")
            cols = [torch.cat([b[k] for b in blocks]) for k in range(3)]
        if cols[0].numel() == 0:
            raise ValueError("empty epoch")
        self.enqueue_epoch(cols[0], cols[1], cols[2], batch_size)
        st = self._sync_stats()
        print("[Training Epoch {}], Loss {}".format(epoch_id, st.loss))
        self.writer.add_scalar("model/loss", st.loss_sum, epoch_id)
