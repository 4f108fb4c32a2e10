"""Drop-in ``CollaborativeMemoryNetwork`` / ``cmnEngine`` for beta_rec/models/cmn.py on libhiprec.so.

The model ``PairwiseGMF`` (``pairwise_gmf.py``) pre-trains: its two tables are handed to
``cmnEngine(config, user_embeddings, item_embeddings, item_user_list)`` (examples/train_cmn.py:100-108), which adds an
output memory, a two-hop attention over each item's neighbourhood (the users who interacted with it) and a small
output module.  Interface parity (file:line = beta_rec/...): ``CollaborativeMemoryNetwork(config, user_embeddings,
item_embeddings, item_user_list, device)`` models/cmn.py:12-132 (the seven-argument ``forward(..., evaluation=)``,
``predict(users, items)``), ``VariableLengthMemoryLayer`` models/vlml.py (its ``hop_mapping`` only: the layer's
arithmetic lives in the kernel), ``cmnEngine`` :135-275 (``train_single_batch(batch) -> float``, ``train_an_epoch``,
its own ``bpr_loss``).  Same FLAT config keys as the reference reads (``emb_dim device_str regs batch_size lr momentum
training_l2_lambda grad_clip neg_count``) next to ``config["model"]`` / ``config["system"]`` which its base class reads;
same ``state_dict`` keys and the same constructed weights for the same torch seed.

Kept from the reference on purpose:
* the L2 term is ``lambda * ||W||_2`` (the norm, not its square) and covers ``mem_layer.hop_mapping.1.weight`` ONLY: of
  the three names cmn.py:188-195 tests, the other two (``output_module.dense.weight``, ``output_module.out.weight``)
  name no parameter of the model;
* the optimizer is ``RMSprop(lr=config["lr"], momentum=config["momentum"])`` unless ``config["model"]["optimizer"]``
  names ``sgd`` / ``adam`` / ``rmsprop`` (``cmn_default.json`` says adam);
* ``predict`` is the plain dot product of the two memories: the memory network takes no part in evaluation.

Forward, loss and backward run in ``csrc/cmn.hip``; the gradient-norm clip and the optimizer sweep are the shared
``csrc/pgmf.hip`` / ``csrc/optim.hip``.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .data import DeviceTensorBatcher
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor
from .pairwise_gmf import truncated_normal_
from .torch_engine import HipOptimizer


class VariableLengthMemoryLayer(nn.Module):
    """models/vlml.py:7-26: the container of the hop mappings (``hop_mapping["1"]`` for two hops); parameters are
    views of the model's flat buffer."""

    def __init__(self, hops, emb_dim, device, mappings):
        super().__init__()
        self.hops = hops
        self.device = device
        self.emb_dim = emb_dim
        self.hop_mapping = nn.ModuleDict(mappings)


def neighborhood_csr(item_user_list, n_items):
    """The item -> users CSR of ``item_user_list`` (a dict item id -> list of user ids), one row per item of the table,
    every list in its own order; an item the dict does not hold gets the one-entry list ``[item id]``, which is what
    ``cmn_train_loader`` feeds for it (data/deprecated_data.py:831-847).  ``(rowptr int64 [n_items + 1], col int64)``."""
    lens = np.ones(n_items, dtype=np.int64)
    for i, lst in item_user_list.items():
        if not 0 <= int(i) < n_items:
            raise IndexError(f"item_user_list holds item {i}, outside [0, {n_items})")
        lens[int(i)] = len(lst)
        if len(lst) < 1:
            raise ValueError(f"item_user_list[{i}] is empty")
    rowptr = np.zeros(n_items + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = np.empty(int(rowptr[-1]), dtype=np.int64)
    known = np.zeros(n_items, dtype=bool)
    for i, lst in item_user_list.items():
        col[rowptr[int(i)]:rowptr[int(i) + 1]] = np.asarray(lst, dtype=np.int64)
        known[int(i)] = True
    missing = np.nonzero(~known)[0]
    col[rowptr[missing]] = missing
    return torch.from_numpy(rowptr), torch.from_numpy(col)


class CollaborativeMemoryNetwork(_FlatModel):
    """models/cmn.py:12-132.  Flat buffer, in ``named_parameters()`` order:
    [user_memory | item_memory | user_output | hop W | hop b | dense W | dense b | out w]."""

    def __init__(self, config, user_embeddings, item_embeddings, item_user_list, device):
        super().__init__()
        self.config = config
        self.device = device
        self.emb_dim = int(config["emb_dim"])
        self.neighborhood = item_user_list
        self.max_neighbors = max([len(x) for x in item_user_list.values()])
        config["max_neighbors"] = self.max_neighbors
        ue = torch.as_tensor(np.asarray(user_embeddings), dtype=torch.float32)
        ie = torch.as_tensor(np.asarray(item_embeddings), dtype=torch.float32)
        U, I, D = ue.shape[0], ie.shape[0], self.emb_dim
        if ue.shape[1] != D or ie.shape[1] != D:
            raise ValueError(f"the pre-trained tables must be [*, emb_dim = {D}]")
        self.n_users, self.n_items = int(U), int(I)
        v = self._build([("user_memory.weight", (U, D)), ("item_memory.weight", (I, D)),
                         ("user_output.weight", (U, D)),
                         ("mem_layer.hop_mapping.1.weight", (D, D)), ("mem_layer.hop_mapping.1.bias", (D,)),
                         ("dense.weight", (D, 2 * D)), ("dense.bias", (D,)), ("out.weight", (1, D))])
        # RNG order of cmn.py:29-61 / vlml.py:18-25: nn.Embedding's own N(0,1) for each of the three tables (the first
        # two are then replaced by the pre-trained tables, the third by a truncated normal), nn.Linear's default init
        # followed by kaiming_normal_ (bias 1.0) for the hop mapping and the dense layer, nn.Linear's default init
        # followed by xavier_uniform_ for the output weight
        v["user_memory.weight"].normal_(0, 1)
        v["user_memory.weight"].copy_(ue)
        v["item_memory.weight"].normal_(0, 1)
        v["item_memory.weight"].copy_(ie)
        v["user_output.weight"].normal_(0, 1)
        truncated_normal_(v["user_output.weight"], std=0.01)
        for wname, bname, fan_in in (("mem_layer.hop_mapping.1.weight", "mem_layer.hop_mapping.1.bias", D),
                                     ("dense.weight", "dense.bias", 2 * D)):
            lin = nn.Linear(fan_in, D, bias=True)
            nn.init.kaiming_normal_(lin.weight)
            v[wname].copy_(lin.weight.data)
            v[bname].fill_(1.0)
        lin = nn.Linear(D, 1, bias=False)
        nn.init.xavier_uniform_(lin.weight)
        v["out.weight"].copy_(lin.weight.data)
        self.user_memory = _ParamView(v["user_memory.weight"])
        self.item_memory = _ParamView(v["item_memory.weight"])
        self.user_output = _ParamView(v["user_output.weight"])
        self.mem_layer = VariableLengthMemoryLayer(
            2, D, device, {"1": _ParamView(v["mem_layer.hop_mapping.1.weight"], v["mem_layer.hop_mapping.1.bias"])})
        self.dense = _ParamView(v["dense.weight"], v["dense.bias"])
        self.out = _ParamView(v["out.weight"])
        self._csr_host = None
        self._csr = None

    def _owner(self, name):
        mod = self
        parts = name.split(".")
        for p in parts[:-1]:
            mod = mod[p] if isinstance(mod, nn.ModuleDict) else getattr(mod, p)
        return mod, parts[-1]

    # ---- device-side argument blocks ---------------------------------------------------------------------
    def tables(self, flat=None):
        """hiprec_cmn_tables over the weight buffer (or a same-shaped gradient buffer)."""
        flat = self._flat if flat is None else flat
        base = flat.data_ptr()
        ptrs = [base + 4 * self.offset_of(n) for n, _ in self._spec]
        return _lib.CmnTables(*ptrs, self.n_users, self.n_items, self.emb_dim, 0)

    def csr(self):
        """``(rowptr, col)`` of the constructor's ``item_user_list`` on the weights' device, built once."""
        dev = self._flat.device
        if self._csr_host is None:
            self._csr_host = neighborhood_csr(self.neighborhood, self.n_items)
        if self._csr is None or self._csr[0].device != dev:
            self._csr = tuple(t.to(dev) for t in self._csr_host)
        return self._csr

    def batch_tensors(self, batch_data, sides=2):
        """The seven arrays of cmn.py:166-174 (tensors on any device, numpy or lists) as contiguous int64 tensors on
        the weights' device: ``users[B] pos[B] neg[B] pos_nbr[B, Lp] pos_len[B] neg_nbr[B, Ln] neg_len[B]``."""
        dev = self._flat.device
        if len(batch_data) != 7:
            raise ValueError("a CMN batch is (users, items, neg_items, neighborhoods, lengths, neg_neighborhoods, "
                             "neg_lengths)")
        users, pos, neg, pn, pl, nn_, nl = batch_data
        users_t, pos_t, pl_t = (index_tensor(x, dev) for x in (users, pos, pl))
        B = users_t.numel()
        if B == 0:
            raise ValueError("empty batch")

        def matrix(x):
            x = x if torch.is_tensor(x) else np.asarray(x)
            if x.ndim != 2 or x.shape[0] != B or x.shape[1] < 1:
                raise ValueError("neighborhoods must be [batch, padded length >= 1]")
            return index_tensor(x, dev).view(x.shape[0], x.shape[1])

        pn_t = matrix(pn)
        if pos_t.numel() != B or pl_t.numel() != B:
            raise ValueError("batch tensors differ in length")
        if sides == 1:
            return users_t, pos_t, None, pn_t, pl_t, None, None
        neg_t, nl_t = index_tensor(neg, dev), index_tensor(nl, dev)
        nn_t = matrix(nn_)
        if neg_t.numel() != B or nl_t.numel() != B:
            raise ValueError("batch tensors differ in length")
        return users_t, pos_t, neg_t, pn_t, pl_t, nn_t, nl_t

    # ---- reference API -----------------------------------------------------------------------------------
    def forward(self, input_users, input_items, input_items_negative, input_neighborhoods,
                input_neighborhood_lengths, input_neighborhoods_negative, input_neighborhood_lengths_negative,
                evaluation=False):
        """cmn.py:69-121 without autograd: the positive scores ``[B]`` when ``evaluation``, else ``(pos, neg)``."""
        lib = self._require_hip()
        dev = self._flat.device
        stats = self._device_stats()
        u, p, n, pn, pl, nn_, nl = self.batch_tensors(
            (input_users, input_items, input_items_negative, input_neighborhoods, input_neighborhood_lengths,
             input_neighborhoods_negative, input_neighborhood_lengths_negative), 1 if evaluation else 2)
        B = u.numel()
        pos_s = torch.empty(B, dtype=torch.float32, device=dev)
        neg_s = None if evaluation else torch.empty(B, dtype=torch.float32, device=dev)
        w = self.tables()
        _lib.check(lib.hiprec_cmn_grad_padded(
            ctypes.byref(w), None, _lib.ptr(u), _lib.ptr(p), _lib.ptr(n), _lib.ptr(pn), _lib.ptr(pl), pn.shape[1],
            _lib.ptr(nn_), _lib.ptr(nl), 0 if evaluation else nn_.shape[1], B, 1.0 / B, 0.0, _lib.ptr(pos_s),
            _lib.ptr(neg_s), _lib.ptr(stats), None, 0, None, 0, _lib.stream_ptr(dev)))
        self._check_status()
        return pos_s if evaluation else (pos_s, neg_s)

    def ranking_factors(self):
        """``(M, E, 1.0, None)`` for full-catalogue ranking (``recommend.recommend``): ``predict`` is their dot
        product."""
        self._require_hip()
        return self.user_memory.weight.data, self.item_memory.weight.data, 1.0, None

    def predict(self, users, items):
        """cmn.py:123-132: ``sum_d M[u] * E[i]`` (the two-table dot-product kernel UltraGCN's predict uses)."""
        lib = self._require_hip()
        dev = self._flat.device
        users_t, items_t = index_tensor(users, dev), index_tensor(items, dev)
        if users_t.numel() != items_t.numel():
            raise ValueError("users and items differ in length")
        stats = self._device_stats()
        scores = torch.empty(users_t.numel(), dtype=torch.float32, device=dev)
        base = self._flat.data_ptr()
        w = _lib.UltraGcnTables(base, base + 4 * self.offset_of("item_memory.weight"), self.n_users, self.n_items,
                                self.emb_dim, 0)
        _lib.check(lib.hiprec_ultragcn_predict(ctypes.byref(w), _lib.ptr(users_t), _lib.ptr(items_t), users_t.numel(),
                                               _lib.ptr(scores), _lib.ptr(stats), _lib.stream_ptr(dev)))
        self._check_status()
        return scores


class cmnEngine(FlatModelEngine):   # noqa: N801  (the reference's name)
    """models/cmn.py:135-275."""

    def __init__(self, config, user_embeddings, item_embeddings, item_user_list):
        self.config = config
        self.device = config["device_str"]
        self.model = CollaborativeMemoryNetwork(config, user_embeddings, item_embeddings, item_user_list, self.device)
        self.regs = config["regs"]  # read and never used, as in the reference
        self.batch_size = config["batch_size"]
        # cmn.py:147-149 builds RMSprop(lr, momentum); ModelEngine.__init__ then replaces it when
        # config["model"]["optimizer"] names one of sgd/adam/rmsprop (torch_engine.py:23-39)
        self.optimizer = HipOptimizer("rmsprop", config["lr"], momentum=config["momentum"])
        self._ws = None
        super(cmnEngine, self).__init__(config)

    def set_optimizer(self):
        name = self.config["model"]["optimizer"] if "optimizer" in self.config["model"] else None
        if name in _lib.OPT_KINDS:
            self.optimizer = HipOptimizer(name, self.config["model"]["lr"])

    def _alloc_extra(self, lib, dev):
        self._ws = None
        self._clip_ws = torch.zeros(lib.hiprec_clip_workspace_bytes() // 8, dtype=torch.float64, device=dev)

    def _workspace(self, lib, batch):
        need = lib.hiprec_cmn_workspace_bytes(self.model.emb_dim, int(batch))
        self._ws = _lib.grow(self._ws, need, torch.uint8, self.model.flat.device)
        return self._ws

    def _l2_lambda(self):
        # data-parallel replicas: the lambda ||W|| term (loss and gradient) is added once, on rank 0
        return float(self.config["training_l2_lambda"]) if self._dp_rank == 0 else 0.0

    @staticmethod
    def _seven(batch_data):
        """A loader batch ``(ratings[B, 3], pos_nbr, pos_len, neg_nbr, neg_len)`` (cmn.py:223-261) as the seven arrays."""
        if len(batch_data) != 5:
            return batch_data
        ratings, pn, pl, nn_, nl = batch_data
        ratings = ratings if torch.is_tensor(ratings) else np.asarray(ratings)
        return ratings[:, 0], ratings[:, 1], ratings[:, 2], pn, pl, nn_, nl

    def _enqueue_grad(self, batch_data, clip=True):
        """Seven arrays (or a loader's 5-tuple): the padded lists as given.  Three arrays ``(users, pos, neg)``: each
        item's list from the constructor's ``item_user_list`` (the CSR form)."""
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        w, g = m.tables(), m.tables(self._g_flat)
        st = _lib.stream_ptr(dev)
        tail = lambda B: (B, self._batch_share() / B, self._l2_lambda(), None, None, _lib.ptr(self._stats),   # noqa: E731
                          _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(self._workspace(lib, B)),
                          self._ws.numel(), st)
        if len(batch_data) == 3:
            users, pos, neg = (index_tensor(x, dev) for x in batch_data)
            if not (users.numel() == pos.numel() == neg.numel()):
                raise ValueError("batch tensors differ in length")
            if users.numel() == 0:
                raise ValueError("empty batch")
            rowptr, col = m.csr()
            _lib.check(lib.hiprec_cmn_grad_csr(ctypes.byref(w), ctypes.byref(g), _lib.ptr(users), _lib.ptr(pos),
                                               _lib.ptr(neg), _lib.ptr(rowptr), _lib.ptr(col), *tail(users.numel())))
        else:
            u, p, n, pn, pl, nn_, nl = m.batch_tensors(self._seven(batch_data))
            _lib.check(lib.hiprec_cmn_grad_padded(
                ctypes.byref(w), ctypes.byref(g), _lib.ptr(u), _lib.ptr(p), _lib.ptr(n), _lib.ptr(pn), _lib.ptr(pl),
                pn.shape[1], _lib.ptr(nn_), _lib.ptr(nl), nn_.shape[1], *tail(u.numel())))
        if clip:
            _lib.check(lib.hiprec_clip_grad_norm(
                _lib.ptr(self._g_flat), self._g_flat.numel(), float(self.config["grad_clip"]),
                _lib.ptr(self._clip_ws), self._clip_ws.numel() * 8, st))

    def _enqueue_step(self, batch_data):
        """grad, then clip_grad_norm_ + optimizer.step() as one sums-of-squares launch and one sweep."""
        self._enqueue_grad(batch_data, clip=False)
        lib, m, opt = _lib.load(), self.model, self.optimizer
        _lib.check(lib.hiprec_clip_opt_dense_step(
            opt.kind, _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(opt.exp_avg), _lib.ptr(opt.exp_avg_sq),
            m.flat.numel(), opt.lr, opt.beta1, opt.beta2, opt.eps, _lib.ptr(self._stats), _lib.ptr(self._scratch), -1,
            float(self.config["grad_clip"]), _lib.ptr(self._clip_ws), self._clip_ws.numel() * 8,
            _lib.stream_ptr(m.flat.device)))

    def backward_only(self, batch_data, clip=True):
        """zero_grad + forward + loss + backward (+ clip) without the optimizer step:
        ``(loss, grads, total_norm)``; ``total_norm`` is None when ``clip`` is False."""
        self._enqueue_grad(batch_data, clip)
        st, grads = self._finish_backward_only()
        return st.loss, grads, (float(self._clip_ws[0]) if clip else None)

    def train_single_batch(self, batch_data):
        """cmn.py:153-200: one step on the seven arrays, returns ``batch_loss.item()``."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_step(batch_data)
        return self._sync_stats().loss

    def enqueue_epoch(self, users, pos, neg):
        """One epoch over resident device triples in visiting order (batches of ``batch_size``, the last one short),
        the lists from the item -> users CSR, enqueued by ``hiprec_cmn_epoch`` with no host work between steps and
        no sync."""
        lib = self._setup()
        m, opt = self.model, self.optimizer
        dev = m.flat.device
        users, pos, neg = (index_tensor(x, dev) for x in (users, pos, neg))
        if not (users.numel() == pos.numel() == neg.numel()):
            raise ValueError("epoch arrays differ in length")
        if self._dp_world != 1:
            raise NotImplementedError("the resident CMN epoch is single-process; replicas step batch by batch")
        w, g = m.tables(), m.tables(self._g_flat)
        rowptr, col = m.csr()
        ws = self._workspace(lib, min(int(self.batch_size), max(1, users.numel())))
        _lib.check(lib.hiprec_cmn_epoch(
            ctypes.byref(w), ctypes.byref(g), _lib.ptr(users), _lib.ptr(pos), _lib.ptr(neg), _lib.ptr(rowptr),
            _lib.ptr(col), users.numel(), int(self.batch_size), self._l2_lambda(), float(self.config["grad_clip"]),
            opt.kind, opt.lr, opt.beta1, opt.beta2, opt.eps, _lib.ptr(m.flat), _lib.ptr(self._g_flat),
            _lib.ptr(opt.exp_avg), _lib.ptr(opt.exp_avg_sq), m.flat.numel(), _lib.ptr(self._stats),
            _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(), _lib.ptr(self._clip_ws),
            self._clip_ws.numel() * 8, _lib.stream_ptr(dev)))

    def train_an_epoch(self, train_loader, epoch_id):
        """cmn.py:202-267.  A loader with ``cmn_train_loader`` is asked for ``cmn_train_loader(batch_size, True,
        neg_count)`` exactly as the reference asks; its batches (or those of any other iterable of such 5-tuples) go
        through the padded form one after the other with ONE host sync at the end.  A ``data.DeviceTensorBatcher`` over
        ``(users, pos, neg)`` is run resident: one device-side permutation, the whole epoch enqueued from C on the
        item -> users CSR.  Prints the LAST batch's loss and logs the epoch sum."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        self._setup()
        dev = self.model.flat.device
        if isinstance(train_loader, DeviceTensorBatcher) and len(train_loader.tensors) == 3:
            if train_loader.batch_size != int(self.batch_size):
                raise ValueError("the batcher's batch size differs from config['batch_size']")
            perm = train_loader.permutation()
            cols = [t.to(dev) if perm is None else t.to(dev)[perm] for t in train_loader.tensors]
            if cols[0].numel() == 0:
                raise ValueError("empty epoch")
            self.enqueue_epoch(*cols)
            st = self._sync_stats()
        else:
            if hasattr(train_loader, "cmn_train_loader"):
                train_loader = train_loader.cmn_train_loader(self.batch_size, True, self.config["neg_count"])
            st = self._run_epoch(train_loader)
        print("[Training Epoch {}], Loss {}".format(epoch_id, st.loss))
        self.writer.add_scalar("model/loss", st.loss_sum, epoch_id)

    def bpr_loss(self, pos_score, neg_score):
        """cmn.py:269-275 on caller-supplied score tensors (utility, not the fused path): eps inside the log."""
        return torch.mean(-1 * torch.log(torch.sigmoid(pos_score - neg_score) + 1e-12))
