"""``SRGNN`` / ``SRGNNEngine``: the session-graph gated GNN with attention readout (Wu et al., "Session-based
Recommendation with Graph Neural Networks", AAAI 2019) on libhiprec.so.

There is no counterpart in the reference; ``tests/srgnn_torch.py`` (a restatement in plain torch ops with dense
adjacency matrices) is the specification, ``include/hiprec.h`` states the contract:

* ids are ``1 .. n_node - 1``, 0 is the padding id and ``n_node`` counts it (as NARM's ``n_items`` does);
* a batch is NARM's: ``(seq [T, B] int64 time-major zero-padded, target [B], lens)``, so ``data.session_prefixes`` and
  ``data.SessionLoader`` serve it.  Unlike NARM, a 0 inside a session's length is an error;
* the session graph: nodes are a session's distinct ids ascending, the edges the SET of its transitions (a repeated
  transition is one edge, ``s_t == s_{t+1}`` a self-loop that counts), both neighbourhood means feed a GRU-style gate,
  ``step`` times with the same weights;
* the readout ``alpha_t = linear_three . sigmoid(linear_one(h_T) + linear_two(x_t))`` goes into ``s_g`` as it is (no
  softmax over positions); ``a = linear_transform([s_g | h_T])``, or ``s_g`` with ``nonhybrid``;
* scores are ``a . embedding[1:]``: ``n_node - 1`` columns, column ``j`` is item ``j + 1``; the loss is the mean
  cross-entropy against ``target - 1``.

Config keys under ``config["model"]`` (the paper's defaults): ``hidden_size`` 100, ``step`` 1, ``lr`` 1e-3, ``l2`` 1e-5
(Adam's weight decay on every element; the returned loss excludes it), ``lr_dc_step`` 3, ``lr_dc`` 0.1, ``batch_size``
100, ``nonhybrid`` False; ``n_node`` is ``config["dataset"]["n_node"]``.  There is no dropout in this model.

Every element is drawn ``uniform(-1 / sqrt(H), 1 / sqrt(H))``, one ``uniform_`` call per parameter in ``state_dict()``
order on torch's default CPU generator.  Deviations from the published code: its unused ``linear_edge_f``
is left out, and the padding id is no node of the session graph (there it is an isolated node that nothing reads).

Graph build, forward, loss and backward run in ``csrc/srgnn.hip`` (everything GEMM-shaped through the grouped GEMM of
``csrc/ncf.hip``), the optimizer is the shared dense sweep, ``recommend_next`` ranks the catalogue through
``csrc/topk.hip``.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor
from .narm import _session_batch

MAX_HIDDEN, MAX_STEP, MAX_LEN, MAX_BATCH = 128, 4, 256, 1024      # kSrgnnMax*
DEFAULTS = {"hidden_size": 100, "step": 1, "lr": 1e-3, "l2": 1e-5, "lr_dc_step": 3, "lr_dc": 0.1, "batch_size": 100,
            "nonhybrid": False}
GRAPH_FIELDS = ("n_nodes", "node_off", "slot_off", "alias", "nodes", "node_sess", "node_cnt", "in_start", "indeg",
                "out_start", "outdeg", "in_idx", "out_idx")


def _get(cfg, key):
    return cfg[key] if key in cfg else DEFAULTS[key]


def _spec(n_node, H):
    return [("embedding.weight", (n_node, H)), ("gnn.w_ih", (3 * H, 2 * H)), ("gnn.w_hh", (3 * H, H)),
            ("gnn.b_ih", (3 * H,)), ("gnn.b_hh", (3 * H,)), ("gnn.b_iah", (H,)), ("gnn.b_oah", (H,)),
            ("gnn.linear_edge_in.weight", (H, H)), ("gnn.linear_edge_in.bias", (H,)),
            ("gnn.linear_edge_out.weight", (H, H)), ("gnn.linear_edge_out.bias", (H,)),
            ("linear_one.weight", (H, H)), ("linear_one.bias", (H,)), ("linear_two.weight", (H, H)),
            ("linear_two.bias", (H,)), ("linear_three.weight", (1, H)), ("linear_transform.weight", (H, 2 * H)),
            ("linear_transform.bias", (H,))]


class _GnnParams(torch.nn.Module):
    """The gated cell's parameters under the published names, as views of the flat buffer."""

    def __init__(self, v):
        super().__init__()
        for n in ("w_ih", "w_hh", "b_ih", "b_hh", "b_iah", "b_oah"):
            setattr(self, n, torch.nn.Parameter(v[f"gnn.{n}"], requires_grad=False))
        self.linear_edge_in = _ParamView(v["gnn.linear_edge_in.weight"], v["gnn.linear_edge_in.bias"])
        self.linear_edge_out = _ParamView(v["gnn.linear_edge_out.weight"], v["gnn.linear_edge_out.bias"])


def _checked_batch(seq, lens, device):
    """``narm._session_batch`` plus what SR-GNN adds: limits, no padding id inside a length.  Returns
    ``(seq_t, lens_t, B, T, n_rows)`` with ``n_rows = sum(lens)``."""
    seq_t, lens_t, B, T = _session_batch(seq, lens, device)
    if B > MAX_BATCH:
        raise ValueError(f"a step holds at most {MAX_BATCH} sessions, got {B}")
    if T > MAX_LEN:
        raise ValueError(f"a session holds at most {MAX_LEN} items, got {T}")
    seq_h = seq.cpu().numpy() if torch.is_tensor(seq) else np.asarray(seq)
    lens_h = np.asarray(lens.cpu() if torch.is_tensor(lens) else lens, dtype=np.int64).reshape(-1)
    inside = np.arange(T)[:, None] < lens_h[None, :]
    if bool(((seq_h.reshape(T, B) == 0) & inside).any()):
        raise ValueError("the padding id 0 inside a session's length")
    return seq_t, lens_t, B, T, int(lens_h.sum())


class SRGNN(_FlatModel):
    """The model: flat buffer in ``state_dict()`` order (``_spec``)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        m = config["model"]
        self.n_node = int(config["dataset"]["n_node"])
        self.hidden_size = int(_get(m, "hidden_size"))
        self.step = int(_get(m, "step"))
        self.nonhybrid = bool(_get(m, "nonhybrid"))
        self.batch_size = int(_get(m, "batch_size"))
        self.l2 = float(_get(m, "l2"))
        H = self.hidden_size
        if self.n_node < 2:
            raise ValueError("SR-GNN needs n_node >= 2 (the padding id 0 is counted)")
        if not 1 <= H <= MAX_HIDDEN:
            raise ValueError(f"hidden_size must be in 1..{MAX_HIDDEN}, got {H}")
        if not 1 <= self.step <= MAX_STEP:
            raise ValueError(f"step must be in 1..{MAX_STEP}, got {self.step}")
        if not 1 <= self.batch_size <= MAX_BATCH:
            raise ValueError(f"batch_size must be in 1..{MAX_BATCH}, got {self.batch_size}")
        if self.l2 < 0.0:
            raise ValueError("l2 must be >= 0")
        self.shape = _lib.SrgnnShape(self.n_node, H, self.step, int(self.nonhybrid), 0)
        v = self._build(_spec(self.n_node, H))
        stdv = 1.0 / float(np.sqrt(H))
        with torch.no_grad():
            for view in v.values():      # state_dict() order, one draw per parameter
                view.uniform_(-stdv, stdv)
        self.embedding = _ParamView(v["embedding.weight"])
        self.gnn = _GnnParams(v)
        self.linear_one = _ParamView(v["linear_one.weight"], v["linear_one.bias"])
        self.linear_two = _ParamView(v["linear_two.weight"], v["linear_two.bias"])
        self.linear_three = _ParamView(v["linear_three.weight"])
        self.linear_transform = _ParamView(v["linear_transform.weight"], v["linear_transform.bias"])
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, seq_len, n_rows):
        need = lib.hiprec_srgnn_workspace_bytes(ctypes.byref(self.shape), int(batch), int(seq_len), int(n_rows))
        if need == 0:
            raise ValueError(f"unsupported batch {batch} x session length {seq_len} (at most {MAX_BATCH} x {MAX_LEN})")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def graph(self, seq, lengths):
        """The builder's arrays for a batch (``include/hiprec.h`` names and explains them) as a dict of int32 device
        tensors; ``alias`` comes back ``[T, B]``."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, lens_t, B, T, R = _checked_batch(seq, lengths, dev)
        stats = self._device_stats()
        n = lib.hiprec_srgnn_graph_ints(B, T, R)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(lib.hiprec_srgnn_graph(ctypes.byref(self.shape), _lib.ptr(seq_t), _lib.ptr(lens_t), B, T, R,
                                          _lib.ptr(out), out.numel() * 4, _lib.ptr(stats), _lib.stream_ptr(dev)))
        self._check_status()
        sizes = [B, B + 1, B + 1, B * T] + [R] * 9
        parts = dict(zip(GRAPH_FIELDS, torch.split(out, sizes)))
        parts["alias"] = parts["alias"].view(T, B)
        return parts

    def query(self, seq, lengths):
        """The forward up to ``a``: ``[B, H]`` with ``scores = query embedding.weight[1:]^T``."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, lens_t, B, T, R = _checked_batch(seq, lengths, dev)
        stats = self._device_stats()
        out = torch.empty((B, self.hidden_size), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, T, R)
        _lib.check(lib.hiprec_srgnn_grad(
            ctypes.byref(self.shape), _lib.ptr(self._flat), None, _lib.ptr(seq_t), _lib.ptr(lens_t), None, B, T, R, 0.0,
            _lib.ptr(out), _lib.ptr(stats), None, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def forward(self, seq, lengths):
        """``[B, n_node - 1]`` scores on the device (column ``j`` is item ``j + 1``), without autograd: the query against
        ``embedding.weight[1:]`` through the exact-fp32 MFMA GEMM."""
        q = self.query(seq, lengths)
        lib, dev = _lib.load(), self._flat.device
        B, I, H = q.shape[0], self.n_node - 1, self.hidden_size
        scores = torch.empty((B, I), dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_gemm_f32(0, B, I, H, _lib.ptr(q), H, _lib.ptr(self.embedding.weight.data[1:]), H,
                                       _lib.ptr(scores), I, None, 0, None, 0, _lib.stream_ptr(dev)))
        return scores


class SRGNNEngine(FlatModelEngine):
    """Training and inference around ``SRGNN``."""

    def __init__(self, config):
        self.config = config
        self.model = SRGNN(config)
        super(SRGNNEngine, self).__init__(config)
        m = config["model"]
        self._base_lr = float(_get(m, "lr"))
        self._lr_dc_step = int(_get(m, "lr_dc_step"))
        self._lr_dc = float(_get(m, "lr_dc"))
        self._n_batches = 0

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_srgnn_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat SR-GNN buffer is not laid out as libhiprec.so expects; rebuild the library")

    # ---- the step ----------------------------------------------------------------------------------------------
    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 3:
            raise ValueError("an SR-GNN batch is (seq [T, B], target [B], lens)")
        seq, target, lens = batch_data
        seq_t, lens_t, B, T, R = _checked_batch(seq, lens, dev)
        target_h = np.asarray(target.cpu() if torch.is_tensor(target) else target, dtype=np.int64).reshape(-1)
        if target_h.size != B:
            raise ValueError(f"{target_h.size} targets for a batch of {B} sessions")
        if int(target_h.min()) < 1 or int(target_h.max()) >= m.n_node:
            raise ValueError(f"targets must be in 1..{m.n_node - 1}")
        target_t = index_tensor(target, dev)
        ws = m.workspace(lib, B, T, R)
        _lib.check(lib.hiprec_srgnn_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), _lib.ptr(lens_t),
            _lib.ptr(target_t), B, T, R, m.l2, None, _lib.ptr(self._stats), _lib.ptr(self._scratch),
            self._scratch.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))

    def train_single_batch(self, batch_data, ratings=None):
        """One step on ``(seq, target, lens)``: the loss (without the ``l2`` term)."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_grad(batch_data)
        self._enqueue_opt()
        return self._sync_stats().loss

    def _epoch_step(self, batch):
        self._n_batches += 1
        self._enqueue_step(batch)

    def epoch_lr(self, epoch):
        """``StepLR(step_size=lr_dc_step, gamma=lr_dc)``: epoch ``e`` runs at ``lr * lr_dc ** (e // lr_dc_step)``."""
        return self._base_lr * self._lr_dc ** (int(epoch) // self._lr_dc_step)

    def train_an_epoch(self, train_loader, epoch):
        """The epoch at ``epoch_lr(epoch)``, every step enqueued back to back with ONE host sync at the end; returns the
        mean of the per-batch losses and writes it to the writer."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.optimizer.lr = self.epoch_lr(epoch)
        self._n_batches = 0
        st = self._run_epoch(train_loader)
        mean_loss = st.loss_sum / max(self._n_batches, 1)
        print("[Training Epoch {}], Loss {:.6f}".format(epoch, mean_loss))
        self.writer.add_scalar("model/loss", mean_loss, epoch)
        return mean_loss

    # ---- inference ---------------------------------------------------------------------------------------------
    def predict(self, user_profile):
        """The softmax over items ``1 .. n_node - 1`` of one profile's scores as a numpy ``[n_node - 1]`` (entry ``j`` is
        item ``j + 1``)."""
        self.model.eval()
        seq = np.asarray(user_profile, dtype=np.int64).reshape(-1, 1)
        scores = self.model.forward(seq, [seq.shape[0]])
        return torch.softmax(scores, dim=1).cpu().numpy()[0]

    def recommend(self, user_profile, user_id=None):
        """``[([item], score), ...]`` over all items, sorted by score descending."""
        pred = self.predict(user_profile)
        order = np.argsort(-pred, kind="stable")
        return [([int(i) + 1], float(pred[i])) for i in order]

    def recommend_next(self, profiles, k, seen=None):
        """The ``k`` best next items for every profile, the whole catalogue ranked in one call: ``query`` against
        ``embedding.weight[1:]`` through ``recommend.topk_factors``; ids are shifted back by one, so the padding id is
        never returned.  ``profiles``: a ragged list of id lists, or a ``(padded [n, T] array, lengths)`` pair.
        ``seen``: None, or a ``(rows, items)`` pair of equally long id columns -- profile ``r`` is never recommended
        item ``i`` (0 entries are ignored).  Results come back in the caller's order: ``(items [n, k] int64, scores
        [n, k] fp32)`` on the device, ``-1`` / ``-inf`` in a tail with nothing left."""
        from .recommend import topk_factors

        self.model.eval()
        if isinstance(profiles, tuple) and len(profiles) == 2 and np.ndim(profiles[0]) == 2:
            padded = np.asarray(profiles[0], dtype=np.int64)
            lens = np.asarray(profiles[1], dtype=np.int64).reshape(-1)
            if lens.size != padded.shape[0]:
                raise ValueError("one length per padded profile is needed")
        else:
            lens = np.fromiter((len(p) for p in profiles), dtype=np.int64, count=len(profiles))
            if lens.size == 0 or int(lens.min()) < 1:
                raise ValueError("every profile needs at least one item")
            padded = np.zeros((lens.size, int(lens.max())), dtype=np.int64)
            padded[np.arange(padded.shape[1])[None, :] < lens[:, None]] = np.concatenate(
                [np.asarray(p, dtype=np.int64) for p in profiles])
        n = lens.size
        if n < 1 or int(lens.min()) < 1 or int(lens.max()) > padded.shape[1]:
            raise ValueError("lengths must be in 1 .. the padded width")
        H = self.model.hidden_size
        q = torch.empty((n, H), dtype=torch.float32, device=self.model.flat.device)
        for r0 in range(0, n, MAX_BATCH):
            r1 = min(n, r0 + MAX_BATCH)
            T = int(lens[r0:r1].max())
            q[r0:r1] = self.model.query(np.ascontiguousarray(padded[r0:r1, :T].T), lens[r0:r1])
        dev = q.device
        table = self.model.embedding.weight.data[1:]
        if seen is not None:
            rows, items = (index_tensor(x, dev) for x in seen)
            if rows.numel() != items.numel():
                raise ValueError("seen must be a (rows, items) pair of equally long id columns")
            keep = items != 0
            seen = (rows[keep], items[keep] - 1)
        items, scores = topk_factors(q, table, 1.0, None, torch.arange(n, device=dev), k, seen)
        return torch.where(items >= 0, items + 1, items), scores
