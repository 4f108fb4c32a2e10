"""``GRU4Rec`` / ``GRU4RecEngine``: the session-parallel GRU recommender (Hidasi et al., "Session-based Recommendations
with Recurrent Neural Networks", ICLR 2016; Hidasi and Karatzoglou, "Recurrent Neural Networks with Top-k Gains for
Session-based Recommendations", CIKM 2018) on libhiprec.so.

There is no counterpart in the reference; the papers and ``tests/gru4rec_torch.py`` (a restatement in plain torch ops)
are the specification, ``include/hiprec.h`` states the contract:

* items are ``0 .. n_items - 1`` and no id is special;
* ``batch_size`` slots each walk one session, one event per step.  The hidden state of every layer is carried from step
  to step as a constant (no back-propagation through time); a slot whose ``reset`` byte is set starts from zero;
* the input row is ``Wy[item]`` (``constrained_embedding``, the default: input and output share the table, so
  ``in_0 = layers[-1]``) or ``E[item]`` of width ``embedding``;
* a row is scored against the other rows' targets plus ``n_sample`` extra sampled items, never against the catalogue:
  ``R[i, j] = <h_last[i], Wy[cand[j]]> + By[cand[j]]`` with ``cand = [targets | samples]``;
* ``loss``: ``"cross-entropy"`` (sampled softmax, logQ shift ``logq * log p``) or ``"bpr-max"`` (with ``bpreg`` and
  ``elu_param``); both are sums over the batch.

Config keys under ``config["model"]``: ``layers constrained_embedding embedding loss bpreg elu_param logq n_sample
sample_alpha dropout_p_embed dropout_p_hidden batch_size optimizer lr``; ``n_items`` is ``config["dataset"]["n_items"]``.
Dropout follows the house convention: ``dropout_rng`` is ``"torch_cpu"`` (default: ``torch.empty(shape).bernoulli_(1 - p)``
for the input rows ``[B, in_0]`` and then every layer's output ``[B, H_l]``, so the torch seed reproduces them) or
``"device"`` (``hiprec_edge_dropout_mask`` seeded by ``dropout_seed`` and the step count); explicit
``keep_masks=[embed, hidden_0, ...]`` are accepted too.  A rate of 0, and eval mode, draws nothing.

Not built: the one-hot input form, the TOP1 and plain BPR losses, Adagrad with momentum (the optimizer is
the shared dense sweep: ``sgd``, ``adam``, ``rmsprop``) and back-propagation through time.

Forward, loss and backward run in ``csrc/gru4rec.hip`` (everything GEMM-shaped through the grouped GEMM of
``csrc/ncf.hip``), ``recommend_next`` ranks the catalogue through ``csrc/topk.hip``.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor

MAX_LAYERS, MAX_HIDDEN, MAX_DIM, MAX_BATCH, MAX_SAMPLE = 3, 128, 128, 2048, 4096      # kGru4recMax*
LOSSES = ("bpr-max", "cross-entropy")      # HIPREC_GRU4REC_*


def _get(cfg, key, default):
    return cfg[key] if key in cfg else default


def _spec(n_items, layers, D):
    """``state_dict()`` names and shapes; ``D == 0``: constrained (no ``E``)."""
    spec = [("Wy.weight", (n_items, layers[-1])), ("By.weight", (n_items, 1))]
    if D:
        spec.append(("E.weight", (n_items, D)))
    for i, H in enumerate(layers):
        fan_in = layers[i - 1] if i else (D or layers[-1])
        spec += [(f"G.{i}.weight_ih", (3 * H, fan_in)), (f"G.{i}.weight_hh", (3 * H, H)), (f"G.{i}.bias_ih", (3 * H,)),
                 (f"G.{i}.bias_hh", (3 * H,))]
    return spec


class _CellParams(nn.Module):
    """``nn.GRUCell``'s parameters under its names, as views of the flat buffer."""

    def __init__(self, views, i):
        super().__init__()
        for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            setattr(self, n, nn.Parameter(views[f"G.{i}.{n}"], requires_grad=False))


def _glorot_(view):
    fan_out, fan_in = view.shape
    bound = float(np.sqrt(6.0 / (fan_in + fan_out)))
    view.uniform_(-bound, bound)


class GRU4Rec(_FlatModel):
    """The model: flat buffer in ``state_dict()`` order (``_spec``) plus the carried state ``h_l [B, H_l]`` per layer."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        m = config["model"]
        self.n_items = int(config["dataset"]["n_items"])
        self.layers = [int(h) for h in m["layers"]]
        self.constrained = bool(_get(m, "constrained_embedding", True))
        self.loss = m["loss"]
        self.bpreg, self.elu_param, self.logq = (float(_get(m, k, 0.0)) for k in ("bpreg", "elu_param", "logq"))
        self.n_sample = int(_get(m, "n_sample", 0))
        self.sample_alpha = float(_get(m, "sample_alpha", 1.0))
        self.dropout_p_embed = float(_get(m, "dropout_p_embed", 0.0))
        self.dropout_p_hidden = float(_get(m, "dropout_p_hidden", 0.0))
        self.batch_size = int(m["batch_size"])
        if self.n_items < 1:
            raise ValueError("GRU4Rec needs n_items >= 1")
        if not 1 <= len(self.layers) <= MAX_LAYERS:
            raise ValueError(f"layers must hold 1..{MAX_LAYERS} hidden sizes, got {self.layers}")
        for h in self.layers:
            if not 1 <= h <= MAX_HIDDEN:
                raise ValueError(f"every entry of layers must be in 1..{MAX_HIDDEN}, got {h}")
        self.embedding = 0
        if not self.constrained:
            self.embedding = int(m["embedding"])
            if not 1 <= self.embedding <= MAX_DIM:
                raise ValueError(f"embedding must be in 1..{MAX_DIM}, got {self.embedding}")
        if self.loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}, got {self.loss!r}")
        if self.bpreg < 0.0 or self.elu_param < 0.0:
            raise ValueError("bpreg and elu_param must be >= 0")
        if not 0 <= self.n_sample <= MAX_SAMPLE:
            raise ValueError(f"n_sample must be in 0..{MAX_SAMPLE}, got {self.n_sample}")
        if not 1 <= self.batch_size <= MAX_BATCH:
            raise ValueError(f"batch_size must be in 1..{MAX_BATCH}, got {self.batch_size}")
        for p in (self.dropout_p_embed, self.dropout_p_hidden):
            if not 0.0 <= p < 1.0:
                raise ValueError("dropout_p_embed and dropout_p_hidden must be in [0, 1)")
        L = len(self.layers)
        self.in_width = self.embedding or self.layers[-1]
        self.shape = _lib.Gru4recShape(self.n_items, L, (ctypes.c_int32 * 3)(*(self.layers + [0] * (3 - L))),
                                       self.embedding, LOSSES.index(self.loss))
        v = self._build(_spec(self.n_items, self.layers, self.embedding))
        # drawn in state_dict() order from torch's global generator: one seed gives one model.  Glorot-uniform per
        # [H, in] gate block and for the tables; the biases and By stay zero
        with torch.no_grad():
            for name, view in v.items():
                if name in ("Wy.weight", "E.weight"):
                    _glorot_(view)
                elif name.endswith(("weight_ih", "weight_hh")):
                    for gate in view.chunk(3, 0):
                        _glorot_(gate)
        self.Wy = _ParamView(v["Wy.weight"])
        self.By = _ParamView(v["By.weight"])
        if self.embedding:
            self.E = _ParamView(v["E.weight"])
        self.G = nn.ModuleList(_CellParams(v, i) for i in range(L))
        self._ws = None
        self._states = None

    # ---- the carried state -------------------------------------------------------------------------------------
    def reset_state(self, batch):
        """Zero state for ``batch`` slots on the parameters' device."""
        batch = int(batch)
        if not 1 <= batch <= MAX_BATCH:
            raise ValueError(f"a step holds 1..{MAX_BATCH} slots, got {batch}")
        self._states = [torch.zeros((batch, h), dtype=torch.float32, device=self._flat.device) for h in self.layers]
        return self._states

    @property
    def state(self):
        """The per-layer state tensors ``[B, H_l]`` (None before the first step)."""
        return self._states

    def _state_for(self, batch):
        if self._states is None or self._states[0].device != self._flat.device:
            self.reset_state(batch)
        if self._states[0].shape[0] != batch:
            raise ValueError(f"the carried state holds {self._states[0].shape[0]} slots, the step {batch}: "
                             "call reset_state(batch) first")
        return (ctypes.c_void_p * len(self.layers))(*[s.data_ptr() for s in self._states])

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, n_sample):
        need = lib.hiprec_gru4rec_workspace_bytes(ctypes.byref(self.shape), int(batch), int(n_sample))
        if need == 0:
            raise ValueError(f"unsupported step of {batch} slots and {n_sample} samples (at most {MAX_BATCH} and "
                             f"{MAX_SAMPLE})")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def _slots(self, in_items, reset):
        dev = self._flat.device
        in_t = index_tensor(in_items, dev)
        B = int(in_t.numel())
        if not 1 <= B <= MAX_BATCH:
            raise ValueError(f"a step holds 1..{MAX_BATCH} slots, got {B}")
        reset_t = None
        if reset is not None:
            reset_t = reset if torch.is_tensor(reset) else torch.as_tensor(np.asarray(reset))
            if reset_t.dtype != torch.uint8:      # the loader's device slices pass through as they are
                reset_t = (reset_t != 0).to(torch.uint8)
            reset_t = reset_t.to(dev).reshape(-1).contiguous()
            if reset_t.numel() != B:
                raise ValueError(f"{reset_t.numel()} reset bytes for {B} slots")
        return in_t, reset_t, B

    def step(self, in_items, reset=None):
        """The eval step (no dropout, no loss): the state advances by one event per slot; returns ``h_last [B, H]``."""
        lib = self._require_hip()
        dev = self._flat.device
        in_t, reset_t, B = self._slots(in_items, reset)
        state = self._state_for(B)
        stats = self._device_stats()
        out = torch.empty((B, self.layers[-1]), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, 0)
        _lib.check(lib.hiprec_gru4rec_grad(
            ctypes.byref(self.shape), _lib.ptr(self._flat), None, state, _lib.ptr(in_t), None,
            None if reset_t is None else _lib.ptr(reset_t), None, B, 0, None, 0.0, 1.0, 0.0, 0.0, None, 1.0, 1.0,
            _lib.ptr(out), _lib.ptr(stats), None, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def scores(self, h):
        """``h Wy^T + By``: ``[B, n_items]`` through the exact-fp32 MFMA GEMM."""
        lib, dev = _lib.load(), self._flat.device
        B, I, H = h.shape[0], self.n_items, self.layers[-1]
        out = torch.empty((B, I), dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_gemm_f32(0, B, I, H, _lib.ptr(h), H, _lib.ptr(self.Wy.weight.data), H, _lib.ptr(out), I,
                                       _lib.ptr(self.By.weight.data), 0, None, 0, _lib.stream_ptr(dev)))
        return out

    def forward(self, in_items, reset=None):
        """The eval step and the scores of every item after it: ``[B, n_items]`` on the device."""
        return self.scores(self.step(in_items, reset))

    def item_factors(self):
        """``(Wy [n_items, H], By [n_items])``: views of the flat buffer."""
        return self.Wy.weight.data, self.By.weight.data[:, 0]

    def walk(self, padded, lens):
        """``h_last`` after each profile's last event: ``padded [n, T]`` ids (anything valid behind a profile's length),
        ``lens [n]``; every profile starts from zero and is frozen once it has ended.  The carried training state is
        left as it was.  ``[n, H]`` on the device."""
        dev = self._flat.device
        padded = np.asarray(padded, dtype=np.int64)
        lens = np.asarray(lens, dtype=np.int64).reshape(-1)
        n = lens.size
        if n < 1 or padded.ndim != 2 or padded.shape[0] != n or int(lens.min()) < 1 or int(lens.max()) > padded.shape[1]:
            raise ValueError("every profile needs a length in 1 .. the padded width")
        out = torch.empty((n, self.layers[-1]), dtype=torch.float32, device=dev)
        kept = self._states
        try:
            for r0 in range(0, n, MAX_BATCH):
                r1 = min(n, r0 + MAX_BATCH)
                T = int(lens[r0:r1].max())
                ids = torch.from_numpy(np.ascontiguousarray(padded[r0:r1, :T].T)).to(dev)
                ln = torch.from_numpy(lens[r0:r1]).to(dev)
                self.reset_state(r1 - r0)
                h_end = out[r0:r1]
                for t in range(T):
                    live = (ln > t)[:, None]
                    before = [s.clone() for s in self._states]
                    h = self.step(ids[t])
                    for s, b in zip(self._states, before):
                        s.copy_(torch.where(live, s, b))
                    h_end.copy_(h if t == 0 else torch.where(live, h, h_end))
        finally:
            self._states = kept
        return out


class GRU4RecEngine(FlatModelEngine):
    """Training and inference around ``GRU4Rec``."""

    def __init__(self, config):
        self.config = config
        self.model = GRU4Rec(config)
        self._dropout_step = 0
        self.last_keep_masks = None
        self._log_p = None
        super(GRU4RecEngine, self).__init__(config)
        self._n_batches = 0

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_gru4rec_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat GRU4Rec buffer is not laid out as libhiprec.so expects; rebuild the library")

    def set_item_probs(self, probs):
        """``probs [n_items]``: every item's share of the training events (``SessionParallelLoader.item_probs``), which
        the logQ shift of the cross-entropy loss reads.  An item without support has no finite shift: it must not be a
        candidate."""
        p = torch.as_tensor(np.asarray(probs, dtype=np.float64)).reshape(-1)
        if p.numel() != self.model.n_items:
            raise ValueError(f"{p.numel()} item probabilities for {self.model.n_items} items")
        if float(p.min()) < 0.0:
            raise ValueError("item probabilities must be >= 0")
        self._log_p = torch.log(p).to(torch.float32).to(self.model.flat.device)

    # ---- dropout ---------------------------------------------------------------------------------------------
    def _mask_shapes(self, B):
        m = self.model
        return [(B, m.in_width)] + [(B, h) for h in m.layers]

    def _keep_masks(self, B, keep_masks):
        """``[embed, hidden_0, ...]`` keep masks of one step as uint8 device tensors (None where the rate is 0), or
        None."""
        m = self.model
        shapes = self._mask_shapes(B)
        rates = [m.dropout_p_embed] + [m.dropout_p_hidden] * len(m.layers)
        if not m.training or not any(rates):
            return None
        dev = m.flat.device
        out = [None] * len(shapes)
        if keep_masks is not None:
            if len(keep_masks) != len(shapes):
                raise ValueError(f"{len(shapes)} keep masks expected (embed [B, in_0], then [B, H_l] per layer), got "
                                 f"{len(keep_masks)}")
            for i, (k, s) in enumerate(zip(keep_masks, shapes)):
                if rates[i] == 0.0:
                    continue
                if k is None:
                    raise ValueError(f"keep mask {i} is missing although its dropout rate is {rates[i]}")
                t = torch.as_tensor(np.asarray(k.cpu() if torch.is_tensor(k) else k)).to(torch.uint8)
                if t.numel() != int(np.prod(s)):
                    raise ValueError(f"keep mask of {t.numel()} elements where {s} is expected")
                out[i] = t.reshape(-1).contiguous().to(dev)
            return out
        cfg = self.config["model"]
        rng = _get(cfg, "dropout_rng", "torch_cpu")
        self._dropout_step += 1
        if rng == "torch_cpu":
            for i, s in enumerate(shapes):
                if rates[i]:
                    out[i] = torch.empty(s).bernoulli_(1 - rates[i]).to(torch.uint8).reshape(-1).contiguous().to(dev)
        elif rng == "device":
            seed = int(_get(cfg, "dropout_seed", 0))
            lib = _lib.load()
            for i, s in enumerate(shapes):
                if rates[i]:
                    buf = torch.empty(int(np.prod(s)), dtype=torch.uint8, device=dev)
                    _lib.check(lib.hiprec_edge_dropout_mask(_lib.ptr(buf), buf.numel(), 1.0 - rates[i], seed * 64 + i,
                                                            self._dropout_step, _lib.stream_ptr(dev)))
                    out[i] = buf
        else:
            raise ValueError(f"unknown dropout_rng {rng!r}: 'torch_cpu' or 'device'")
        return out

    # ---- the step ----------------------------------------------------------------------------------------------
    def _enqueue_grad(self, batch_data, keep_masks=None):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 4:
            raise ValueError("a GRU4Rec step is (in_items [B], targets [B], reset [B], samples [S])")
        in_items, targets, reset, samples = batch_data
        in_t, reset_t, B = m._slots(in_items, reset)
        tgt_t = index_tensor(targets, dev)
        if tgt_t.numel() != B:
            raise ValueError(f"{tgt_t.numel()} targets for {B} slots")
        smp_t = index_tensor(samples, dev) if samples is not None else torch.empty(0, dtype=torch.int64, device=dev)
        S = int(smp_t.numel())
        if S > MAX_SAMPLE:
            raise ValueError(f"a step takes at most {MAX_SAMPLE} samples, got {S}")
        if B + S < 2:
            raise ValueError("a row needs a negative: batch + samples must be >= 2")
        shift = m.loss == "cross-entropy" and m.logq != 0.0
        if shift and self._log_p is None:
            raise ValueError("logq != 0 needs the items' event shares: set_item_probs(loader.item_probs)")
        state = m._state_for(B)
        keep = self.last_keep_masks = self._keep_masks(B, keep_masks)
        keep_arr = None
        if keep is not None:
            keep_arr = (ctypes.c_void_p * len(keep))(*[None if k is None else k.data_ptr() for k in keep])
        ws = m.workspace(lib, B, S)
        _lib.check(lib.hiprec_gru4rec_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), state, _lib.ptr(in_t), _lib.ptr(tgt_t),
            None if reset_t is None else _lib.ptr(reset_t), _lib.ptr(smp_t) if S else None, B, S,
            _lib.ptr(self._log_p) if shift else None, m.logq, m.sample_alpha, m.bpreg, m.elu_param, keep_arr,
            1.0 / (1.0 - m.dropout_p_embed), 1.0 / (1.0 - m.dropout_p_hidden), None, _lib.ptr(self._stats),
            _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))

    def backward_only(self, batch_data, keep_masks=None):
        """zero_grad + forward + loss + backward without the optimizer step (the state advances): ``(loss, grads)``."""
        self._enqueue_grad(batch_data, keep_masks)
        st, grads = self._finish_backward_only()
        return st.loss, grads

    def train_single_batch(self, batch_data, ratings=None, keep_masks=None):
        """One step on ``(in_items, targets, reset, samples)``: the loss (a sum over the slots)."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_grad(batch_data, keep_masks)
        self._enqueue_opt()
        return self._sync_stats().loss

    def _epoch_step(self, batch):
        self._n_batches += 1
        self._enqueue_step(batch)

    def train_an_epoch(self, train_loader, epoch_id):
        """Every step of the loader (``data.SessionParallelLoader``) from a zero state, enqueued back to back with ONE
        host sync at the end; returns the mean of the per-step losses and writes it to the writer."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._setup()
        m = self.model
        if getattr(train_loader, "device", "") is None:
            train_loader.device = m.flat.device
        if hasattr(train_loader, "item_probs") and m.loss == "cross-entropy" and m.logq != 0.0:
            self.set_item_probs(train_loader.item_probs)
        m.reset_state(getattr(train_loader, "batch_size", m.batch_size))
        self._n_batches = 0
        st = self._run_epoch(train_loader)
        mean_loss = st.loss_sum / max(self._n_batches, 1)
        print("[Training Epoch {}], Loss {:.6f}".format(epoch_id, mean_loss))
        self.writer.add_scalar("model/loss", mean_loss, epoch_id)
        return mean_loss

    # ---- inference ---------------------------------------------------------------------------------------------
    def predict(self, profile):
        """Eval-mode scores of every item as the event after ``profile`` (a list of ids): a numpy ``[n_items]``."""
        self.model.eval()
        seq = np.asarray(profile, dtype=np.int64).reshape(1, -1)
        if seq.shape[1] < 1:
            raise ValueError("a profile needs at least one item")
        h = self.model.walk(seq, [seq.shape[1]])
        return self.model.scores(h).cpu().numpy()[0]

    def recommend_next(self, profiles, k, seen=None):
        """The ``k`` best next items for every profile, the whole catalogue ranked in one call: ``max(len)`` eval steps
        with finished profiles frozen, then ``h_last`` against ``Wy`` with ``By`` as the item bias through
        ``recommend.topk_factors``.  ``profiles``: a ragged list of id lists, or a ``(padded [n, T] array, lengths)``
        pair.  ``seen``: None, or a ``(rows, items)`` pair of equally long id columns -- profile ``r`` is never
        recommended item ``i``.  Results come back in the caller's order: ``(items [n, k] int64, scores [n, k] fp32)``
        on the device, ``-1`` / ``-inf`` in a tail with nothing left."""
        from .recommend import topk_factors

        self.model.eval()
        if isinstance(profiles, tuple) and len(profiles) == 2 and np.ndim(profiles[0]) == 2:
            padded = np.array(profiles[0], dtype=np.int64)
            lens = np.asarray(profiles[1], dtype=np.int64).reshape(-1)
            if lens.size != padded.shape[0]:
                raise ValueError("one length per padded profile is needed")
            if lens.size and int(lens.min()) >= 1 and int(lens.max()) <= padded.shape[1]:
                padded[np.arange(padded.shape[1])[None, :] >= lens[:, None]] = 0      # what lies behind a length is not read
        else:
            lens = np.fromiter((len(p) for p in profiles), dtype=np.int64, count=len(profiles))
            if lens.size == 0 or int(lens.min()) < 1:
                raise ValueError("every profile needs at least one item")
            padded = np.zeros((lens.size, int(lens.max())), dtype=np.int64)
            padded[np.arange(padded.shape[1])[None, :] < lens[:, None]] = np.concatenate(
                [np.asarray(p, dtype=np.int64) for p in profiles])
        h = self.model.walk(padded, lens)
        n, dev = h.shape[0], h.device
        table, bias = self.model.item_factors()
        if seen is not None:
            rows, items = (index_tensor(x, dev) for x in seen)
            if rows.numel() != items.numel():
                raise ValueError("seen must be a (rows, items) pair of equally long id columns")
            if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
                raise ValueError(f"seen: a row outside [0, {n})")
            if items.numel() and (int(items.min()) < 0 or int(items.max()) >= self.model.n_items):
                raise ValueError(f"seen: an item outside [0, {self.model.n_items})")
            seen = (rows, items)
        return topk_factors(h, table, 1.0, bias, torch.arange(n, device=dev), k, seen)
