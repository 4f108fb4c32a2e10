"""Drop-in ``NARM`` / ``NARMEngine`` for beta_rec/models/narm.py on libhiprec.so.

Interface parity (file:line = beta_rec/models/narm.py): ``NARM(config)`` :17-94 (``forward(seq, lengths)``),
``NARMEngine(config)`` :97-217 (``train_an_epoch(train_loader, epoch) -> mean loss``, ``predict``, ``recommend``, the two
static list helpers).  Same config keys (``config["dataset"]["n_items"]``; ``hidden_size n_layers embedding_dim
dropout_input dropout_hidden batch_size lr_dc_step lr_dc`` under ``config["model"]``), same ``state_dict`` keys and
shapes, and the same constructed weights for the same torch seed: the constructor builds the reference's torch modules
in the reference's order and copies them into the flat buffer.

Kept from the reference on purpose:
* ``n_items`` already counts the padding id 0: the table is ``[n_items, D]``, item 0 scores exactly 0 and sits in the
  softmax's denominator; row 0 of ``emb`` receives a zero gradient through the lookup AND through the scoring path;
* the attention mask is ``seq > 0``, taken from the ids and not from the lengths: a 0 inside a session's length switches
  ``q2`` off at that position while the GRU still steps there (on its biases alone);
* ``alpha = v_t . sigmoid(q1 + mask * q2)`` goes into the weighted sum as it is: there is NO softmax over the positions;
* two dropouts with two rates (the embedded input, ``[c_local, h_T]``), none between stacked GRU layers;
* ``StepLR(step_size=lr_dc_step, gamma=lr_dc)`` driven as ``scheduler.step(epoch=epoch)`` at the top of
  ``train_an_epoch``: epoch ``e`` runs at ``lr * lr_dc ** (e // lr_dc_step)``.

Beyond the reference: ``lens`` may come in any order (the kernels never rely on ``collate_fn``'s sort);
``recommend_next`` ranks the whole catalogue for many profiles in one call through ``csrc/topk.hip``.

Dropout follows the house convention: ``config["model"]["dropout_rng"]`` is ``"torch_cpu"`` (default: the reference's two
masks in its call order and on its shapes, ``[T, B, D]`` then ``[B, 2H]``, so the same torch seed reproduces them) or
``"device"`` (``hiprec_edge_dropout_mask`` seeded by ``dropout_seed`` and the step count); explicit
``keep_masks=[input, hidden]`` are accepted too.  A mask whose rate is 0, and every mask in eval mode, is neither drawn
nor read.  ``_SeqEngine``'s mask plumbing is not reused: it knows one rate and per-block masks.

Forward, loss and backward run in ``csrc/narm.hip`` (the embed through ``csrc/seqrec.hip``, everything GEMM-shaped
through the grouped GEMM of ``csrc/ncf.hip``), the optimizer is the shared dense sweep.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor

MAX_HIDDEN, MAX_DIM, MAX_LAYERS = 128, 128, 4


class _GruParams(nn.Module):
    """``nn.GRU``'s parameters under its names, as views of the flat buffer."""

    def __init__(self, views, n_layers):
        super().__init__()
        for l in range(n_layers):
            for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                setattr(self, f"{n}_l{l}", Parameter(views[f"gru.{n}_l{l}"], requires_grad=False))


def _spec(n_items, D, H, L):
    spec = [("emb.weight", (n_items, D))]
    for l in range(L):
        spec += [(f"gru.weight_ih_l{l}", (3 * H, D if l == 0 else H)), (f"gru.weight_hh_l{l}", (3 * H, H)),
                 (f"gru.bias_ih_l{l}", (3 * H,)), (f"gru.bias_hh_l{l}", (3 * H,))]
    return spec + [("a_1.weight", (H, H)), ("a_2.weight", (H, H)), ("v_t.weight", (1, H)), ("b.weight", (2 * H, D))]


def _session_batch(seq, lens, device):
    """``seq [T, B]`` time-major and ``lens [B]`` checked against each other: ``(seq_t, lens_t, B, T)`` on the device.
    Raises ValueError where the reference cannot run (``pack_padded_sequence`` / ``pad_packed_sequence``)."""
    shape = tuple(seq.shape) if torch.is_tensor(seq) else np.asarray(seq).shape
    if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
        raise ValueError("seq must be [length >= 1, batch >= 1] (time-major, as collate_fn makes it)")
    T, B = int(shape[0]), int(shape[1])
    lens_h = np.asarray(lens.cpu() if torch.is_tensor(lens) else lens, dtype=np.int64).reshape(-1)
    if lens_h.size != B:
        raise ValueError(f"{lens_h.size} lengths for a batch of {B} sessions")
    if int(lens_h.min()) < 1:
        raise ValueError("every session needs a length >= 1")
    if int(lens_h.max()) != T:
        raise ValueError(f"the longest session ({int(lens_h.max())}) must fill the padded length {T}")
    return index_tensor(seq, device), torch.from_numpy(lens_h).to(device), B, T


class NARM(_FlatModel):
    """models/narm.py:17-94.  Flat buffer in ``state_dict()`` order (``_spec``)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.n_items = int(config["dataset"]["n_items"])
        m = config["model"]
        self.hidden_size = int(m["hidden_size"])
        self.batch_size = m["batch_size"]
        self.n_layers = int(m["n_layers"])
        self.dropout_input = float(m["dropout_input"])
        self.dropout_hidden = float(m["dropout_hidden"])
        self.embedding_dim = int(m["embedding_dim"])
        I, D, H, L = self.n_items, self.embedding_dim, self.hidden_size, self.n_layers
        if I < 2:
            raise ValueError("NARM needs n_items >= 2 (the padding id 0 is counted)")
        if not 1 <= H <= MAX_HIDDEN:
            raise ValueError(f"hidden_size must be in 1..{MAX_HIDDEN}, got {H}")
        if not 1 <= D <= MAX_DIM:
            raise ValueError(f"embedding_dim must be in 1..{MAX_DIM}, got {D}")
        if not 1 <= L <= MAX_LAYERS:
            raise ValueError(f"n_layers must be in 1..{MAX_LAYERS}, got {L}")
        for p in (self.dropout_input, self.dropout_hidden):
            if not 0.0 <= p < 1.0:
                raise ValueError("dropout_input and dropout_hidden must be in [0, 1)")
        self.shape = _lib.NarmShape(I, D, H, L, 0)
        v = self._build(_spec(I, D, H, L))
        # the reference's constructor, module by module, for its RNG order (narm.py:39-46); nn.Dropout draws nothing
        emb = nn.Embedding(I, D, padding_idx=0)
        gru = nn.GRU(D, H, L)
        mods = {"emb": emb, "gru": gru, "a_1": nn.Linear(H, H, bias=False), "a_2": nn.Linear(H, H, bias=False),
                "v_t": nn.Linear(H, 1, bias=False), "b": nn.Linear(D, 2 * H, bias=False)}
        for name, view in v.items():
            mod, attr = name.split(".")
            view.copy_(getattr(mods[mod], attr).data)
        self.emb = _ParamView(v["emb.weight"])
        self.gru = _GruParams(v, L)
        self.a_1 = _ParamView(v["a_1.weight"])
        self.a_2 = _ParamView(v["a_2.weight"])
        self.v_t = _ParamView(v["v_t.weight"])
        self.b = _ParamView(v["b.weight"])
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, seq_len):
        need = lib.hiprec_narm_workspace_bytes(ctypes.byref(self.shape), int(batch), int(seq_len))
        if need == 0:
            raise ValueError(f"unsupported batch {batch} x session length {seq_len}")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def query(self, seq, lengths):
        """The eval-mode forward up to ``c_t b.weight``: ``[B, D]`` with ``scores = query emb.weight^T``."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, lens_t, B, T = _session_batch(seq, lengths, dev)
        stats = self._device_stats()
        out = torch.empty((B, self.embedding_dim), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, T)
        _lib.check(lib.hiprec_narm_grad(
            ctypes.byref(self.shape), _lib.ptr(self._flat), None, _lib.ptr(seq_t), _lib.ptr(lens_t), None, B, T, None,
            1.0, 1.0, _lib.ptr(out), _lib.ptr(stats), None, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return out

    # ---- reference API -----------------------------------------------------------------------------------------
    def forward(self, seq, lengths):
        """narm.py:50-88 in eval mode (no dropout), without autograd: ``[B, n_items]`` scores on the device, the query
        against the whole table through the exact-fp32 MFMA GEMM."""
        q = self.query(seq, lengths)
        lib, dev = _lib.load(), self._flat.device
        B, I, D = q.shape[0], self.n_items, self.embedding_dim
        scores = torch.empty((B, I), dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_gemm_f32(0, B, I, D, _lib.ptr(q), D, _lib.ptr(self.emb.weight.data), D, _lib.ptr(scores), I,
                                       None, 0, None, 0, _lib.stream_ptr(dev)))
        return scores


class NARMEngine(FlatModelEngine):
    """models/narm.py:97-217."""

    def __init__(self, config):
        self.config = config
        self.model = NARM(config)
        self._dropout_step = 0
        self.last_keep_masks = None
        super(NARMEngine, self).__init__(config)
        self._base_lr = float(config["model"]["lr"])
        self._lr_dc_step = int(config["model"]["lr_dc_step"])
        self._lr_dc = float(config["model"]["lr_dc"])
        self._n_batches = 0

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_narm_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat NARM buffer is not laid out as libhiprec.so expects; rebuild the library")

    # ---- dropout ---------------------------------------------------------------------------------------------
    def _mask_shapes(self, B, T):
        m = self.model
        return [(T, B, m.embedding_dim), (B, 2 * m.hidden_size)]

    def _keep_masks(self, B, T, keep_masks):
        """``[input, hidden]`` keep masks of one step as uint8 device tensors (None where the rate is 0), or None."""
        m = self.model
        rates = (m.dropout_input, m.dropout_hidden)
        if not m.training or not any(rates):
            return None
        dev = m.flat.device
        shapes = self._mask_shapes(B, T)
        out = [None, None]
        if keep_masks is not None:
            if len(keep_masks) != 2:
                raise ValueError(f"2 keep masks expected (input [T, B, D], hidden [B, 2H]), got {len(keep_masks)}")
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
        rng = cfg["dropout_rng"] if "dropout_rng" in cfg else "torch_cpu"
        self._dropout_step += 1
        if rng == "torch_cpu":
            # nn.Dropout on the CPU draws torch.empty_like(input).bernoulli_(1 - p) on the reference's shapes, in its
            # call order; a rate of 0 draws nothing
            for i, s in enumerate(shapes):
                if rates[i]:
                    out[i] = torch.empty(s).bernoulli_(1 - rates[i]).to(torch.uint8).reshape(-1).contiguous().to(dev)
        elif rng == "device":
            seed = int(cfg["dropout_seed"]) if "dropout_seed" in cfg else 0
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
        if len(batch_data) != 3:
            raise ValueError("a NARM batch is (seq [T, B], target [B], lens)")
        seq, target, lens = batch_data
        seq_t, lens_t, B, T = _session_batch(seq, lens, dev)
        target_t = index_tensor(target, dev)
        if target_t.numel() != B:
            raise ValueError(f"{target_t.numel()} targets for a batch of {B} sessions")
        keep = self.last_keep_masks = self._keep_masks(B, T, keep_masks)
        keep_arr = None
        if keep is not None:
            keep_arr = (ctypes.c_void_p * 2)(*[None if k is None else k.data_ptr() for k in keep])
        ws = m.workspace(lib, B, T)
        _lib.check(lib.hiprec_narm_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), _lib.ptr(lens_t),
            _lib.ptr(target_t), B, T, keep_arr, 1.0 / (1.0 - m.dropout_input), 1.0 / (1.0 - m.dropout_hidden), None,
            _lib.ptr(self._stats), _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)))

    def backward_only(self, batch_data, keep_masks=None):
        """zero_grad + forward + loss + backward without the optimizer step: ``(loss, grads)``."""
        self._enqueue_grad(batch_data, keep_masks)
        st, grads = self._finish_backward_only()
        return st.loss, grads

    def train_single_batch(self, batch_data, ratings=None, keep_masks=None):
        """One iteration of the reference's epoch loop (narm.py:129-142) on ``(seq, target, lens)``: the loss."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_grad(batch_data, keep_masks)
        self._enqueue_opt()
        return self._sync_stats().loss

    def _epoch_step(self, batch):
        self._n_batches += 1
        self._enqueue_step(batch)

    def epoch_lr(self, epoch):
        """``StepLR(step_size=lr_dc_step, gamma=lr_dc)`` after ``scheduler.step(epoch=epoch)``."""
        return self._base_lr * self._lr_dc ** (int(epoch) // self._lr_dc_step)

    def train_an_epoch(self, train_loader, epoch):
        """narm.py:113-152: the epoch at ``lr * lr_dc ** (epoch // lr_dc_step)``, every step enqueued back to back with
        ONE host sync at the end; returns the mean of the per-batch losses and writes it to the writer."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        print("Start Epoch #", epoch)
        self.optimizer.lr = self.epoch_lr(epoch)
        self._n_batches = 0
        st = self._run_epoch(train_loader)
        mean_loss = st.loss_sum / max(self._n_batches, 1)
        print("Epoch: {}, train loss: {:.4f}".format(epoch, mean_loss))
        self.writer.add_scalar("model/loss", mean_loss, epoch)
        return mean_loss

    # ---- inference ---------------------------------------------------------------------------------------------
    def predict(self, user_profile, batch=1):
        """narm.py:154-185: eval mode, the softmax over all ``n_items`` of one profile's scores as a numpy ``[I]``."""
        self.model.eval()
        seq = np.asarray(user_profile, dtype=np.int64).reshape(-1, 1)
        scores = self.model.forward(seq, [seq.shape[0]])
        return torch.softmax(scores, dim=1).cpu().numpy()[0]

    def recommend(self, user_profile, user_id=None):
        """narm.py:187-207: ``[([index], score), ...]`` over all items, sorted by score descending."""
        pred = self.predict(user_profile, batch=1)
        order = np.argsort(-pred, kind="stable")
        return [([int(i)], float(pred[i])) for i in order]

    @staticmethod
    def get_recommendation_list(recommendation):
        return list(map(lambda x: x[0], recommendation))

    @staticmethod
    def get_recommendation_confidence_list(recommendation):
        return list(map(lambda x: x[1], recommendation))

    def recommend_next(self, profiles, k, seen=None):
        """The ``k`` best next items for every profile, the whole catalogue ranked in one call: ``query`` against
        ``emb.weight[1:]`` through ``recommend.topk_factors``; ids are shifted back by one, so the padding id is never
        returned.  ``profiles``: a ragged list of id lists, or a ``(padded [n, T] array, lengths)`` pair.  ``seen``:
        None, or a ``(rows, items)`` pair of equally long id columns -- profile ``r`` is never recommended item ``i``
        (ids as the model knows them; 0 entries are ignored).  The kernel batch is sorted by length; the results come
        back in the caller's order: ``(items [n, k] int64, scores [n, k] fp32)`` on the device, ``-1`` / ``-inf`` in a
        tail with nothing left."""
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
            flat = np.concatenate([np.asarray(p, dtype=np.int64) for p in profiles])
            padded[np.arange(padded.shape[1])[None, :] < lens[:, None]] = flat
        n = lens.size
        if n < 1 or int(lens.min()) < 1 or int(lens.max()) > padded.shape[1]:
            raise ValueError("lengths must be in 1 .. the padded width")
        order = np.argsort(-lens, kind="stable")
        T = int(lens.max())
        seq = np.ascontiguousarray(padded[order, :T].T)
        q_sorted = self.model.query(seq, lens[order])
        dev = q_sorted.device
        q = torch.empty_like(q_sorted)
        q[torch.from_numpy(order).to(dev)] = q_sorted
        table = self.model.emb.weight.data[1:]
        if seen is not None:
            rows, items = (index_tensor(x, dev) for x in seen)
            if rows.numel() != items.numel():
                raise ValueError("seen must be a (rows, items) pair of equally long id columns")
            keep = items != 0
            seen = (rows[keep], items[keep] - 1)
        items, scores = topk_factors(q, table, 1.0, None, torch.arange(n, device=dev), k, seen)
        return torch.where(items >= 0, items + 1, items), scores
