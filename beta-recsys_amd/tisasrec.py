"""Drop-in ``TiSASRec`` / ``TiSASRecEngine`` for beta_rec/models/tisasrec.py on libhiprec.so.

Interface parity (file:line = beta_rec/models/tisasrec.py): ``TiSASRec(config)`` :168-360 (``seq2feats``, ``forward``,
``predict``), ``TiSASRecEngine(config)`` :363-424 (``train_single_batch((u, seq, time_seq, time_matrix, pos, neg)) ->
float``, ``train_an_epoch(sampler, epoch_id)``).  Same config keys (``n_users n_items emb_dim maxlen time_span num_blocks
num_heads dropout_rate batch_size l2_emb`` under ``config["model"]``), same ``state_dict`` keys and shapes, and the same
constructed weights for the same torch seed: the constructor builds the reference's torch modules in the reference's
order and copies them into the flat buffer.

Kept from the reference on purpose (beyond what ``sasrec.py`` lists, which holds here too):
* no positional row is added to the sequence; the absolute positions enter as keys and values only, and every
  (query, key) pair adds a row of ``time_matrix_K_emb`` to its key and of ``time_matrix_V_emb`` to its value, selected by
  ``time_matrices[b, i, j]``;
* three separate ``Linear`` layers for Q / K / V and no output projection;
* a padded QUERY row attends uniformly over all positions in the reference; its output reaches nothing (the block's
  output is multiplied by the timeline mask), so the kernel writes zeros there.  Padded KEYS are attended to;
* the four position / time dropout masks are drawn once per step and shared by every block.

The gathered ``[B, T, T, D]`` tensors of the reference are never made (``csrc/tisasrec.hip``).  Their dropout masks are:
``B * T * T * D`` bytes each, 184 MB at the reference's default shape, in every ``dropout_rng`` mode.

``time_matrices`` may be ``None`` wherever a ``time_seq [B, T]`` is given instead: the matrix ``min(|t_i - t_j|,
time_span)`` is then built on the device (``hiprec_time_relation``).

Dropout follows the SASRec convention: ``config["model"]["dropout_rng"]`` is ``"torch_cpu"`` (default: one CPU draw per
mask of the reference's shapes, in its call order) or ``"device"`` (``hiprec_edge_dropout_mask`` seeded by
``dropout_seed`` and the step count); ``train_single_batch(batch, keep_masks=[...])`` takes the ``5 + 3 * num_blocks``
masks explicitly (embedding, abs-pos-K, abs-pos-V ``[B, T, D]``; time-K, time-V ``[B, T, T, D]``; per block attention
``[H * B, T, T]``, dropout1, dropout2 ``[B, T, D]``).  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor
from .sasrec import HEAD_WIDTHS, MAX_DIM, MAX_LEN, _FeedForwardParams

MAX_SPAN = 256
N_FIXED_MASKS = 5


class _TimeAwareAttentionParams(nn.Module):
    """``TimeAwareMultiHeadAttention``'s three ``Linear(D, D)``."""

    def __init__(self, qw, qb, kw, kb, vw, vb):
        super().__init__()
        self.Q_w = _ParamView(qw, qb)
        self.K_w = _ParamView(kw, kb)
        self.V_w = _ParamView(vw, vb)


def _spec(n_items, maxlen, time_span, D, nb):
    spec = [("item_emb.weight", (n_items + 1, D)), ("abs_pos_K_emb.weight", (maxlen, D)),
            ("abs_pos_V_emb.weight", (maxlen, D)), ("time_matrix_K_emb.weight", (time_span + 1, D)),
            ("time_matrix_V_emb.weight", (time_span + 1, D))]
    for b in range(nb):
        spec += [(f"attention_layernorms.{b}.weight", (D,)), (f"attention_layernorms.{b}.bias", (D,))]
    for b in range(nb):
        for m in ("Q_w", "K_w", "V_w"):
            spec += [(f"attention_layers.{b}.{m}.weight", (D, D)), (f"attention_layers.{b}.{m}.bias", (D,))]
    for b in range(nb):
        spec += [(f"forward_layernorms.{b}.weight", (D,)), (f"forward_layernorms.{b}.bias", (D,))]
    for b in range(nb):
        spec += [(f"forward_layers.{b}.conv1.weight", (D, D, 1)), (f"forward_layers.{b}.conv1.bias", (D,)),
                 (f"forward_layers.{b}.conv2.weight", (D, D, 1)), (f"forward_layers.{b}.conv2.bias", (D,))]
    return spec + [("last_layernorm.weight", (D,)), ("last_layernorm.bias", (D,))]


class TiSASRec(_FlatModel):
    """models/tisasrec.py:168-360.  Flat buffer in ``state_dict()`` order (``_spec``)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.user_num = config["n_users"]
        self.item_num = int(config["n_items"])
        self.hidden_units = int(config["emb_dim"])
        self.maxlen = int(config["maxlen"])
        self.time_span = int(config["time_span"])
        self.num_blocks = int(config["num_blocks"])
        self.num_heads = int(config["num_heads"])
        self.dropout_rate = float(config["dropout_rate"])
        self.batch_size = config["batch_size"]
        self.l2_emb = float(config["l2_emb"])
        D, H, T, nb, n_items, span = (self.hidden_units, self.num_heads, self.maxlen, self.num_blocks, self.item_num,
                                      self.time_span)
        if nb < 1 or H < 1 or n_items < 1 or T < 1 or span < 1:
            raise ValueError("TiSASRec needs num_blocks, num_heads, n_items, maxlen and time_span >= 1")
        if D % H != 0 or D // H not in HEAD_WIDTHS:
            raise ValueError(f"the HIP attention supports head widths emb_dim / num_heads in {HEAD_WIDTHS}; "
                             f"got emb_dim {D}, num_heads {H}")
        if D > MAX_DIM:
            raise ValueError(f"emb_dim must be <= {MAX_DIM}, got {D}")
        if T > MAX_LEN:
            raise ValueError(f"maxlen must be <= {MAX_LEN}, got {T}")
        if span > MAX_SPAN:
            raise ValueError(f"time_span must be <= {MAX_SPAN}, got {span}")
        if not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
        self.shape = _lib.TisasrecShape(n_items, D, H, T, span, nb, 0)
        v = self._build(_spec(n_items, T, span, D, nb))
        # the reference's constructor, module by module, for its RNG order (tisasrec.py:194-233); LayerNorm draws nothing
        tables = (("item_emb", nn.Embedding(n_items + 1, D, padding_idx=0)), ("abs_pos_K_emb", nn.Embedding(T, D)),
                  ("abs_pos_V_emb", nn.Embedding(T, D)), ("time_matrix_K_emb", nn.Embedding(span + 1, D)),
                  ("time_matrix_V_emb", nn.Embedding(span + 1, D)))
        for name, emb in tables:
            v[name + ".weight"].copy_(emb.weight.data)
        v["last_layernorm.weight"].fill_(1.0)
        for b in range(nb):
            linears = [nn.Linear(D, D) for _ in range(3)]            # Q_w, K_w, V_w
            convs = [nn.Conv1d(D, D, kernel_size=1) for _ in range(2)]
            v[f"attention_layernorms.{b}.weight"].fill_(1.0)
            v[f"forward_layernorms.{b}.weight"].fill_(1.0)
            for name, mod in zip(("attention_layers.{}.Q_w", "attention_layers.{}.K_w", "attention_layers.{}.V_w",
                                  "forward_layers.{}.conv1", "forward_layers.{}.conv2"), linears + convs):
                v[name.format(b) + ".weight"].copy_(mod.weight.data)
                v[name.format(b) + ".bias"].copy_(mod.bias.data)
        for name, _ in tables:
            setattr(self, name, _ParamView(v[name + ".weight"]))
        ln = lambda p: _ParamView(v[p + ".weight"], v[p + ".bias"])   # noqa: E731
        self.attention_layernorms = nn.ModuleList(ln(f"attention_layernorms.{b}") for b in range(nb))
        self.attention_layers = nn.ModuleList(
            _TimeAwareAttentionParams(*(v[f"attention_layers.{b}.{m}.{t}"] for m in ("Q_w", "K_w", "V_w")
                                        for t in ("weight", "bias")))
            for b in range(nb))
        self.forward_layernorms = nn.ModuleList(ln(f"forward_layernorms.{b}") for b in range(nb))
        self.forward_layers = nn.ModuleList(
            _FeedForwardParams(*(v[f"forward_layers.{b}.{n}"] for n in ("conv1.weight", "conv1.bias", "conv2.weight",
                                                                       "conv2.bias")))
            for b in range(nb))
        self.last_layernorm = ln("last_layernorm")
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, seq_len):
        need = lib.hiprec_tisasrec_workspace_bytes(ctypes.byref(self.shape), int(batch), int(seq_len))
        if need == 0:
            raise ValueError(f"unsupported batch {batch} x sequence length {seq_len}")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def sequences(self, seqs):
        """``[B, T]`` ids (numpy, list or tensor) as ``(flat int64 device tensor, B, T)``; T must be <= maxlen."""
        shape = tuple(seqs.shape) if torch.is_tensor(seqs) else np.asarray(seqs).shape
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError("sequences must be [batch >= 1, length >= 1]")
        if shape[1] > self.maxlen:
            raise ValueError(f"sequence length {shape[1]} exceeds maxlen {self.maxlen}")
        return index_tensor(seqs, self._flat.device), int(shape[0]), int(shape[1])

    def time_matrices(self, time_matrices, time_seq, B, T):
        """The ``[B, T, T]`` relation matrices as a flat int32 device tensor; built on the device from ``time_seq
        [B, T]`` when ``time_matrices`` is None."""
        dev = self._flat.device
        if time_matrices is None:
            if time_seq is None:
                raise ValueError("either the time matrices or the time sequences are needed")
            ts = index_tensor(time_seq, dev)
            if ts.numel() != B * T:
                raise ValueError(f"time_seq holds {ts.numel()} entries where [{B}, {T}] is expected")
            out = torch.empty(B * T * T, dtype=torch.int32, device=dev)
            _lib.check(_lib.load().hiprec_time_relation(_lib.ptr(ts), B, T, self.time_span, _lib.ptr(out),
                                                        _lib.stream_ptr(dev)))
            return out
        if not torch.is_tensor(time_matrices):
            time_matrices = torch.as_tensor(np.asarray(time_matrices))
        if time_matrices.numel() != B * T * T:
            raise ValueError(f"time_matrices holds {time_matrices.numel()} entries where [{B}, {T}, {T}] is expected")
        return time_matrices.to(dev, torch.int32).reshape(-1).contiguous()

    # ---- reference API -----------------------------------------------------------------------------------------
    def seq2feats(self, user_ids, log_seqs, time_matrices, time_seq=None):
        """tisasrec.py:238-302 in eval mode (no dropout), without autograd: ``[B, T, D]`` features on the device."""
        lib = self._require_hip()
        dev = self._flat.device
        seq, B, T = self.sequences(log_seqs)
        tm = self.time_matrices(time_matrices, time_seq, B, T)
        stats = self._device_stats()
        feats = torch.empty((B, T, self.hidden_units), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, T)
        _lib.check(lib.hiprec_tisasrec_grad(
            ctypes.byref(self.shape), _lib.ptr(self._flat), None, _lib.ptr(seq), _lib.ptr(tm), None, None, B, T, 0.0, None,
            1.0, _lib.ptr(feats), _lib.ptr(stats), None, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return feats

    def forward(self, user_ids, log_seqs, time_matrices, pos_seqs, neg_seqs, time_seq=None):
        """tisasrec.py:304-335 in eval mode: ``(pos_logits, neg_logits)``, each ``[B, T]`` (``user_ids`` is unused)."""
        feats = self.seq2feats(user_ids, log_seqs, time_matrices, time_seq)
        dev = self._flat.device
        out = []
        for ids in (pos_seqs, neg_seqs):
            idx = index_tensor(ids, dev)
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) > self.item_num):
                raise IndexError(f"item id outside [0, {self.item_num}]")
            out.append((feats * self.item_emb.weight.data[idx].view(feats.shape)).sum(-1))
        return tuple(out)

    def predict(self, user_ids, log_seqs, time_matrices, item_indices, time_seq=None):
        """tisasrec.py:337-360: ``[n_seqs, n_indices]`` logits of the last position's feature against the rows of
        ``item_indices`` (1-D), through the exact-fp32 MFMA GEMM."""
        feats = self.seq2feats(user_ids, log_seqs, time_matrices, time_seq)
        lib, dev = _lib.load(), self._flat.device
        idx = index_tensor(item_indices, dev)
        if np.ndim(item_indices) != 1:
            raise ValueError("item_indices must be 1-D: one list of candidate items for every sequence")
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) > self.item_num):
            raise IndexError(f"item id outside [0, {self.item_num}]")
        rows = self.item_emb.weight.data[idx].contiguous()
        B, T, D = feats.shape
        logits = torch.empty((B, idx.numel()), dtype=torch.float32, device=dev)
        if idx.numel():
            last = feats[:, T - 1, :]
            _lib.check(lib.hiprec_gemm_f32(0, B, idx.numel(), D, ctypes.c_void_p(last.data_ptr()), T * D, _lib.ptr(rows),
                                           D, _lib.ptr(logits), idx.numel(), None, 0, None, 0, _lib.stream_ptr(dev)))
        return logits


class TiSASRecEngine(FlatModelEngine):
    """models/tisasrec.py:363-424."""

    def __init__(self, config):
        self.config = config
        print(config)
        self.model = TiSASRec(config["model"])
        self.num_batch = config["model"]["n_users"] // config["model"]["batch_size"]
        self._dropout_step = 0
        super(TiSASRecEngine, self).__init__(config)

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_tisasrec_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat TiSASRec buffer is not laid out as libhiprec.so expects; rebuild the library")

    # ---- dropout ---------------------------------------------------------------------------------------------
    def _mask_shapes(self, B, T):
        m = self.model
        D = m.hidden_units
        shapes = [(B * T, D)] * 3 + [(B, T, T, D)] * 2
        for _ in range(m.num_blocks):
            shapes += [(m.num_heads * B, T, T), (B * T, D), (B * T, D)]
        return shapes

    def _keep_masks(self, B, T, keep_masks):
        """The ``5 + 3 * num_blocks`` keep masks of one step as uint8 device tensors, or None (no dropout)."""
        m = self.model
        p = m.dropout_rate
        if p == 0.0 or not m.training:
            return None
        dev = m.flat.device
        shapes = self._mask_shapes(B, T)
        if keep_masks is not None:
            if len(keep_masks) != len(shapes):
                raise ValueError(f"{len(shapes)} keep masks expected (embedding, abs-pos-K, abs-pos-V, time-K, time-V; "
                                 f"per block attention, dropout1, dropout2), got {len(keep_masks)}")
            out = []
            for k, s in zip(keep_masks, shapes):
                t = torch.as_tensor(np.asarray(k.cpu() if torch.is_tensor(k) else k)).to(torch.uint8)
                if t.numel() != int(np.prod(s)):
                    raise ValueError(f"keep mask of {t.numel()} elements where {s} is expected")
                out.append(t.reshape(-1).contiguous().to(dev))
            return out
        cfg = self.config["model"]
        rng = cfg["dropout_rng"] if "dropout_rng" in cfg else "torch_cpu"
        self._dropout_step += 1
        D = m.hidden_units
        out = []
        if rng == "torch_cpu":
            # nn.Dropout on the CPU draws torch.empty_like(input).bernoulli_(1 - p): the embedding and the position rows
            # are [B, T, D], the gathered time rows [B, T, T, D], the attention's [H * B, T, T], and the two FFN dropouts
            # see Conv1d's [B, D, T] layout
            for i, s in enumerate(shapes):
                if i >= N_FIXED_MASKS and (i - N_FIXED_MASKS) % 3 != 0:
                    k = torch.empty(B, D, T).bernoulli_(1 - p).transpose(1, 2)
                else:
                    k = torch.empty(s).bernoulli_(1 - p)
                out.append(k.to(torch.uint8).reshape(-1).contiguous().to(dev))
        elif rng == "device":
            seed = int(cfg["dropout_seed"]) if "dropout_seed" in cfg else 0
            lib = _lib.load()
            for i, s in enumerate(shapes):
                buf = torch.empty(int(np.prod(s)), dtype=torch.uint8, device=dev)
                _lib.check(lib.hiprec_edge_dropout_mask(_lib.ptr(buf), buf.numel(), 1.0 - p, seed * 64 + i,
                                                        self._dropout_step, _lib.stream_ptr(dev)))
                out.append(buf)
        else:
            raise ValueError(f"unknown dropout_rng {rng!r}: 'torch_cpu' or 'device'")
        return out

    # ---- the step ----------------------------------------------------------------------------------------------
    def _enqueue_grad(self, batch_data, keep_masks=None):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 6:
            raise ValueError("a TiSASRec batch is (u, seq, time_seq, time_matrix, pos, neg)")
        _, seq, time_seq, time_matrix, pos, neg = batch_data
        seq_t, B, T = m.sequences(seq)
        pos_t, neg_t = index_tensor(pos, dev), index_tensor(neg, dev)
        if pos_t.numel() != seq_t.numel() or neg_t.numel() != seq_t.numel():
            raise ValueError("seq, pos and neg differ in shape")
        tm_t = m.time_matrices(time_matrix, time_seq, B, T)
        keep = self._keep_masks(B, T, keep_masks)
        self.last_keep_masks = keep
        keep_arr = None
        if keep is not None:
            keep_arr = (ctypes.c_void_p * len(keep))(*[k.data_ptr() for k in keep])
        ks = 1.0 / (1.0 - m.dropout_rate)
        ws = m.workspace(lib, B, T)
        l2 = m.l2_emb if self._dp_rank == 0 else 0.0
        _lib.check(lib.hiprec_tisasrec_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), _lib.ptr(tm_t),
            _lib.ptr(pos_t), _lib.ptr(neg_t), B, T, l2, keep_arr, ks, None, _lib.ptr(self._stats),
            _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))

    def backward_only(self, batch_data, keep_masks=None):
        """zero_grad + forward + loss + backward without the optimizer step: ``(loss, grads)``."""
        self._enqueue_grad(batch_data, keep_masks)
        st, grads = self._finish_backward_only()
        return st.loss, grads

    def train_single_batch(self, batch_data, ratings=None, keep_masks=None):
        """tisasrec.py:375-394: one step on ``(u, seq, time_seq, time_matrix, pos, neg)``, returns ``loss.item()``."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_grad(batch_data, keep_masks)
        self._enqueue_opt()
        return self._sync_stats().loss

    def train_an_epoch(self, sampler, epoch_id):
        """tisasrec.py:396-424: ``n_users // batch_size`` calls of ``sampler.next_batch()``, the float losses summed."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        total_loss = 0
        for _ in range(self.num_batch):
            u, seq, time_seq, time_matrix, pos, neg = sampler.next_batch()
            batch_data = (np.array(u), np.array(seq), np.array(time_seq),
                          None if time_matrix is None else np.array(time_matrix), np.array(pos), np.array(neg))
            total_loss += self.train_single_batch(batch_data)
        print("[Training Epoch {}], Loss {}".format(epoch_id, total_loss))
        self.writer.add_scalar("model/loss", total_loss, epoch_id)

    def recommend_next(self, log_seqs, time_matrices, k, seen=None, time_seq=None):
        """The ``k`` best next items for every sequence of ``log_seqs [n, T]`` with its ``time_matrices [n, T, T]`` (or
        None and ``time_seq [n, T]``): the last position's feature against ``item_emb.weight[1:]`` through
        ``recommend.topk_factors``; ids are shifted back by one, so the padding row can never be recommended.  ``seen``
        as in ``SASRecEngine.recommend_next``.  Returns ``(items [n, k] int64, scores [n, k] fp32)`` on the device,
        ``-1`` / ``-inf`` in a tail with nothing left."""
        from .recommend import topk_factors

        m = self.model
        feats = m.seq2feats(None, log_seqs, time_matrices, time_seq)
        n, T, _ = feats.shape
        table = m.item_emb.weight.data[1:]
        if seen is not None:
            rows, items = (index_tensor(x, feats.device) for x in seen)
            if rows.numel() != items.numel():
                raise ValueError("seen must be a (rows, items) pair of equally long id columns")
            keep = items != 0
            seen = (rows[keep], items[keep] - 1)
        items, scores = topk_factors(feats[:, T - 1, :], table, 1.0, None, torch.arange(n, device=feats.device), k, seen)
        return torch.where(items >= 0, items + 1, items), scores
