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
from ._seqrec import _FeedForwardParams, _SeqEngine, _SeqModel
from .flat_engine import _ParamView, index_tensor

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


class TiSASRec(_SeqModel):
    """models/tisasrec.py:168-360.  Flat buffer in ``state_dict()`` order (``_spec``)."""

    _WORKSPACE_BYTES, _PARAM_FLOATS = "hiprec_tisasrec_workspace_bytes", "hiprec_tisasrec_param_floats"

    def __init__(self, config):
        super().__init__()
        self.time_span = span = int(config["time_span"])
        self._configure(config, "TiSASRec needs num_blocks, num_heads, n_items, maxlen and time_span >= 1", span < 1)
        if span > MAX_SPAN:
            raise ValueError(f"time_span must be <= {MAX_SPAN}, got {span}")
        D, H, T, nb, n_items = self.hidden_units, self.num_heads, self.maxlen, self.num_blocks, self.item_num
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

    # ---- device-side plumbing --------------------------------------------------------------------------------
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
        return self._logits(self.seq2feats(user_ids, log_seqs, time_matrices, time_seq), pos_seqs, neg_seqs)

    def predict(self, user_ids, log_seqs, time_matrices, item_indices, time_seq=None):
        """tisasrec.py:337-360: ``[n_seqs, n_indices]`` logits of the last position's feature against the rows of
        ``item_indices`` (1-D), through the exact-fp32 MFMA GEMM."""
        return self._predict_from_feats(self.seq2feats(user_ids, log_seqs, time_matrices, time_seq), item_indices)


class TiSASRecEngine(_SeqEngine):
    """models/tisasrec.py:363-424 (``train_single_batch`` :375-394)."""

    _N_FIXED_MASKS, _MASK_NAMES = N_FIXED_MASKS, "embedding, abs-pos-K, abs-pos-V, time-K, time-V"

    def __init__(self, config):
        self.config = config
        print(config)
        self.model = TiSASRec(config["model"])
        self.num_batch = config["model"]["n_users"] // config["model"]["batch_size"]
        self._dropout_step = 0
        super(TiSASRecEngine, self).__init__(config)

    # ---- dropout ---------------------------------------------------------------------------------------------
    def _mask_shapes(self, B, T):
        m = self.model
        D = m.hidden_units
        shapes = [(B * T, D)] * 3 + [(B, T, T, D)] * 2
        for _ in range(m.num_blocks):
            shapes += [(m.num_heads * B, T, T), (B * T, D), (B * T, D)]
        return shapes

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
        keep_arr = self._keep_array(B, T, keep_masks)
        ks = 1.0 / (1.0 - m.dropout_rate)
        ws = m.workspace(lib, B, T)
        l2 = m.l2_emb if self._dp_rank == 0 else 0.0
        _lib.check(lib.hiprec_tisasrec_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), _lib.ptr(tm_t),
            _lib.ptr(pos_t), _lib.ptr(neg_t), B, T, l2, keep_arr, ks, None, _lib.ptr(self._stats),
            _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))

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
        return self._recommend_from_feats(self.model.seq2feats(None, log_seqs, time_matrices, time_seq), k, seen)
