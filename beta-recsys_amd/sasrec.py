"""Drop-in ``SASRec`` / ``SASRecEngine`` for beta_rec/models/sasrec.py on libhiprec.so.

Interface parity (file:line = beta_rec/models/sasrec.py): ``SASRec(config)`` :42-190 (``log2feats``, ``predict``),
``SASRecEngine(config)`` :193-240 (``train_single_batch((u, seq, pos, neg)) -> float``, ``train_an_epoch(sampler,
epoch_id)``).  Same config keys (``n_users n_items emb_dim maxlen num_blocks num_heads dropout_rate batch_size l2_emb``
under ``config["model"]``), same ``state_dict`` keys and shapes, and the same constructed weights for the same torch
seed: the constructor builds the reference's torch modules in the reference's order and copies them into the flat
buffer.

Kept from the reference on purpose:
* keys and values of the attention are the UN-normalised block input, the query is its LayerNorm, and the residual is
  taken on the normalised query (``x = Q + mha``); likewise the feed-forward residual is taken on its normalised input;
* the attention has a causal mask and NO key-padding mask: left-padded positions are attended to, their key is the
  key third of ``in_proj_bias``;
* the positional row is added at padded positions too, before the timeline mask;
* the L2 term is ``l2_emb * ||item_emb.weight||_2`` -- the norm, not its square, over the whole table: a dense gradient
  ``l2_emb * W / ||W||`` on every row at every step.  Where ``||W|| == 0`` the reference's ``torch.norm`` backward
  yields a zero gradient (its sub-gradient at the origin), and so does the kernel: no NaN reaches the update;
* the loss mask is ``pos != 0`` while the timeline mask is ``seq != 0``.

Dropout follows the NCF convention: ``config["model"]["dropout_rng"]`` is ``"torch_cpu"`` (default: one CPU draw per
mask of the reference's shapes, in its call order) or ``"device"`` (``hiprec_edge_dropout_mask`` seeded by
``dropout_seed`` and the step count); ``train_single_batch(batch, keep_masks=[...])`` takes the ``1 + 3 * num_blocks``
masks explicitly.  ``"torch_cpu"`` reproduces the reference's own masks for the same torch seed (pinned by
tests/golden/sasrec_rmsprop_drop.npz; see tools/gen_golden_sasrec.py for what was observed).  At ``dropout_rate == 0``
no mask is drawn or read.

Forward, loss and backward run in ``csrc/sasrec.hip`` and ``csrc/seqrec.hip`` (the stages shared with TiSASRec; the
projections through the grouped GEMM of ``csrc/ncf.hip``), the optimizer is the shared dense sweep.  There is no CPU
path.  What the two models share in Python is in ``_seqrec.py``.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import _lib
from ._seqrec import HEAD_WIDTHS, MAX_DIM, MAX_LEN, _FeedForwardParams, _SeqEngine, _SeqModel  # noqa: F401
from .flat_engine import _ParamView, index_tensor


class _AttentionParams(nn.Module):
    """The parameters of one ``nn.MultiheadAttention`` under its names, as views of the flat buffer."""

    def __init__(self, in_w, in_b, out_w, out_b):
        super().__init__()
        self.in_proj_weight = Parameter(in_w, requires_grad=False)
        self.in_proj_bias = Parameter(in_b, requires_grad=False)
        self.out_proj = _ParamView(out_w, out_b)


def _spec(n_items, maxlen, D, nb):
    spec = [("item_emb.weight", (n_items + 1, D)), ("pos_emb.weight", (maxlen, D))]
    for b in range(nb):
        spec += [(f"attention_layernorms.{b}.weight", (D,)), (f"attention_layernorms.{b}.bias", (D,))]
    for b in range(nb):
        spec += [(f"attention_layers.{b}.in_proj_weight", (3 * D, D)), (f"attention_layers.{b}.in_proj_bias", (3 * D,)),
                 (f"attention_layers.{b}.out_proj.weight", (D, D)), (f"attention_layers.{b}.out_proj.bias", (D,))]
    for b in range(nb):
        spec += [(f"forward_layernorms.{b}.weight", (D,)), (f"forward_layernorms.{b}.bias", (D,))]
    for b in range(nb):
        spec += [(f"forward_layers.{b}.conv1.weight", (D, D, 1)), (f"forward_layers.{b}.conv1.bias", (D,)),
                 (f"forward_layers.{b}.conv2.weight", (D, D, 1)), (f"forward_layers.{b}.conv2.bias", (D,))]
    return spec + [("last_layernorm.weight", (D,)), ("last_layernorm.bias", (D,))]


class SASRec(_SeqModel):
    """models/sasrec.py:42-190.  Flat buffer in ``state_dict()`` order (``_spec``)."""

    _WORKSPACE_BYTES, _PARAM_FLOATS = "hiprec_sasrec_workspace_bytes", "hiprec_sasrec_param_floats"

    def __init__(self, config):
        super().__init__()
        self._configure(config, "SASRec needs num_blocks >= 1, num_heads >= 1, n_items >= 1 and maxlen >= 1")
        D, H, T, nb, n_items = self.hidden_units, self.num_heads, self.maxlen, self.num_blocks, self.item_num
        self.shape = _lib.SasrecShape(n_items, D, H, T, nb)
        v = self._build(_spec(n_items, T, D, nb))
        # the reference's constructor, module by module, for its RNG order (sasrec.py:61-87); LayerNorm draws nothing
        item_emb = nn.Embedding(n_items + 1, D, padding_idx=0)
        pos_emb = nn.Embedding(T, D)
        v["item_emb.weight"].copy_(item_emb.weight.data)
        v["pos_emb.weight"].copy_(pos_emb.weight.data)
        v["last_layernorm.weight"].fill_(1.0)
        for b in range(nb):
            mha = nn.MultiheadAttention(D, H, self.dropout_rate)
            conv1 = nn.Conv1d(D, D, kernel_size=1)
            conv2 = nn.Conv1d(D, D, kernel_size=1)
            v[f"attention_layernorms.{b}.weight"].fill_(1.0)
            v[f"forward_layernorms.{b}.weight"].fill_(1.0)
            v[f"attention_layers.{b}.in_proj_weight"].copy_(mha.in_proj_weight.data)
            v[f"attention_layers.{b}.in_proj_bias"].copy_(mha.in_proj_bias.data)
            v[f"attention_layers.{b}.out_proj.weight"].copy_(mha.out_proj.weight.data)
            v[f"attention_layers.{b}.out_proj.bias"].copy_(mha.out_proj.bias.data)
            for name, conv in (("conv1", conv1), ("conv2", conv2)):
                v[f"forward_layers.{b}.{name}.weight"].copy_(conv.weight.data)
                v[f"forward_layers.{b}.{name}.bias"].copy_(conv.bias.data)
        self.item_emb = _ParamView(v["item_emb.weight"])
        self.pos_emb = _ParamView(v["pos_emb.weight"])
        ln = lambda p: _ParamView(v[p + ".weight"], v[p + ".bias"])   # noqa: E731
        self.attention_layernorms = nn.ModuleList(ln(f"attention_layernorms.{b}") for b in range(nb))
        self.attention_layers = nn.ModuleList(
            _AttentionParams(*(v[f"attention_layers.{b}.{n}"] for n in ("in_proj_weight", "in_proj_bias",
                                                                       "out_proj.weight", "out_proj.bias")))
            for b in range(nb))
        self.forward_layernorms = nn.ModuleList(ln(f"forward_layernorms.{b}") for b in range(nb))
        self.forward_layers = nn.ModuleList(
            _FeedForwardParams(*(v[f"forward_layers.{b}.{n}"] for n in ("conv1.weight", "conv1.bias", "conv2.weight",
                                                                       "conv2.bias")))
            for b in range(nb))
        self.last_layernorm = ln("last_layernorm")

    # ---- reference API -----------------------------------------------------------------------------------------
    def log2feats(self, log_seqs):
        """sasrec.py:92-136 in eval mode (no dropout), without autograd: ``[B, T, D]`` features on the device."""
        lib = self._require_hip()
        dev = self._flat.device
        seq, B, T = self.sequences(log_seqs)
        stats = self._device_stats()
        feats = torch.empty((B, T, self.hidden_units), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, T)
        _lib.check(lib.hiprec_sasrec_grad(
            ctypes.byref(self.shape), _lib.ptr(self._flat), None, _lib.ptr(seq), None, None, B, T, 0.0, None, 1.0,
            _lib.ptr(feats), _lib.ptr(stats), None, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return feats

    def forward(self, user_ids, log_seqs, pos_seqs, neg_seqs):
        """sasrec.py:138-165 in eval mode: ``(pos_logits, neg_logits)``, each ``[B, T]`` (``user_ids`` is unused)."""
        return self._logits(self.log2feats(log_seqs), pos_seqs, neg_seqs)

    def predict(self, user_ids, log_seqs, item_indices):
        """sasrec.py:167-190: ``[n_seqs, n_indices]`` logits of the last position's feature against the rows of
        ``item_indices`` (1-D), through the exact-fp32 MFMA GEMM."""
        return self._predict_from_feats(self.log2feats(log_seqs), item_indices)


class SASRecEngine(_SeqEngine):
    """models/sasrec.py:193-240 (``train_single_batch`` :205-224)."""

    _N_FIXED_MASKS, _MASK_NAMES = 1, "embedding"

    def __init__(self, config):
        self.config = config
        print(config)
        self.model = SASRec(config["model"])
        self.num_batch = config["model"]["n_users"] // config["model"]["batch_size"]
        self._dropout_step = 0
        super(SASRecEngine, self).__init__(config)

    # ---- dropout ---------------------------------------------------------------------------------------------
    def _mask_shapes(self, B, T):
        m = self.model
        shapes = [(B * T, m.hidden_units)]
        for _ in range(m.num_blocks):
            shapes += [(B * m.num_heads, T, T), (B * T, m.hidden_units), (B * T, m.hidden_units)]
        return shapes

    # ---- the step ----------------------------------------------------------------------------------------------
    def _enqueue_grad(self, batch_data, keep_masks=None):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 4:
            raise ValueError("a SASRec batch is (u, seq, pos, neg)")
        _, seq, pos, neg = batch_data
        seq_t, B, T = m.sequences(seq)
        pos_t, neg_t = index_tensor(pos, dev), index_tensor(neg, dev)
        if pos_t.numel() != seq_t.numel() or neg_t.numel() != seq_t.numel():
            raise ValueError("seq, pos and neg differ in shape")
        keep_arr = self._keep_array(B, T, keep_masks)
        ks = 1.0 / (1.0 - m.dropout_rate)
        ws = m.workspace(lib, B, T)
        l2 = m.l2_emb if self._dp_rank == 0 else 0.0
        _lib.check(lib.hiprec_sasrec_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), _lib.ptr(pos_t),
            _lib.ptr(neg_t), B, T, l2, keep_arr, ks, None, _lib.ptr(self._stats), _lib.ptr(self._scratch),
            self._scratch.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))

    def train_an_epoch(self, sampler, epoch_id):
        """sasrec.py:226-240: ``n_users // batch_size`` calls of ``sampler.next_batch()``, the float losses summed."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        total_loss = 0
        for _ in range(self.num_batch):
            u, seq, pos, neg = sampler.next_batch()
            batch_data = np.array(u), np.array(seq), np.array(pos), np.array(neg)
            total_loss += self.train_single_batch(batch_data)
        print("[Training Epoch {}], Loss {}".format(epoch_id, total_loss))
        self.writer.add_scalar("model/loss", total_loss, epoch_id)

    def recommend_next(self, log_seqs, k, seen=None):
        """The ``k`` best next items for every sequence of ``log_seqs [n, T]``: the last position's feature against
        ``item_emb.weight[1:]`` through ``recommend.topk_factors``; ids are shifted back by one, so the padding row can
        never be recommended.  ``seen``: None, or a ``(rows, items)`` pair of equally long id columns -- row ``r`` of
        ``log_seqs`` is never recommended item ``i`` (item ids as the model knows them, 1 .. n_items).  Returns
        ``(items [n, k] int64, scores [n, k] fp32)`` on the device, ``-1`` / ``-inf`` in a tail with nothing left."""
        return self._recommend_from_feats(self.model.log2feats(log_seqs), k, seen)
