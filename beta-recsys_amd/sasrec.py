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

Forward, loss and backward run in ``csrc/sasrec.hip`` (the projections through the grouped GEMM of ``csrc/ncf.hip``),
the optimizer is the shared dense sweep.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor

MAX_DIM, MAX_LEN, HEAD_WIDTHS = 128, 256, (16, 32, 64)


class _AttentionParams(nn.Module):
    """The parameters of one ``nn.MultiheadAttention`` under its names, as views of the flat buffer."""

    def __init__(self, in_w, in_b, out_w, out_b):
        super().__init__()
        self.in_proj_weight = Parameter(in_w, requires_grad=False)
        self.in_proj_bias = Parameter(in_b, requires_grad=False)
        self.out_proj = _ParamView(out_w, out_b)


class _FeedForwardParams(nn.Module):
    """``PointWiseFeedForward``'s two ``Conv1d(kernel_size=1)``."""

    def __init__(self, w1, b1, w2, b2):
        super().__init__()
        self.conv1 = _ParamView(w1, b1)
        self.conv2 = _ParamView(w2, b2)


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


class SASRec(_FlatModel):
    """models/sasrec.py:42-190.  Flat buffer in ``state_dict()`` order (``_spec``)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.user_num = config["n_users"]
        self.item_num = int(config["n_items"])
        self.hidden_units = int(config["emb_dim"])
        self.maxlen = int(config["maxlen"])
        self.num_blocks = int(config["num_blocks"])
        self.num_heads = int(config["num_heads"])
        self.dropout_rate = float(config["dropout_rate"])
        self.batch_size = config["batch_size"]
        self.l2_emb = float(config["l2_emb"])
        D, H, T, nb, n_items = self.hidden_units, self.num_heads, self.maxlen, self.num_blocks, self.item_num
        if nb < 1 or H < 1 or n_items < 1 or T < 1:
            raise ValueError("SASRec needs num_blocks >= 1, num_heads >= 1, n_items >= 1 and maxlen >= 1")
        if D % H != 0 or D // H not in HEAD_WIDTHS:
            raise ValueError(f"the HIP attention supports head widths emb_dim / num_heads in {HEAD_WIDTHS}; "
                             f"got emb_dim {D}, num_heads {H}")
        if D > MAX_DIM:
            raise ValueError(f"emb_dim must be <= {MAX_DIM}, got {D}")
        if T > MAX_LEN:
            raise ValueError(f"maxlen must be <= {MAX_LEN}, got {T}")
        if not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
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
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, seq_len):
        need = lib.hiprec_sasrec_workspace_bytes(ctypes.byref(self.shape), int(batch), int(seq_len))
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
        feats = self.log2feats(log_seqs)
        dev = self._flat.device
        out = []
        for ids in (pos_seqs, neg_seqs):
            idx = index_tensor(ids, dev)
            if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) > self.item_num):
                raise IndexError(f"item id outside [0, {self.item_num}]")
            out.append((feats * self.item_emb.weight.data[idx].view(feats.shape)).sum(-1))
        return tuple(out)

    def predict(self, user_ids, log_seqs, item_indices):
        """sasrec.py:167-190: ``[n_seqs, n_indices]`` logits of the last position's feature against the rows of
        ``item_indices`` (1-D), through the exact-fp32 MFMA GEMM."""
        feats = self.log2feats(log_seqs)
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


class SASRecEngine(FlatModelEngine):
    """models/sasrec.py:193-240."""

    def __init__(self, config):
        self.config = config
        print(config)
        self.model = SASRec(config["model"])
        self.num_batch = config["model"]["n_users"] // config["model"]["batch_size"]
        self._dropout_step = 0
        super(SASRecEngine, self).__init__(config)

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_sasrec_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat SASRec buffer is not laid out as libhiprec.so expects; rebuild the library")

    # ---- dropout ---------------------------------------------------------------------------------------------
    def _mask_shapes(self, B, T):
        m = self.model
        shapes = [(B * T, m.hidden_units)]
        for _ in range(m.num_blocks):
            shapes += [(B * m.num_heads, T, T), (B * T, m.hidden_units), (B * T, m.hidden_units)]
        return shapes

    def _keep_masks(self, B, T, keep_masks):
        """The ``1 + 3 * num_blocks`` keep masks of one step as uint8 device tensors, or None (no dropout)."""
        m = self.model
        p = m.dropout_rate
        if p == 0.0 or not m.training:
            return None
        dev = m.flat.device
        shapes = self._mask_shapes(B, T)
        if keep_masks is not None:
            if len(keep_masks) != len(shapes):
                raise ValueError(f"{len(shapes)} keep masks expected (embedding; per block attention, dropout1, "
                                 f"dropout2), got {len(keep_masks)}")
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
            # nn.Dropout / F.dropout on the CPU draw torch.empty_like(input).bernoulli_(1 - p): the embedding's input is
            # [B, T, D], the attention's [B * H, T, T], the two FFN dropouts see Conv1d's [B, D, T] layout
            for i, s in enumerate(shapes):
                if i == 0 or i % 3 == 1:
                    k = torch.empty(s).bernoulli_(1 - p)
                else:
                    k = torch.empty(B, D, T).bernoulli_(1 - p).transpose(1, 2)
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
        if len(batch_data) != 4:
            raise ValueError("a SASRec batch is (u, seq, pos, neg)")
        _, seq, pos, neg = batch_data
        seq_t, B, T = m.sequences(seq)
        pos_t, neg_t = index_tensor(pos, dev), index_tensor(neg, dev)
        if pos_t.numel() != seq_t.numel() or neg_t.numel() != seq_t.numel():
            raise ValueError("seq, pos and neg differ in shape")
        keep = self._keep_masks(B, T, keep_masks)
        self.last_keep_masks = keep
        keep_arr = None
        if keep is not None:
            keep_arr = (ctypes.c_void_p * len(keep))(*[k.data_ptr() for k in keep])
        ks = 1.0 / (1.0 - m.dropout_rate)
        ws = m.workspace(lib, B, T)
        l2 = m.l2_emb if self._dp_rank == 0 else 0.0
        _lib.check(lib.hiprec_sasrec_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), _lib.ptr(pos_t),
            _lib.ptr(neg_t), B, T, l2, keep_arr, ks, None, _lib.ptr(self._stats), _lib.ptr(self._scratch),
            self._scratch.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))

    def backward_only(self, batch_data, keep_masks=None):
        """zero_grad + forward + loss + backward without the optimizer step: ``(loss, grads)``."""
        self._enqueue_grad(batch_data, keep_masks)
        st, grads = self._finish_backward_only()
        return st.loss, grads

    def train_single_batch(self, batch_data, ratings=None, keep_masks=None):
        """sasrec.py:205-224: one step on ``(u, seq, pos, neg)``, returns ``loss.item()``."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_grad(batch_data, keep_masks)
        self._enqueue_opt()
        return self._sync_stats().loss

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
        from .recommend import topk_factors

        m = self.model
        feats = m.log2feats(log_seqs)
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
