"""``BERT4Rec`` / ``BERT4RecEngine`` on libhiprec.so: the bidirectional, cloze-trained sequence model of Sun et al.
(CIKM 2019).  The reference has no such model; ``include/hiprec.h`` holds the definition, ``tests/bert4rec_torch.py``
restates it in plain torch.

Ids: 0 is padding, 1 .. n_items are items, ``mask_id = n_items + 1`` is the ``[MASK]`` token.  Config keys
(``config["model"]``): ``n_users n_items emb_dim maxlen num_blocks num_heads dropout_rate batch_size``; optional
``ffn_dim`` (1 .. 512, default ``4 * emb_dim``) and ``mask_prob`` (default 0.2, read by whoever builds the
``data.ClozeSampler``).  There is no regulariser.

The model is post-LN: ``x = LN(x + drop(sublayer(x)))``; attention runs over all keys with ``seq != 0``; the
feed-forward is ``fc2(gelu(fc1(x)))`` with the exact (erf) GELU.  The loss is the cross-entropy over items 1 .. n_items
of ``<LN(gelu(dense(x))), item_emb[j]> + out_bias[j]`` at the labelled positions; the ``[n_labelled, n_items]`` score
matrix is never formed (csrc/bert4rec.hip).

Dropout follows the other sequence models (``_seqrec._SeqEngine``): ``dropout_rng`` is ``"device"`` by default here
(there is no reference stream to imitate), ``train_single_batch(batch, keep_masks=[...])`` takes the
``1 + 3 * num_blocks`` masks explicitly: embedding ``[B * T, D]``, then per block the probabilities ``[B * H, T, T]``,
dropout1 and dropout2 ``[B * T, D]``.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import _lib
from ._seqrec import _SeqEngine, _SeqModel
from .flat_engine import _ParamView, index_tensor
from .sasrec import _AttentionParams

MAX_FFN = 512


class _GeluFeedForwardParams(nn.Module):
    def __init__(self, w1, b1, w2, b2):
        super().__init__()
        self.fc1 = _ParamView(w1, b1)
        self.fc2 = _ParamView(w2, b2)


class _HeadParams(nn.Module):
    """``head.dense`` / ``head.layernorm`` as views; calling it applies the head (``BERT4Rec.head(rows)``)."""

    def __init__(self, dw, db, lw, lb, apply_fn):
        super().__init__()
        self.dense = _ParamView(dw, db)
        self.layernorm = _ParamView(lw, lb)
        self._apply_fn = apply_fn

    def forward(self, rows):
        return self._apply_fn(rows)


def spec(n_items, maxlen, D, nb, F):
    """``(name, shape)`` of every parameter in ``state_dict()`` order: the layout of the flat buffer."""
    s = [("item_emb.weight", (n_items + 2, D)), ("pos_emb.weight", (maxlen, D)),
         ("emb_layernorm.weight", (D,)), ("emb_layernorm.bias", (D,))]
    for b in range(nb):
        s += [(f"attention_layers.{b}.in_proj_weight", (3 * D, D)), (f"attention_layers.{b}.in_proj_bias", (3 * D,)),
              (f"attention_layers.{b}.out_proj.weight", (D, D)), (f"attention_layers.{b}.out_proj.bias", (D,))]
    for b in range(nb):
        s += [(f"attention_layernorms.{b}.weight", (D,)), (f"attention_layernorms.{b}.bias", (D,))]
    for b in range(nb):
        s += [(f"forward_layers.{b}.fc1.weight", (F, D)), (f"forward_layers.{b}.fc1.bias", (F,)),
              (f"forward_layers.{b}.fc2.weight", (D, F)), (f"forward_layers.{b}.fc2.bias", (D,))]
    for b in range(nb):
        s += [(f"forward_layernorms.{b}.weight", (D,)), (f"forward_layernorms.{b}.bias", (D,))]
    return s + [("head.dense.weight", (D, D)), ("head.dense.bias", (D,)), ("head.layernorm.weight", (D,)),
                ("head.layernorm.bias", (D,)), ("out_bias", (n_items + 1,))]


class BERT4Rec(_SeqModel):
    """Flat buffer in ``state_dict()`` order (``spec``).  Truncated-normal(std 0.02) tables and matrices, zero biases,
    unit LayerNorm weights; the padding row is zero."""

    _WORKSPACE_BYTES, _PARAM_FLOATS = "hiprec_bert4rec_workspace_bytes", "hiprec_bert4rec_param_floats"

    def __init__(self, config):
        super().__init__()
        config = dict(config)
        config.setdefault("l2_emb", 0.0)          # no regulariser: the shared parser's key is supplied here
        self._configure(config, "BERT4Rec needs num_blocks >= 1, num_heads >= 1, n_items >= 1 and maxlen >= 1")
        self.l2_emb = 0.0
        D, H, T, nb, n_items = self.hidden_units, self.num_heads, self.maxlen, self.num_blocks, self.item_num
        self.ffn_dim = int(config["ffn_dim"]) if config.get("ffn_dim") is not None else 4 * D
        if not 1 <= self.ffn_dim <= MAX_FFN:
            raise ValueError(f"ffn_dim must be in 1..{MAX_FFN}, got {self.ffn_dim}")
        self.mask_prob = float(config.get("mask_prob", 0.2))
        if not 0.0 < self.mask_prob < 1.0:
            raise ValueError("mask_prob must be in (0, 1)")
        self.mask_id = n_items + 1
        self.shape = _lib.Bert4recShape(n_items, D, H, T, nb, self.ffn_dim, 0)
        v = self._build(spec(n_items, T, D, nb, self.ffn_dim))
        for name, view in v.items():
            if name.endswith("bias"):
                continue
            if "layernorm" in name:
                view.fill_(1.0)
            else:
                nn.init.trunc_normal_(view, std=0.02, a=-0.04, b=0.04)
        v["item_emb.weight"][0].zero_()
        ln = lambda p: _ParamView(v[p + ".weight"], v[p + ".bias"])   # noqa: E731
        self.item_emb = _ParamView(v["item_emb.weight"])
        self.pos_emb = _ParamView(v["pos_emb.weight"])
        self.emb_layernorm = ln("emb_layernorm")
        self.attention_layers = nn.ModuleList(
            _AttentionParams(*(v[f"attention_layers.{b}.{n}"] for n in ("in_proj_weight", "in_proj_bias",
                                                                       "out_proj.weight", "out_proj.bias")))
            for b in range(nb))
        self.attention_layernorms = nn.ModuleList(ln(f"attention_layernorms.{b}") for b in range(nb))
        self.forward_layers = nn.ModuleList(
            _GeluFeedForwardParams(*(v[f"forward_layers.{b}.{n}"] for n in ("fc1.weight", "fc1.bias", "fc2.weight",
                                                                           "fc2.bias")))
            for b in range(nb))
        self.forward_layernorms = nn.ModuleList(ln(f"forward_layernorms.{b}") for b in range(nb))
        # model.head(rows) applies dense + GELU + LayerNorm to the given rows (the module is callable)
        self.head = _HeadParams(v["head.dense.weight"], v["head.dense.bias"], v["head.layernorm.weight"],
                                v["head.layernorm.bias"], self._head_rows)
        self.out_bias = Parameter(v["out_bias"], requires_grad=False)

    def state_dict(self, *args, **kwargs):
        """In the order of the flat buffer (a module's own parameter, ``out_bias``, would otherwise come first)."""
        sd = super().state_dict(*args, **kwargs)
        names = [n for n, _ in self._spec]
        if set(names) != set(sd):
            return sd
        return type(sd)((n, sd[n]) for n in names)

    # ---- calls ---------------------------------------------------------------------------------------------------
    def log2feats(self, seqs):
        """The last block's output in eval mode, without autograd: ``[B, T, D]`` on the device.  ``seqs [B, T]`` holds
        ids in 0 .. n_items + 1 (``[MASK]`` included)."""
        lib = self._require_hip()
        dev = self._flat.device
        seq, B, T = self.sequences(seqs)
        stats = self._device_stats()
        feats = torch.empty((B, T, self.hidden_units), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, T)
        _lib.check(lib.hiprec_bert4rec_grad(
            ctypes.byref(self.shape), _lib.ptr(self._flat), None, _lib.ptr(seq), 0, None, None, B, T, None, 1.0,
            _lib.ptr(feats), _lib.ptr(stats), None, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return feats

    def _head_rows(self, rows):
        """``head.layernorm(gelu(head.dense(rows)))`` for ``rows [n, D]`` (a device tensor): ``[n, D]``."""
        lib = self._require_hip()
        dev = self._flat.device
        rows = torch.as_tensor(rows, dtype=torch.float32, device=dev).contiguous()
        if rows.dim() != 2 or rows.shape[1] != self.hidden_units or rows.shape[0] < 1:
            raise ValueError(f"rows must be [n >= 1, {self.hidden_units}]")
        n, D = int(rows.shape[0]), self.hidden_units
        out = torch.empty_like(rows)
        tmp = torch.empty(2 * ((n * D + 3) // 4 * 4) + 2 * ((n + 3) // 4 * 4), dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_bert4rec_head(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(rows), n,
                                            _lib.ptr(out), _lib.ptr(tmp), tmp.numel(), _lib.stream_ptr(dev)))
        return out

    def _class_ids(self, ids):
        idx = index_tensor(ids, self._flat.device)
        if idx.numel() and (int(idx.min()) < 1 or int(idx.max()) > self.item_num):
            raise IndexError(f"item id outside [1, {self.item_num}]: padding and [MASK] are no classes")
        return idx

    def predict(self, seqs, item_indices):
        """``[n_seqs, n_indices]`` logits of the LAST position of every sequence (put ``mask_id`` there to ask for the
        next item) against the items ``item_indices`` (1-D, ids in 1 .. n_items), ``out_bias`` included."""
        lib, dev = _lib.load(), self._flat.device
        if np.ndim(item_indices) != 1:
            raise ValueError("item_indices must be 1-D: one list of candidate items for every sequence")
        idx = self._class_ids(item_indices)
        feats = self.log2feats(seqs)
        B, D = feats.shape[0], self.hidden_units
        h = self.head(feats[:, -1, :])
        logits = torch.empty((B, idx.numel()), dtype=torch.float32, device=dev)
        if idx.numel():
            rows = self.item_emb.weight.data[idx].contiguous()
            _lib.check(lib.hiprec_gemm_f32(0, B, idx.numel(), D, _lib.ptr(h), D, _lib.ptr(rows), D, _lib.ptr(logits),
                                           idx.numel(), None, 0, None, 0, _lib.stream_ptr(dev)))
            logits += self.out_bias.data[idx]
        return logits


def labelled_positions(labels, n, device):
    """``labels [B, T]`` (0 = not predicted) as the compact list the kernels take: ``(n_lab, lab_pos, lab_item)``, the
    flat positions ascending.  Host labels go through numpy (no device sync); device labels through ``torch.nonzero``."""
    if torch.is_tensor(labels) and labels.device.type != "cpu":
        flat = labels.to(device, torch.int64).reshape(-1)
        pos = torch.nonzero(flat).reshape(-1)
        items = flat[pos]
    else:
        flat = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels, dtype=np.int64).reshape(-1)
        at = np.flatnonzero(flat)
        pos, items = torch.from_numpy(at).to(device), torch.from_numpy(flat[at]).to(device)
    if flat.shape[0] != n:
        raise ValueError("seq and labels differ in shape")
    return int(pos.numel()), pos.contiguous(), items.contiguous()


class BERT4RecEngine(_SeqEngine):
    """``train_single_batch((users, seq, labels)) -> float``, ``train_an_epoch(sampler, epoch_id)``,
    ``recommend_next(histories, k, seen=None)``; checkpoints through the flat-model base."""

    _N_FIXED_MASKS, _MASK_NAMES = 1, "embedding"

    def __init__(self, config):
        self.config = config
        if "dropout_rng" not in config["model"]:
            config["model"]["dropout_rng"] = "device"
        print(config)
        self.model = BERT4Rec(config["model"])
        self.num_batch = config["model"]["n_users"] // config["model"]["batch_size"]
        self._dropout_step = 0
        super(BERT4RecEngine, self).__init__(config)

    def _mask_shapes(self, B, T):
        m = self.model
        shapes = [(B * T, m.hidden_units)]
        for _ in range(m.num_blocks):
            shapes += [(B * m.num_heads, T, T), (B * T, m.hidden_units), (B * T, m.hidden_units)]
        return shapes

    def _enqueue_grad(self, batch_data, keep_masks=None):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 3:
            raise ValueError("a BERT4Rec batch is (users, seq, labels)")
        _, seq, labels = batch_data
        seq_t, B, T = m.sequences(seq)
        n_lab, lab_pos, lab_item = labelled_positions(labels, B * T, dev)
        keep_arr = self._keep_array(B, T, keep_masks)
        ks = 1.0 / (1.0 - m.dropout_rate)
        ws = m.workspace(lib, B, T)
        self._lab = (lab_pos, lab_item)      # alive until the call has run
        _lib.check(lib.hiprec_bert4rec_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), n_lab,
            _lib.ptr(lab_pos) if n_lab else None, _lib.ptr(lab_item) if n_lab else None, B, T, keep_arr, ks, None,
            _lib.ptr(self._stats), _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)))

    def train_an_epoch(self, sampler, epoch_id):
        """``n_users // batch_size`` calls of ``sampler.next_batch()``, the float losses summed."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        total_loss = 0
        for _ in range(self.num_batch):
            u, seq, labels = sampler.next_batch()
            total_loss += self.train_single_batch((np.array(u), np.array(seq), np.array(labels)))
        print("[Training Epoch {}], Loss {}".format(epoch_id, total_loss))
        self.writer.add_scalar("model/loss", total_loss, epoch_id)

    def query_sequences(self, histories):
        """Item histories (a ``[n, L]`` array left-padded with 0, or a list of lists) as the model is queried: the last
        ``maxlen - 1`` items of each, then ``[MASK]``, left-padded: ``[n, T]`` int64.  A ``[MASK]`` id inside a history
        raises."""
        m = self.model
        if torch.is_tensor(histories):
            histories = histories.cpu().numpy()
        rows = [np.asarray(h, dtype=np.int64).reshape(-1) for h in histories]
        if not rows:
            raise ValueError("no history given")
        rows = [r[r != 0][-(m.maxlen - 1):] if m.maxlen > 1 else r[:0] for r in rows]
        for r in rows:
            if r.size and (r.min() < 1 or r.max() > m.item_num):
                raise ValueError(f"a history holds an id outside [1, {m.item_num}] (the [MASK] token {m.mask_id} is "
                                 "appended here, never passed in)")
        T = max(r.size for r in rows) + 1
        out = np.zeros((len(rows), T), dtype=np.int64)
        for i, r in enumerate(rows):
            out[i, T - 1 - r.size:T - 1] = r
        out[:, -1] = m.mask_id
        return out

    def recommend_next(self, histories, k, seen=None):
        """The ``k`` best next items for every history: ``[MASK]`` is appended, the eval forward and the head run on
        that last position, and items 1 .. n_items are ranked by ``<h, item_emb[j]> + out_bias[j]`` through
        ``recommend.topk_factors`` (ties to the lower id).  ``seen``: None, or a ``(rows, items)`` pair of equally long
        id columns -- row ``r`` is never recommended item ``i`` (ids 1 .. n_items; 0 entries are ignored).  Returns
        ``(items [n, k] int64, scores [n, k] fp32)`` on the device, ``-1`` / ``-inf`` in a tail with nothing left; neither
        0 nor ``mask_id`` can occur."""
        from .recommend import topk_factors

        m = self.model
        feats = m.log2feats(self.query_sequences(histories))
        h = m.head(feats[:, -1, :])
        n, dev = h.shape[0], h.device
        table = m.item_emb.weight.data[1:m.item_num + 1]
        bias = m.out_bias.data[1:]
        if seen is not None:
            rows, items = (index_tensor(x, dev) for x in seen)
            if rows.numel() != items.numel():
                raise ValueError("seen must be a (rows, items) pair of equally long id columns")
            if items.numel() and (int(items.min()) < 0 or int(items.max()) > m.item_num):
                raise ValueError(f"seen holds an item id outside [0, {m.item_num}] (the [MASK] token {m.mask_id} is no item)")
            if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
                raise ValueError(f"seen holds a row outside [0, {n})")
            keep = items != 0
            seen = (rows[keep], items[keep] - 1)
        items, scores = topk_factors(h, table, 1.0, bias, torch.arange(n, device=dev), k, seen)
        return torch.where(items >= 0, items + 1, items), scores
