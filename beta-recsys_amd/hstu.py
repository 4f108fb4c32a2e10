"""``HSTU`` / ``HSTUEngine``: the Hierarchical Sequential Transduction Unit (Zhai et al., "Actions Speak Louder than Words:
Trillion-Parameter Sequential Transducers for Generative Recommendations", ICML 2024) on libhiprec.so.

There is no counterpart in the reference; the paper and ``tests/hstu_torch.py`` (a restatement in plain torch ops) are the
specification, ``include/hiprec.h`` states the contract:

* items are ``1 .. n_items`` and 0 is padding (``item_emb.weight`` row 0 is zero and stays zero); a batch is
  ``(u, seq, time_seq, pos, neg)``, each ``[B, L <= maxlen]`` (``u`` is ignored), or ``(u, seq, pos, neg)`` with
  ``rel_bias="pos"``; shorter inputs are left-padded with 0 to ``maxlen``;
* ``x = (item_emb[seq] sqrt(D) + pos_emb[t]) * valid``; per block ``u | v | q | k = SiLU(LN(x) uvqk)``, the attention
  weights are ``SiLU(q k^T + pos_w[offset] + ts_w[time bucket]) / maxlen`` under the causal and padding masks -- pointwise,
  no softmax --, ``x = (x + o(LN_noaffine(A v) * u)) * valid``; ``f = LN(x)``; there is no feed-forward sub-layer;
* the time bucket of a pair is ``min(num_buckets, floor(ln(max(|t_next(i) - t_j|, 1)) / 0.301))``, exact in integers;
* the loss is the SASRec family's BCE-with-logits over ``pos != 0`` with one negative per position.

Config keys under ``config["model"]``: ``n_users n_items emb_dim maxlen num_blocks num_heads attention_dim linear_dim
dropout_rate batch_size optimizer lr`` and, optional, ``num_buckets`` (1 .. 255, default 128), ``rel_bias``
(``"pos_time"``, the default, or ``"pos"``), ``l2_emb`` (default 0), ``dropout_rng`` (``"device"``, the only stream there
is) and ``dropout_seed``.  ``train_single_batch(batch, keep_masks=[...])`` takes the ``1 + num_blocks`` keep masks
explicitly: the embedding's ``[B * maxlen, emb_dim]``, then per block the gated output's ``[B * maxlen, H * linear_dim]``.

The attention runs in ``csrc/hstu.hip``; no ``[B, H, T, T]`` tensor in fp32 reaches memory.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._stats import _new_stats, raise_on_status, read_stats
from ._seqrec import HEAD_WIDTHS, MAX_DIM, MAX_LEN, _SeqEngine, _SeqModel
from .flat_engine import _ParamView, index_tensor

MAX_BLOCKS, MAX_BUCKETS = 16, 255
REL_BIAS = {"pos_time": 0, "pos": 1}


def time_thresholds(num_buckets):
    """``thr[k - 1]``: the smallest integer gap that falls into bucket ``k``, as the library's host code derives it."""
    out = np.empty(int(num_buckets), dtype=np.int64)
    _lib.check(_lib.load().hiprec_hstu_time_thresholds(int(num_buckets), out.ctypes.data))
    return out


def spec(n_items, maxlen, D, nb, H, dqk, dv, num_buckets, rel_bias):
    """``(name, shape)`` of every parameter in ``state_dict()`` order: the layout of the flat buffer."""
    s = [("item_emb.weight", (n_items + 1, D)), ("pos_emb.weight", (maxlen, D))]
    for b in range(nb):
        p = f"blocks.{b}."
        s += [(p + "norm.weight", (D,)), (p + "norm.bias", (D,)), (p + "uvqk", (D, 2 * H * dv + 2 * H * dqk)),
              (p + "pos_w", (2 * maxlen - 1,))]
        if rel_bias == "pos_time":
            s.append((p + "ts_w", (num_buckets + 1,)))
        s += [(p + "o.weight", (D, H * dv)), (p + "o.bias", (D,))]
    return s + [("last_norm.weight", (D,)), ("last_norm.bias", (D,))]


class _BlockParams(nn.Module):
    """One block's parameters as views of the flat buffer, registered in its order."""

    def __init__(self, v, b, with_time):
        super().__init__()
        p = f"blocks.{b}."
        self.norm = _ParamView(v[p + "norm.weight"], v[p + "norm.bias"])
        self.uvqk = nn.Parameter(v[p + "uvqk"], requires_grad=False)
        self.pos_w = nn.Parameter(v[p + "pos_w"], requires_grad=False)
        if with_time:
            self.ts_w = nn.Parameter(v[p + "ts_w"], requires_grad=False)
        self.o = _ParamView(v[p + "o.weight"], v[p + "o.bias"])


def bucket_bytes(time_seq, seq, num_buckets):
    """``[B, T, T]`` uint8 on the device of ``seq``: the time bucket of every pair ``j <= i`` (``hiprec_hstu_buckets``)."""
    lib = _lib.load()
    dev = seq.device
    B, T = (int(n) for n in seq.shape)
    ts = index_tensor(time_seq, dev)
    if ts.numel() != B * T:
        raise ValueError(f"time_seq holds {ts.numel()} entries where [{B}, {T}] is expected")
    out = torch.zeros((B, T, T), dtype=torch.uint8, device=dev)
    stats = _new_stats(dev)
    _lib.check(lib.hiprec_hstu_buckets(_lib.ptr(ts), _lib.ptr(index_tensor(seq, dev)), B, T, int(num_buckets),
                                       _lib.ptr(out), _lib.ptr(stats), _lib.stream_ptr(dev)))
    raise_on_status(read_stats(stats).status)
    return out


def attention_stage(act, pos_w, ts_w, seq, buckets, heads, attention_dim, linear_dim, maxlen, dav=None):
    """The attention stage alone (``hiprec_hstu_attention``) on device tensors: ``act [B, T, 2 H dv + 2 H dqk]`` =
    ``u | v | q | k``, ``pos_w [2 maxlen - 1]``, ``ts_w [num_buckets + 1]`` with ``buckets [B, T, T]`` uint8 (both None:
    no time term), ``seq [B, T]``.  Returns ``av [B, T, H dv]`` and, with ``dav``, ``(av, dq, dk, dv, dpos_w, dts_w)``."""
    lib = _lib.load()
    dev = act.device
    B, T, Wt = (int(n) for n in act.shape)
    H, dq, dv = int(heads), int(attention_dim), int(linear_dim)
    nbk = 1 if ts_w is None else int(ts_w.numel()) - 1
    need = lib.hiprec_hstu_attention_scratch_floats(B, T, H, nbk)
    if need < 0 or Wt != 2 * H * (dq + dv) or pos_w.numel() != 2 * int(maxlen) - 1 or (ts_w is None) != (buckets is None):
        raise ValueError("attention_stage: act [B, T <= maxlen, 2 H dv + 2 H dqk], pos_w [2 maxlen - 1], ts_w with buckets")
    act, pos_w = act.contiguous().float(), pos_w.contiguous().float()
    seq_t = index_tensor(seq, dev)
    av = torch.empty((B, T, H * dv), dtype=torch.float32, device=dev)
    opt = lambda t: None if t is None else _lib.ptr(t)      # noqa: E731
    dact = dpos = dts = scratch = None
    if dav is not None:
        dav = dav.contiguous().float()
        dact, dpos = torch.zeros_like(act), torch.zeros_like(pos_w)
        dts = None if ts_w is None else torch.zeros_like(ts_w, dtype=torch.float32)
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
    if ts_w is not None:
        ts_w, buckets = ts_w.contiguous().float(), buckets.contiguous()
    _lib.check(lib.hiprec_hstu_attention(
        _lib.ptr(act), _lib.ptr(pos_w), opt(ts_w), _lib.ptr(seq_t), opt(buckets), opt(dav), B, T, H, dq, dv, int(maxlen),
        nbk, _lib.ptr(av), opt(dact), opt(dpos), opt(dts), opt(scratch), need if dav is not None else 0,
        _lib.stream_ptr(dev)))
    if dav is None:
        return av
    du, dvv, dqq, dkk = dact.split([H * dv, H * dv, H * dq, H * dq], dim=-1)
    return av, dqq, dkk, dvv, dpos, dts


class HSTU(_SeqModel):
    """Flat buffer in ``state_dict()`` order (``spec``).  Normal(0, 0.02) ``uvqk``, ``pos_w`` and ``ts_w``, Xavier-uniform
    ``o.weight``, truncated-normal(0, 0.02) tables, zero biases, unit LayerNorm weights; the padding row is zero."""

    _WORKSPACE_BYTES, _PARAM_FLOATS = "hiprec_hstu_workspace_bytes", "hiprec_hstu_param_floats"

    def __init__(self, config):
        super().__init__()
        self._configure(config)
        v = self._build(spec(self.item_num, self.maxlen, self.hidden_units, self.num_blocks, self.num_heads,
                             self.attention_dim, self.linear_dim, self.num_buckets, self.rel_bias))
        for name, view in v.items():
            if name.endswith(("uvqk", "pos_w", "ts_w")):
                view.normal_(0.0, 0.02)
            elif name.endswith("o.weight"):
                nn.init.xavier_uniform_(view)
            elif name.endswith("emb.weight"):
                nn.init.trunc_normal_(view, std=0.02)
            elif name.endswith("norm.weight"):
                view.fill_(1.0)
        v["item_emb.weight"][0].zero_()
        self.item_emb = _ParamView(v["item_emb.weight"])
        self.pos_emb = _ParamView(v["pos_emb.weight"])
        self.blocks = nn.ModuleList(_BlockParams(v, b, self.rel_bias == "pos_time") for b in range(self.num_blocks))
        self.last_norm = _ParamView(v["last_norm.weight"], v["last_norm.bias"])

    def _configure(self, config):
        """The model's own keys; the head widths do not depend on ``emb_dim``.  The limits are csrc/hstu.hip's."""
        self.config = config
        self.user_num = config.get("n_users")
        self.item_num = int(config["n_items"])
        self.hidden_units = int(config["emb_dim"])
        self.maxlen = int(config["maxlen"])
        self.num_blocks = int(config["num_blocks"])
        self.num_heads = int(config["num_heads"])
        self.attention_dim = int(config["attention_dim"])
        self.linear_dim = int(config["linear_dim"])
        self.num_buckets = int(config.get("num_buckets", 128))
        self.rel_bias = config.get("rel_bias", "pos_time")
        self.dropout_rate = float(config.get("dropout_rate", 0.0))
        self.batch_size = config.get("batch_size")
        self.l2_emb = float(config.get("l2_emb", 0.0))
        D, H = self.hidden_units, self.num_heads
        if not 0.0 <= self.dropout_rate < 1.0:
            raise ValueError("dropout_rate must be in [0, 1)")
        if D % 16 or not 16 <= D <= MAX_DIM:
            raise ValueError(f"emb_dim must be a multiple of 16 in 16..{MAX_DIM}, got {D}")
        if not 1 <= self.maxlen <= MAX_LEN:
            raise ValueError(f"maxlen must be in 1..{MAX_LEN}, got {self.maxlen}")
        if not 1 <= self.num_blocks <= MAX_BLOCKS:
            raise ValueError(f"num_blocks must be in 1..{MAX_BLOCKS}, got {self.num_blocks}")
        if self.attention_dim not in HEAD_WIDTHS or self.linear_dim not in HEAD_WIDTHS:
            raise ValueError(f"attention_dim and linear_dim must be in {HEAD_WIDTHS}, got {self.attention_dim} and "
                             f"{self.linear_dim}")
        if H < 1 or H * self.attention_dim > MAX_DIM or H * self.linear_dim > MAX_DIM:
            raise ValueError(f"num_heads * attention_dim and num_heads * linear_dim must be in 1..{MAX_DIM}, got num_heads {H}")
        if not 1 <= self.num_buckets <= MAX_BUCKETS:
            raise ValueError(f"num_buckets must be in 1..{MAX_BUCKETS}, got {self.num_buckets}")
        if self.rel_bias not in REL_BIAS:
            raise ValueError(f"rel_bias must be one of {sorted(REL_BIAS)}, got {self.rel_bias!r}")
        self.shape = _lib.HstuShape(self.item_num, D, H, self.attention_dim, self.linear_dim, self.maxlen, self.num_blocks,
                                    self.num_buckets, REL_BIAS[self.rel_bias])
        lib = _lib.load()
        if lib.hiprec_hstu_param_floats(ctypes.byref(self.shape)) < 0:      # n_items: the library's text
            raise ValueError((lib.hiprec_last_error() or b"beyond the library's limits").decode())
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def padded(self, ids, B, L, what):
        """``[B, L]`` ids or time stamps as a flat int64 device tensor ``[B * maxlen]``, left-padded with 0."""
        t = index_tensor(ids, self._flat.device)
        if t.numel() != B * L:
            raise ValueError(f"{what} holds {t.numel()} entries where [{B}, {L}] is expected")
        if L < self.maxlen:
            t = torch.nn.functional.pad(t.view(B, L), (self.maxlen - L, 0)).reshape(-1).contiguous()
        return t

    def sequences(self, seqs, time_seq=None):
        """``(seq, time_seq or None, B, maxlen)`` as flat int64 device tensors, left-padded with 0 to ``maxlen``."""
        _, B, L = super().sequences(seqs)
        if self.rel_bias == "pos_time" and time_seq is None:
            raise ValueError("rel_bias 'pos_time' needs time_seq next to the sequences")
        ts = self.padded(time_seq, B, L, "time_seq") if self.rel_bias == "pos_time" else None
        return self.padded(seqs, B, L, "seq"), ts, B, self.maxlen

    def all_feats(self, seqs, time_seq=None):
        """The eval forward: ``f`` at every position, ``[B, maxlen, D]`` on the device."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, ts_t, B, T = self.sequences(seqs, time_seq)
        stats = self._device_stats()
        out = torch.empty((B, T, self.hidden_units), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, T)
        _lib.check(lib.hiprec_hstu_feats(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(seq_t),
                                         None if ts_t is None else _lib.ptr(ts_t), B, T, _lib.ptr(out), _lib.ptr(stats),
                                         _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def feats(self, seqs, time_seq=None):
        """``f`` at the last position of every sequence, ``[B, D]`` on the device."""
        return self.all_feats(seqs, time_seq)[:, -1, :].contiguous()

    def predict(self, seqs, item_indices, time_seq=None):
        """``[B, K]`` scores of ``f`` against the rows of ``item_indices`` (1-D, ids in ``0 .. n_items``)."""
        return self._predict_from_feats(self.all_feats(seqs, time_seq), item_indices)

    def attention_stage(self, act, block, seq, buckets=None, dav=None):
        """``attention_stage`` with block ``block``'s bias weights and this model's widths."""
        blk = self.blocks[block]
        return attention_stage(act, blk.pos_w.data, blk.ts_w.data if self.rel_bias == "pos_time" else None, seq, buckets,
                               self.num_heads, self.attention_dim, self.linear_dim, self.maxlen, dav)


class HSTUEngine(_SeqEngine):
    """``train_single_batch((u, seq, time_seq, pos, neg)) -> float``, ``backward_only``, ``train_an_epoch(sampler,
    epoch_id)``, ``predict``, ``recommend_next``; checkpoints through the flat-model base."""

    _N_FIXED_MASKS, _MASK_NAMES = 1, "embedding, then per block the gated attention output"

    def __init__(self, config):
        self.config = config
        m = config["model"]
        if m.setdefault("dropout_rng", "device") != "device":
            raise ValueError("HSTU draws its dropout masks on the device: dropout_rng must be 'device'")
        self.model = HSTU(m)
        self.num_batch = max(1, int(m["n_users"]) // int(m["batch_size"])) if "n_users" in m and "batch_size" in m else 1
        self._dropout_step = 0
        super(HSTUEngine, self).__init__(config)

    def _mask_shapes(self, B, T):
        m = self.model
        return [(B * T, m.hidden_units)] + [(B * T, m.num_heads * m.linear_dim)] * m.num_blocks

    def _enqueue_grad(self, batch_data, keep_masks=None):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        timed = m.rel_bias == "pos_time"
        if len(batch_data) != (5 if timed else 4):
            raise ValueError("an HSTU batch is (u, seq, time_seq, pos, neg), or (u, seq, pos, neg) with rel_bias 'pos'")
        seq, pos, neg = batch_data[1], batch_data[-2], batch_data[-1]
        L = int(np.shape(seq)[1]) if np.ndim(seq) == 2 else 0
        seq_t, ts_t, B, T = m.sequences(seq, batch_data[2] if timed else None)
        pos_t, neg_t = m.padded(pos, B, L, "pos"), m.padded(neg, B, L, "neg")
        keep_arr = self._keep_array(B, T, keep_masks)
        ks = 1.0 / (1.0 - m.dropout_rate)
        ws = m.workspace(lib, B, T)
        l2 = m.l2_emb if self._dp_rank == 0 else 0.0
        _lib.check(lib.hiprec_hstu_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t),
            None if ts_t is None else _lib.ptr(ts_t), _lib.ptr(pos_t), _lib.ptr(neg_t), B, T, l2, keep_arr, ks, None,
            _lib.ptr(self._stats), _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)))

    def train_an_epoch(self, sampler, epoch_id):
        """``n_users // batch_size`` calls of ``sampler.next_batch()``: ``data.TimeSequenceSampler``'s 6-tuple (its
        ``time_matrix`` is ignored), or ``data.SequenceSampler``'s 4-tuple with ``rel_bias="pos"``."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self.model.train()
        total_loss = 0.0
        for _ in range(self.num_batch):
            b = sampler.next_batch()
            batch = (b[0], b[1], b[2], b[-2], b[-1]) if self.model.rel_bias == "pos_time" else (b[0], b[1], b[-2], b[-1])
            total_loss += self.train_single_batch(tuple(np.array(a) for a in batch))
        print("[Training Epoch {}], Loss {}".format(epoch_id, total_loss))
        self.writer.add_scalar("model/loss", total_loss, epoch_id)
        return total_loss

    # ---- inference ---------------------------------------------------------------------------------------------
    def predict(self, seqs, item_indices, time_seq=None):
        """Eval-mode scores ``[B, K]`` of the candidate list ``item_indices [K]`` for every sequence."""
        self.model.eval()
        return self.model.predict(seqs, item_indices, time_seq)

    def recommend_next(self, seqs, k, seen=None, time_seq=None):
        """The ``k`` best next items for every sequence of ``seqs [n, L]``: ``f`` at the last position against
        ``item_emb.weight[1:]`` through ``recommend.topk_factors``; the padding id is never returned.  ``seen`` as in
        ``SASRecEngine.recommend_next``.  Returns ``(items [n, k] int64, scores [n, k] fp32)`` on the device."""
        self.model.eval()
        return self._recommend_from_feats(self.model.all_feats(seqs, time_seq), k, seen)
