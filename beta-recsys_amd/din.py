"""``DIN`` / ``DINEngine``: the Deep Interest Network (Zhou, Zhu, Song, Fan, Zhu, Ma, Yan, Jin, Li and Gai, "Deep Interest
Network for Click-Through Rate Prediction", KDD 2018) on libhiprec.so: the ranking stage, where the history is re-read for
every candidate.

There is no counterpart in the reference; the paper and ``tests/din_torch.py`` (a restatement in plain torch ops with
autograd, in the naive concatenated form) are the specification, ``include/hiprec.h`` states the contract:

* items are ``1 .. n_items`` and 0 is padding (``item_emb.weight`` row 0 is zero and stays zero); a batch is
  ``(seq [B, L <= maxlen], cand [B, C], label [B, C])``; ``seq`` is left-padded with 0 to ``maxlen``; ``cand == 0`` marks a
  dead slot: no loss, no gradient, logit 0;
* the activation unit scores every (history item, candidate) pair: ``a_t = att.2(act(att.1(act(att.0([q, e_t, q - e_t,
  q * e_t]))))) / sqrt(D)``, 0 at padding, no softmax; ``pooled = sum_t a_t e_t``; the tower reads ``[pooled, q, pooled * q]``
  through Linear + Dice (or PReLU) layers to one logit; the loss is BCE-with-logits, the mean over the live candidates.

Config keys under ``config["model"]``: ``n_items emb_dim maxlen batch_size optimizer lr`` and, optional, ``att_hidden``
([80, 40]), ``dnn_hidden`` ([200, 80]), ``att_activation`` (``sigmoid`` | ``prelu``), ``dnn_activation`` (``dice`` |
``prelu``).  Not built: ``att_softmax``, Dice inside the activation unit, a ranking of the whole catalogue (the score of an
item depends on the item through the unit, so it is no dot product against a user vector).

Everything runs in ``csrc/din.hip`` (the Linear layers and the two shared first-layer terms through the grouped GEMM of
``csrc/ncf.hip``).  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor

_ATT_ACT = {"sigmoid": 0, "prelu": 1}
_DNN_ACT = {"dice": 0, "prelu": 1}


class _Layer(nn.Module):
    """``weight``, ``bias`` and (but for a last layer) ``alpha`` as views of the flat buffer."""

    def __init__(self, weight, bias, alpha=None):
        super().__init__()
        self.weight = Parameter(weight, requires_grad=False)
        self.bias = Parameter(bias, requires_grad=False)
        if alpha is not None:
            self.alpha = Parameter(alpha, requires_grad=False)


class _RankingModel(_FlatModel):
    """What the ranking models share: Dice's running buffers beside the flat buffer, ``seq`` / ``cand`` as device tensors,
    ``predict``.  A subclass builds ``dnn`` / ``dnn_hidden`` / ``dnn_activation`` and defines ``forward(seqs, cand)``."""

    # ---- Dice's running buffers: a second flat buffer, [running_mean, running_var] per tower layer ----------------------------
    def _bind_running(self, flat):
        self._bn = flat
        at = 0
        for layer, w in zip(self.dnn, self.dnn_hidden):
            if self.dnn_activation == "dice":
                layer.register_buffer("running_mean", flat[at:at + w])
                layer.register_buffer("running_var", flat[at + w:at + 2 * w])
            at += 2 * w

    def _apply(self, fn, recurse=True):
        super()._apply(fn)
        moved = fn(self._bn)
        if moved is not self._bn:
            self._bind_running(moved.contiguous())
        return self

    def sequences(self, seqs):
        """``[B, L <= maxlen]`` ids as ``(flat int64 device tensor [B * maxlen], B)``, left-padded with 0."""
        shape = tuple(seqs.shape) if torch.is_tensor(seqs) else np.asarray(seqs).shape
        if len(shape) != 2 or shape[0] < 1 or shape[1] < 1:
            raise ValueError("sequences must be [batch >= 1, length >= 1]")
        B, L, T = int(shape[0]), int(shape[1]), self.maxlen
        if L > T:
            raise ValueError(f"sequence length {L} exceeds maxlen {T}")
        flat = index_tensor(seqs, self._flat.device)
        if L < T:
            flat = torch.nn.functional.pad(flat.view(B, L), (T - L, 0)).reshape(-1).contiguous()
        return flat, B

    def candidates(self, cand, B):
        """``[B, C >= 1]`` ids as ``(flat int64 device tensor, C)``."""
        shape = tuple(cand.shape) if torch.is_tensor(cand) else np.asarray(cand).shape
        if len(shape) != 2 or shape[0] != B or shape[1] < 1:
            raise ValueError(f"candidates must be [{B}, n >= 1]: a list for every sequence")
        return index_tensor(cand, self._flat.device), int(shape[1])

    def predict(self, seqs, cand):
        return self.forward(seqs, cand)


class DIN(_RankingModel):
    """Flat buffer in ``state_dict()`` order: ``item_emb.weight``, ``att.{0,1}.{weight,bias,alpha}``, ``att.2.{weight,bias}``,
    ``dnn.l.{weight,bias,alpha}``, ``out.{weight,bias}``; with ``dice`` every ``dnn.l`` also holds the buffers
    ``running_mean`` / ``running_var`` (views of a second flat buffer).  The unit's alphas are read under ``prelu`` only."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.item_num = int(config["n_items"])
        self.hidden_units = D = int(config["emb_dim"])
        self.maxlen = int(config["maxlen"])
        att = [int(h) for h in (config["att_hidden"] if "att_hidden" in config else (80, 40))]
        dnn = [int(h) for h in (config["dnn_hidden"] if "dnn_hidden" in config else (200, 80))]
        self.att_activation = config["att_activation"] if "att_activation" in config else "sigmoid"
        self.dnn_activation = config["dnn_activation"] if "dnn_activation" in config else "dice"
        if len(att) != 2:
            raise ValueError("att_hidden takes exactly two widths")
        if not 1 <= len(dnn) <= 3:
            raise ValueError("dnn_hidden takes one to three widths")
        if self.att_activation not in _ATT_ACT or self.dnn_activation not in _DNN_ACT:
            raise ValueError("att_activation is 'sigmoid' or 'prelu', dnn_activation 'dice' or 'prelu'")
        self.att_hidden, self.dnn_hidden = att, dnn
        self.batch_size = config["batch_size"] if "batch_size" in config else None
        self.shape = _lib.DinShape(self.item_num, D, self.maxlen, att[0], att[1], _ATT_ACT[self.att_activation],
                                   _DNN_ACT[self.dnn_activation], len(dnn), (ctypes.c_int32 * 3)(*dnn))
        lib = _lib.load()
        if lib.hiprec_din_param_floats(ctypes.byref(self.shape)) < 0:
            raise ValueError((lib.hiprec_last_error() or b"beyond the library's limits").decode())
        spec = [("item_emb.weight", (self.item_num + 1, D)),
                ("att.0.weight", (att[0], 4 * D)), ("att.0.bias", (att[0],)), ("att.0.alpha", (att[0],)),
                ("att.1.weight", (att[1], att[0])), ("att.1.bias", (att[1],)), ("att.1.alpha", (att[1],)),
                ("att.2.weight", (1, att[1])), ("att.2.bias", (1,))]
        fan_in = 3 * D
        for l, w in enumerate(dnn):
            spec += [(f"dnn.{l}.weight", (w, fan_in)), (f"dnn.{l}.bias", (w,)), (f"dnn.{l}.alpha", (w,))]
            fan_in = w
        spec += [("out.weight", (1, fan_in)), ("out.bias", (1,))]
        v = self._build(spec)
        with torch.no_grad():
            for name, t in v.items():
                if name.endswith(".weight"):      # nn.Linear's own bound; the biases stay 0
                    t.uniform_(-1.0, 1.0).mul_(t.shape[-1] ** -0.5)
                elif name.endswith(".alpha"):     # Dice's alpha starts at 0, PReLU's at torch's 0.25
                    t.fill_(0.25 if (self.att_activation if name.startswith("att") else self.dnn_activation) == "prelu"
                            else 0.0)
            v["item_emb.weight"].normal_(0.0, 0.1)
            v["item_emb.weight"][0].zero_()
        self.item_emb = _ParamView(v["item_emb.weight"])
        self.att = nn.ModuleList([_Layer(v["att.0.weight"], v["att.0.bias"], v["att.0.alpha"]),
                                  _Layer(v["att.1.weight"], v["att.1.bias"], v["att.1.alpha"]),
                                  _Layer(v["att.2.weight"], v["att.2.bias"])])
        self.dnn = nn.ModuleList([_Layer(v[f"dnn.{l}.weight"], v[f"dnn.{l}.bias"], v[f"dnn.{l}.alpha"])
                                  for l in range(len(dnn))])
        self.out = _Layer(v["out.weight"], v["out.bias"])
        self._bind_running(torch.cat([torch.cat([torch.zeros(w), torch.ones(w)]) for w in dnn]))
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, n_cand, train):
        need = lib.hiprec_din_workspace_bytes(ctypes.byref(self.shape), int(batch), int(n_cand), int(train))
        if need == 0:
            raise ValueError(f"unsupported call of {batch} sequences with {n_cand} candidates (batch x maxlen and batch x "
                             f"candidates within 2^24)")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def tiles(self):
        """The kernel's tile constants for this shape, as ``hiprec_din_tiles`` states them."""
        out = (ctypes.c_int32 * 7)()
        _lib.check(_lib.load().hiprec_din_tiles(ctypes.byref(self.shape), out))
        return dict(zip(("tile", "chunk_fwd", "chunk_bwd", "slice", "slabs", "resident_fwd", "resident_bwd"), out))

    def forward(self, seqs, cand):
        """Logits ``[B, C]`` of the candidates (0 in dead slots); Dice reads its running statistics."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, B = self.sequences(seqs)
        cand_t, C = self.candidates(cand, B)
        stats = self._device_stats()
        out = torch.empty((B, C), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, C, False)
        _lib.check(lib.hiprec_din_grad(ctypes.byref(self.shape), _lib.ptr(self._flat), None, _lib.ptr(self._bn), 0,
                                       _lib.ptr(seq_t), _lib.ptr(cand_t), None, B, C, _lib.ptr(out), _lib.ptr(stats), None, 0,
                                       _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def attention_stage(self, e, q, mask, dpooled=None):
        """The activation unit and the pooling alone on explicit rows: ``e [B, maxlen, D]`` stands where ``item_emb[seq]``
        does, ``q [B, C, D]`` where ``item_emb[cand]`` does, ``mask [B, maxlen]`` marks the live slots (any pattern).
        Returns ``(pooled [B, C, D], a [B, C, maxlen])``; with ``dpooled [B, C, D]`` also the stage's backward:
        ``(pooled, a, grads of the unit's parameters by name, de, dq)``."""
        lib = self._require_hip()
        dev = self._flat.device
        B, T, D = (int(n) for n in e.shape)
        C = int(q.shape[1])
        if T != self.maxlen or D != self.hidden_units or tuple(mask.shape) != (B, T) or tuple(q.shape) != (B, C, D):
            raise ValueError(f"attention_stage takes e [B, {self.maxlen}, {self.hidden_units}], q [B, C, {self.hidden_units}] "
                             f"and mask [B, {self.maxlen}]")
        rows, qs = (t.to(dev, torch.float32).contiguous() for t in (e, q))
        live = (torch.as_tensor(mask) != 0).to(dev, torch.uint8).contiguous()
        pooled = torch.empty((B, C, D), dtype=torch.float32, device=dev)
        a = torch.empty((B, C, T), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, C, dpooled is not None)
        g = de = dq = None
        if dpooled is not None:
            dpooled = dpooled.to(dev, torch.float32).contiguous()
            lo, hi = self.offset_of("att.0.weight"), self.offset_of("dnn.0.weight")
            g, de, dq = torch.zeros(hi - lo, device=dev), torch.empty_like(rows), torch.empty_like(qs)
        _lib.check(lib.hiprec_din_attention(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(rows), _lib.ptr(qs),
                                            _lib.ptr(live), B, C, _lib.ptr(pooled), _lib.ptr(a), _lib.ptr(dpooled), _lib.ptr(g),
                                            _lib.ptr(de), _lib.ptr(dq), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        if dpooled is None:
            return pooled, a
        grads = {n: g[self.offset_of(n) - lo:self.offset_of(n) - lo + int(np.prod(s))].view(*s)
                 for n, s in self._spec if n.startswith("att.")}
        return pooled, a, grads, de, dq


class _RankingEngine(FlatModelEngine):
    """What the ranking engines share: the step around a subclass's ``_enqueue_grad``, the epoch loop, ``predict`` and
    ``rerank``."""

    def __init__(self, config, model):
        self.config = config
        self.model = model
        self.last_logits = None
        super().__init__(config)
        self._n_batches = 0
        self._update_running = True

    def train_single_batch(self, batch_data, ratings=None):
        """One step on the model's batch: the loss (the mean over the live candidates).  Moves Dice's running buffers."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_grad(batch_data)
        self._enqueue_opt()
        return self._sync_stats().loss

    def backward_only(self, batch_data):
        """``(loss, grads)`` without the optimizer step; Dice's running buffers stay as they are."""
        self._update_running = False
        try:
            return super().backward_only(batch_data)
        finally:
            self._update_running = True

    def _epoch_step(self, batch):
        self._n_batches += 1
        self._enqueue_step(batch)

    def train_an_epoch(self, train_loader, epoch_id):
        """Every batch of the loader enqueued back to back with ONE host sync at the end; returns
        the mean of the per-step losses and writes it to the writer."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._n_batches = 0
        st = self._run_epoch(train_loader)
        mean_loss = st.loss_sum / max(self._n_batches, 1)
        print("[Training Epoch {}], Loss {:.6f}".format(epoch_id, mean_loss))
        self.writer.add_scalar("model/loss", mean_loss, epoch_id)
        return mean_loss

    # ---- inference ---------------------------------------------------------------------------------------------
    def predict(self, seqs, cand):
        """Eval-mode logits ``[B, C]`` of every sequence's own candidate list (0 in dead slots)."""
        self.model.eval()
        return self.model.predict(seqs, cand)

    def rerank(self, seqs, cand, k):
        """The ``k`` best live candidates of every row by ``predict``: ``(items [B, k] int64, logits [B, k])``, best first,
        ``-1`` / ``-inf`` where a row has fewer than ``k`` live candidates."""
        logits = self.predict(seqs, cand)
        ids = index_tensor(cand, logits.device).view(logits.shape)
        if not 1 <= int(k) <= logits.shape[1]:
            raise ValueError(f"k must be in 1 .. {logits.shape[1]}")
        top, at = torch.where(ids != 0, logits, torch.full_like(logits, -float("inf"))).topk(int(k), dim=1)
        items = torch.gather(ids, 1, at)
        return torch.where(torch.isinf(top), torch.full_like(items, -1), items), top


class DINEngine(_RankingEngine):
    """``train_single_batch((seq, cand, label)) -> float``, ``backward_only``, ``train_an_epoch(loader, epoch_id)``,
    ``predict``, ``rerank``; optimizers and checkpoints through the flat-model base."""

    def __init__(self, config):
        super().__init__(config, DIN(config["model"]))

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_din_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat DIN buffer is not laid out as libhiprec.so expects; rebuild the library")

    # ---- the step ----------------------------------------------------------------------------------------------
    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 3:
            raise ValueError("a DIN batch is (seq [B, L], cand [B, C], label [B, C])")
        seq, cand, label = batch_data
        seq_t, B = m.sequences(seq)
        cand_t, C = m.candidates(cand, B)
        lab_t = torch.as_tensor(np.asarray(label) if not torch.is_tensor(label) else label).to(dev, torch.float32)
        lab_t = lab_t.reshape(-1).contiguous()
        if lab_t.numel() != B * C:
            raise ValueError(f"label must be [{B}, {C}]: one for every candidate")
        self.last_logits = torch.empty((B, C), dtype=torch.float32, device=dev)
        ws = m.workspace(lib, B, C, True)
        _lib.check(lib.hiprec_din_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(m._bn), int(self._update_running),
            _lib.ptr(seq_t), _lib.ptr(cand_t), _lib.ptr(lab_t), B, C, _lib.ptr(self.last_logits), _lib.ptr(self._stats),
            _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
