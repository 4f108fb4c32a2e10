"""``DIEN`` / ``DIENEngine``: the Deep Interest Evolution Network (Zhou, Mou, Fan, Pi, Bian, Zhou, Zhu and Gai, "Deep
Interest Evolution Network for Click-Through Rate Prediction", AAAI 2019) on libhiprec.so: DIN's tower over two recurrent
layers in place of DIN's bag.

There is no counterpart in the reference; the paper and ``tests/dien_torch.py`` (a restatement in plain torch ops with
autograd, a Python loop over the positions) are the specification, ``include/hiprec.h`` states the contract:

* ids, ``seq`` (left-padded to ``maxlen``), ``cand`` and ``label`` as DIN's; a training batch is ``(seq, neg_seq, cand,
  label)`` with ``neg_seq [B, L]`` one sampled item per position (``data.EvolutionLoader``);
* the interest extractor is a GRU over ``item_emb[seq]`` (gate order ``r | u | n``, ``n = tanh(W_n x + r * (U_n h) + b_n)``,
  padding positions leave the state unchanged) supervised at every position by the inner-product auxiliary loss; the
  attention is ``softmax_t(h1[b, t] . (att.weight q))`` over the live positions; the interest evolution layer is an AUGRU (the
  update gate scaled by the attention) with one state per (sequence, candidate); the tower reads ``[hT, q, hT * q]``.

Config keys under ``config["model"]``: ``n_items emb_dim maxlen batch_size optimizer lr`` and, optional, ``dnn_hidden``
([200, 80]), ``dnn_activation`` (``dice`` | ``prelu``), ``aux_weight`` (1.0).  Both recurrent layers are ``emb_dim`` wide.
Limits (``ValueError``): ``emb_dim`` a multiple of 16 in 16 .. 128, ``maxlen`` 1 .. 256, one to three ``dnn_hidden`` widths in
1 .. 512, ``batch x maxlen`` and ``batch x candidates`` within 2^24 and, one limit beyond the workspace, a training batch within
``batch x candidates x maxlen <= 2^24`` (the saved rows are counted in 32 bits through the weight-gradient GEMMs).
Not built: the official code's MLP auxiliary net, DIN's activation unit as the attention, user and context fields.

Everything runs in ``csrc/dien.hip`` (the projections through the grouped GEMM of ``csrc/ncf.hip``, the tower through
``csrc/din.hip``).  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import _lib
from .din import _DNN_ACT, _Layer, _RankingEngine, _RankingModel
from .flat_engine import _ParamView


class _Recurrent(nn.Module):
    """``weight_ih``, ``weight_hh`` and ``bias`` of one recurrent layer as views of the flat buffer."""

    def __init__(self, weight_ih, weight_hh, bias):
        super().__init__()
        self.weight_ih = Parameter(weight_ih, requires_grad=False)
        self.weight_hh = Parameter(weight_hh, requires_grad=False)
        self.bias = Parameter(bias, requires_grad=False)


class DIEN(_RankingModel):
    """Flat buffer in ``state_dict()`` order: ``item_emb.weight``, ``extractor.{weight_ih,weight_hh,bias}``, ``att.weight``,
    ``evolve.{weight_ih,weight_hh,bias}``, ``dnn.l.{weight,bias,alpha}``, ``out.{weight,bias}``; Dice's buffers as DIN's."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.item_num = int(config["n_items"])
        self.hidden_units = D = int(config["emb_dim"])
        self.maxlen = int(config["maxlen"])
        dnn = [int(h) for h in (config["dnn_hidden"] if "dnn_hidden" in config else (200, 80))]
        self.dnn_activation = config["dnn_activation"] if "dnn_activation" in config else "dice"
        self.aux_weight = float(config["aux_weight"]) if "aux_weight" in config else 1.0
        if not 1 <= len(dnn) <= 3:
            raise ValueError("dnn_hidden takes one to three widths")
        if self.dnn_activation not in _DNN_ACT:
            raise ValueError("dnn_activation is 'dice' or 'prelu'")
        self.dnn_hidden = dnn
        self.batch_size = config["batch_size"] if "batch_size" in config else None
        self.shape = _lib.DienShape(self.item_num, D, self.maxlen, _DNN_ACT[self.dnn_activation], len(dnn),
                                    (ctypes.c_int32 * 3)(*dnn), self.aux_weight)
        lib = _lib.load()
        if lib.hiprec_dien_param_floats(ctypes.byref(self.shape)) < 0:
            raise ValueError((lib.hiprec_last_error() or b"beyond the library's limits").decode())
        spec = [("item_emb.weight", (self.item_num + 1, D))]
        for name in ("extractor", "evolve"):
            if name == "evolve":
                spec.append(("att.weight", (D, D)))
            spec += [(f"{name}.weight_ih", (3 * D, D)), (f"{name}.weight_hh", (3 * D, D)), (f"{name}.bias", (3 * D,))]
        fan_in = 3 * D
        for l, w in enumerate(dnn):
            spec += [(f"dnn.{l}.weight", (w, fan_in)), (f"dnn.{l}.bias", (w,)), (f"dnn.{l}.alpha", (w,))]
            fan_in = w
        spec += [("out.weight", (1, fan_in)), ("out.bias", (1,))]
        v = self._build(spec)
        with torch.no_grad():
            for name, t in v.items():
                if ".weight" in name:      # nn.Linear's / nn.GRU's own bound; the biases stay 0
                    t.uniform_(-1.0, 1.0).mul_(t.shape[-1] ** -0.5)
                elif name.endswith(".alpha"):
                    t.fill_(0.25 if self.dnn_activation == "prelu" else 0.0)
            v["item_emb.weight"].normal_(0.0, 0.1)
            v["item_emb.weight"][0].zero_()
        self.item_emb = _ParamView(v["item_emb.weight"])
        self.extractor = _Recurrent(*(v[f"extractor.{n}"] for n in ("weight_ih", "weight_hh", "bias")))
        self.att = _ParamView(v["att.weight"])
        self.evolve = _Recurrent(*(v[f"evolve.{n}"] for n in ("weight_ih", "weight_hh", "bias")))
        self.dnn = nn.ModuleList([_Layer(v[f"dnn.{l}.weight"], v[f"dnn.{l}.bias"], v[f"dnn.{l}.alpha"])
                                  for l in range(len(dnn))])
        self.out = _Layer(v["out.weight"], v["out.bias"])
        self._bind_running(torch.cat([torch.cat([torch.zeros(w), torch.ones(w)]) for w in dnn]))
        self._ws = None

    def workspace(self, lib, batch, n_cand, mode):
        """``mode``: 0 scoring, 1 training, 2 / 3 the evolution stage without / with its backward, 4 / 5 the extractor stage
        (``n_cand`` ignored).  A training call is bounded by ``batch x candidates x maxlen <= 2^24`` beside the workspace: the
        rows of the saved gates are counted in 32 bits through the weight-gradient GEMMs."""
        need = lib.hiprec_dien_workspace_bytes(ctypes.byref(self.shape), int(batch), int(n_cand), int(mode))
        if need == 0:
            raise ValueError(f"unsupported call of {batch} sequences with {n_cand} candidates (batch x maxlen and batch x "
                             f"candidates within 2^24; training: batch x candidates x maxlen within 2^24)")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def tiles(self, n_cand=1):
        """The kernels' tile constants for this shape at ``n_cand`` candidates, as ``hiprec_dien_tiles`` states them."""
        out = (ctypes.c_int32 * 8)()
        _lib.check(_lib.load().hiprec_dien_tiles(ctypes.byref(self.shape), int(n_cand), out))
        return dict(zip(("tile", "slots", "slabs", "slices", "resident_extract_fwd", "resident_evolve_fwd",
                         "resident_extract_bwd", "resident_evolve_bwd"), out))

    def forward(self, seqs, cand):
        """Logits ``[B, C]`` of the candidates (0 in dead slots); Dice reads its running statistics."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, B = self.sequences(seqs)
        cand_t, C = self.candidates(cand, B)
        stats = self._device_stats()
        out = torch.empty((B, C), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, C, 0)
        _lib.check(lib.hiprec_dien_score(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(self._bn), _lib.ptr(seq_t),
                                         _lib.ptr(cand_t), B, C, _lib.ptr(out), _lib.ptr(stats), _lib.ptr(ws), ws.numel(),
                                         _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def extract_stage(self, x, mask, dh1=None):
        """The interest extractor alone on explicit rows: ``x [B, maxlen, D]`` stands where ``item_emb[seq]`` does, ``mask
        [B, maxlen]`` marks the live positions (any pattern).  Returns ``h1 [B, maxlen, D]``, the state after every position
        (the carried state at a dead one); with ``dh1 [B, maxlen, D]``, which is read at the live positions only, also the
        stage's backward: ``(h1, dx, gradients of extractor.* by name)``.  The auxiliary loss is not part of it."""
        lib = self._require_hip()
        dev = self._flat.device
        B, T, D = (int(n) for n in x.shape)
        if T != self.maxlen or D != self.hidden_units or tuple(mask.shape) != (B, T):
            raise ValueError(f"extract_stage takes x [B, {self.maxlen}, {self.hidden_units}] and mask [B, {self.maxlen}]")
        rows = x.to(dev, torch.float32).contiguous()
        live = (torch.as_tensor(mask) != 0).to(dev, torch.uint8).contiguous()
        h1 = torch.empty_like(rows)
        ws = self.workspace(lib, B, 1, 5 if dh1 is not None else 4)
        g = dx = None
        lo, hi = self.offset_of("extractor.weight_ih"), self.offset_of("att.weight")
        if dh1 is not None:
            dh1 = dh1.to(dev, torch.float32).contiguous()
            g, dx = torch.zeros(hi - lo, device=dev), torch.empty_like(rows)
        _lib.check(lib.hiprec_dien_extract(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(rows), _lib.ptr(live), B,
                                           _lib.ptr(h1), _lib.ptr(dh1), _lib.ptr(g), _lib.ptr(dx), _lib.ptr(ws), ws.numel(),
                                           _lib.stream_ptr(dev)))
        if dh1 is None:
            return h1
        grads = {n: g[self.offset_of(n) - lo:self.offset_of(n) - lo + int(np.prod(s))].view(*s)
                 for n, s in self._spec if lo <= self.offset_of(n) < hi}
        return h1, dx, grads

    def evolve_stage(self, h1, q, mask, dhT=None):
        """The attention and the AUGRU alone on explicit rows: ``h1 [B, maxlen, D]`` stands where the extractor's states do,
        ``q [B, C, D]`` where ``item_emb[cand]`` does, ``mask [B, maxlen]`` marks the live positions (any pattern).  Returns
        ``(hT [B, C, D], a [B, C, maxlen])``; with ``dhT [B, C, D]`` also the stage's backward:
        ``(hT, a, dh1, dq, gradients of att.weight and evolve.* by name)``."""
        lib = self._require_hip()
        dev = self._flat.device
        B, T, D = (int(n) for n in h1.shape)
        C = int(q.shape[1])
        if T != self.maxlen or D != self.hidden_units or tuple(mask.shape) != (B, T) or tuple(q.shape) != (B, C, D):
            raise ValueError(f"evolve_stage takes h1 [B, {self.maxlen}, {self.hidden_units}], q [B, C, {self.hidden_units}] "
                             f"and mask [B, {self.maxlen}]")
        rows, qs = (t.to(dev, torch.float32).contiguous() for t in (h1, q))
        live = (torch.as_tensor(mask) != 0).to(dev, torch.uint8).contiguous()
        hT = torch.empty((B, C, D), dtype=torch.float32, device=dev)
        a = torch.empty((B, C, T), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, C, 3 if dhT is not None else 2)
        g = dh1 = dq = None
        lo, hi = self.offset_of("att.weight"), self.offset_of("dnn.0.weight")
        if dhT is not None:
            dhT = dhT.to(dev, torch.float32).contiguous()
            g, dh1, dq = torch.zeros(hi - lo, device=dev), torch.empty_like(rows), torch.empty_like(qs)
        _lib.check(lib.hiprec_dien_evolve(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(rows), _lib.ptr(qs),
                                          _lib.ptr(live), B, C, _lib.ptr(hT), _lib.ptr(a), _lib.ptr(dhT), _lib.ptr(g),
                                          _lib.ptr(dh1), _lib.ptr(dq), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        if dhT is None:
            return hT, a
        grads = {n: g[self.offset_of(n) - lo:self.offset_of(n) - lo + int(np.prod(s))].view(*s)
                 for n, s in self._spec if lo <= self.offset_of(n) < hi}
        return hT, a, dh1, dq, grads


class DIENEngine(_RankingEngine):
    """``train_single_batch((seq, neg_seq, cand, label)) -> float``, ``backward_only``, ``train_an_epoch(loader, epoch_id)``
    (``data.EvolutionLoader``), ``predict``, ``rerank``; optimizers and checkpoints through the flat-model base."""

    def __init__(self, config):
        super().__init__(config, DIEN(config["model"]))

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_dien_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat DIEN buffer is not laid out as libhiprec.so expects; rebuild the library")

    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 4:
            raise ValueError("a DIEN batch is (seq [B, L], neg_seq [B, L], cand [B, C], label [B, C])")
        seq, neg, cand, label = batch_data
        seq_t, B = m.sequences(seq)
        neg_t, Bn = m.sequences(neg)
        if Bn != B or tuple(np.shape(neg)) != tuple(np.shape(seq)):
            raise ValueError("neg_seq must have the shape of seq: one sampled item per position")
        cand_t, C = m.candidates(cand, B)
        lab_t = torch.as_tensor(np.asarray(label) if not torch.is_tensor(label) else label).to(dev, torch.float32)
        lab_t = lab_t.reshape(-1).contiguous()
        if lab_t.numel() != B * C:
            raise ValueError(f"label must be [{B}, {C}]: one for every candidate")
        self.last_logits = torch.empty((B, C), dtype=torch.float32, device=dev)
        ws = m.workspace(lib, B, C, 1)
        _lib.check(lib.hiprec_dien_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(m._bn), int(self._update_running),
            _lib.ptr(seq_t), _lib.ptr(neg_t), _lib.ptr(cand_t), _lib.ptr(lab_t), B, C, _lib.ptr(self.last_logits),
            _lib.ptr(self._stats), _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)))
