"""``ETA`` / ``ETAEngine``: End-to-end Target Attention (Chen, Pei, Lv, Li, Ge and Ou, "End-to-End User Behavior Retrieval in
Click-Through Rate Prediction Model", 2021) on libhiprec.so: the ranking model for histories of thousands of events.  Every
(sequence, candidate) pair retrieves ``top_k`` positions by the Hamming distance between SimHash fingerprints and a multi-head
target attention reads only those; after the retrieval nothing in the step depends on the length of the history.

There is no counterpart in the reference; ``tests/eta_torch.py`` (a restatement in plain torch ops with autograd) is the
specification, ``include/hiprec.h`` states the contract:

* ids, ``seq`` (left-padded to ``maxlen``), ``cand`` and ``label`` as DIN's; ``data.CandidateLoader`` serves the batches;
* ``hash.weight [hash_bits, D]`` is a buffer drawn N(0, 1) from ``hash_seed``: in ``state_dict()``, never trained.  Bit ``j`` of
  ``code(x)`` is 1 iff ``hash.weight[j] . x >= 0``; the selection of a pair is the ``top_k`` live positions with the smallest
  ``(popcount(code(q) ^ code(e_t)), -t)``, ascending in ``t``;
* ``Qp = att.q(q)``, ``Kp = att.k(e)``, ``Vp = att.v(e)``; per head ``softmax_j(<Qp_h, Kp_h[sel_j]> / sqrt(dh))`` over the live
  slots weighs ``Vp_h[sel_j]``; ``v = att.o(o)``; the tower reads ``[v, q, v * q]``; BCE-with-logits over the live candidates.

Config keys under ``config["model"]``: ``n_items emb_dim maxlen batch_size optimizer lr`` and, optional, ``hash_bits`` (64),
``top_k`` (48), ``num_heads`` (4), ``hash_seed`` (0), ``dnn_hidden`` ([200, 80]), ``dnn_activation`` (``dice`` | ``prelu``).
Limits (``ValueError``): ``emb_dim`` a multiple of 16 in 16 .. 128, ``maxlen`` 1 .. 4096, ``hash_bits`` in {32, 64, 96, 128},
``top_k`` 1 .. 128, ``num_heads`` dividing ``emb_dim`` with at least 4 dimensions a head, ``batch x maxlen`` and ``batch x
candidates x top_k`` within 2^24.  Not built: a short-term DIN / DIEN branch beside the long one, SIM's category retrieval,
SDIM's bucket sum.

Everything runs in ``csrc/eta.hip`` (the projections through the grouped GEMM of ``csrc/ncf.hip``, the tower through
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


class _Linear(nn.Module):
    """``weight`` and ``bias`` of one projection as views of the flat buffer."""

    def __init__(self, weight, bias):
        super().__init__()
        self.weight = Parameter(weight, requires_grad=False)
        self.bias = Parameter(bias, requires_grad=False)


class _Hash(nn.Module):
    """``weight``: the hash vectors, a buffer beside the flat one."""

    def __init__(self, weight):
        super().__init__()
        self.register_buffer("weight", weight)


class ETA(_RankingModel):
    """Flat buffer in ``state_dict()`` order: ``item_emb.weight``, ``att.{q,k,v,o}.{weight,bias}``, ``dnn.l.{weight,bias,
    alpha}``, ``out.{weight,bias}``; Dice's buffers as DIN's; ``hash.weight`` is a buffer outside the optimizer's sweep."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.item_num = int(config["n_items"])
        self.hidden_units = D = int(config["emb_dim"])
        self.maxlen = int(config["maxlen"])
        self.hash_bits = int(config["hash_bits"]) if "hash_bits" in config else 64
        self.top_k = int(config["top_k"]) if "top_k" in config else 48
        self.num_heads = int(config["num_heads"]) if "num_heads" in config else 4
        self.hash_seed = int(config["hash_seed"]) if "hash_seed" in config else 0
        dnn = [int(h) for h in (config["dnn_hidden"] if "dnn_hidden" in config else (200, 80))]
        self.dnn_activation = config["dnn_activation"] if "dnn_activation" in config else "dice"
        if not 1 <= len(dnn) <= 3:
            raise ValueError("dnn_hidden takes one to three widths")
        if self.dnn_activation not in _DNN_ACT:
            raise ValueError("dnn_activation is 'dice' or 'prelu'")
        self.dnn_hidden = dnn
        self.batch_size = config["batch_size"] if "batch_size" in config else None
        self.shape = _lib.EtaShape(self.item_num, D, self.maxlen, self.hash_bits, self.top_k, self.num_heads,
                                   _DNN_ACT[self.dnn_activation], len(dnn), (ctypes.c_int32 * 3)(*dnn))
        lib = _lib.load()
        if lib.hiprec_eta_param_floats(ctypes.byref(self.shape)) < 0:
            raise ValueError((lib.hiprec_last_error() or b"beyond the library's limits").decode())
        spec = [("item_emb.weight", (self.item_num + 1, D))]
        for p in "qkvo":
            spec += [(f"att.{p}.weight", (D, D)), (f"att.{p}.bias", (D,))]
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
                elif name.endswith(".alpha"):
                    t.fill_(0.25 if self.dnn_activation == "prelu" else 0.0)
            v["item_emb.weight"].normal_(0.0, 0.1)
            v["item_emb.weight"][0].zero_()
        self.item_emb = _ParamView(v["item_emb.weight"])
        self.att = nn.ModuleDict({p: _Linear(v[f"att.{p}.weight"], v[f"att.{p}.bias"]) for p in "qkvo"})
        self.dnn = nn.ModuleList([_Layer(v[f"dnn.{l}.weight"], v[f"dnn.{l}.bias"], v[f"dnn.{l}.alpha"])
                                  for l in range(len(dnn))])
        self.out = _Layer(v["out.weight"], v["out.bias"])
        self._bind_running(torch.cat([torch.cat([torch.zeros(w), torch.ones(w)]) for w in dnn]))
        self.hash = _Hash(torch.randn(self.hash_bits, D, generator=torch.Generator().manual_seed(self.hash_seed)))
        self._ws = None

    def _apply(self, fn, recurse=True):
        super()._apply(fn)
        moved = fn(self.hash.weight)
        if moved is not self.hash.weight:
            self.hash.weight = moved.contiguous()
        return self

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, n_cand, train):
        need = lib.hiprec_eta_workspace_bytes(ctypes.byref(self.shape), int(batch), int(n_cand), int(train))
        if need == 0:
            raise ValueError(f"unsupported call of {batch} sequences with {n_cand} candidates (batch x maxlen and batch x "
                             f"candidates x top_k within 2^24)")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def tiles(self, n_cand=1):
        """The kernels' tile constants for this shape at ``n_cand`` candidates, as ``hiprec_eta_tiles`` states them."""
        out = (ctypes.c_int32 * 6)()
        _lib.check(_lib.load().hiprec_eta_tiles(ctypes.byref(self.shape), int(n_cand), out))
        return dict(zip(("chunk", "words", "codes_in_lds", "rows_per_seq", "scan_waves", "slices"), out))

    def forward(self, seqs, cand):
        """Logits ``[B, C]`` of the candidates (0 in dead slots); Dice reads its running statistics."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, B = self.sequences(seqs)
        cand_t, C = self.candidates(cand, B)
        stats = self._device_stats()
        out = torch.empty((B, C), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, C, False)
        _lib.check(lib.hiprec_eta_grad(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(self.hash.weight), None,
                                       _lib.ptr(self._bn), 0, _lib.ptr(seq_t), _lib.ptr(cand_t), None, B, C, _lib.ptr(out),
                                       _lib.ptr(stats), None, 0, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def _stage_rows(self, e, q):
        B, T, D = (int(n) for n in e.shape)
        if T != self.maxlen or D != self.hidden_units or q.dim() != 3 or (int(q.shape[0]), int(q.shape[2])) != (B, D):
            raise ValueError(f"a stage takes e [B, {self.maxlen}, {self.hidden_units}] and q [B, C, {self.hidden_units}]")
        dev = self._flat.device
        return B, int(q.shape[1]), e.to(dev, torch.float32).contiguous(), q.to(dev, torch.float32).contiguous()

    def retrieve_stage(self, e, q, mask):
        """The retrieval alone on explicit rows: ``e [B, maxlen, D]`` stands where ``item_emb[seq]`` does, ``q [B, C, D]``
        where ``item_emb[cand]`` does, ``mask [B, maxlen]`` marks the live positions (any pattern).  Returns ``(codes_e [B,
        maxlen, hash_bits / 32], codes_q [B, C, hash_bits / 32], sel [B, C, top_k])`` as int32 tensors (the code words are the
        bit patterns)."""
        lib = self._require_hip()
        B, C, rows, qs = self._stage_rows(e, q)
        dev, T, W = self._flat.device, self.maxlen, self.hash_bits // 32
        if tuple(mask.shape) != (B, T):
            raise ValueError(f"retrieve_stage takes mask [B, {T}]")
        live = (torch.as_tensor(mask) != 0).to(dev, torch.uint8).contiguous()
        codes_e = torch.empty((B, T, W), dtype=torch.int32, device=dev)
        codes_q = torch.empty((B, C, W), dtype=torch.int32, device=dev)
        sel = torch.empty((B, C, self.top_k), dtype=torch.int32, device=dev)
        ws = self.workspace(lib, B, C, False)
        _lib.check(lib.hiprec_eta_retrieve(ctypes.byref(self.shape), _lib.ptr(self.hash.weight), _lib.ptr(rows), _lib.ptr(qs),
                                           _lib.ptr(live), B, C, _lib.ptr(codes_e), _lib.ptr(codes_q), _lib.ptr(sel),
                                           _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        return codes_e, codes_q, sel

    def attention_stage(self, e, q, sel, dv=None):
        """The target attention alone on explicit rows and an explicit ``sel [B, C, top_k]`` (every row strictly ascending, its ``-1``
        slots last; undefined for any other row, see ``include/hiprec.h``).  Returns ``v [B, C, D]``; with ``dv [B, C, D]`` also the stage's backward: ``(v, de, dq, gradients of
        att.* by name)``."""
        lib = self._require_hip()
        B, C, rows, qs = self._stage_rows(e, q)
        dev = self._flat.device
        if tuple(sel.shape) != (B, C, self.top_k):
            raise ValueError(f"attention_stage takes sel [B, C, {self.top_k}]")
        sel_t = torch.as_tensor(sel).to(dev, torch.int32).contiguous()
        v = torch.empty_like(qs)
        ws = self.workspace(lib, B, C, dv is not None)
        g = de = dq = None
        lo, hi = self.offset_of("att.q.weight"), self.offset_of("dnn.0.weight")
        if dv is not None:
            dv = dv.to(dev, torch.float32).contiguous()
            g, de, dq = torch.zeros(hi - lo, device=dev), torch.empty_like(rows), torch.empty_like(qs)
        _lib.check(lib.hiprec_eta_attention(ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(rows), _lib.ptr(qs),
                                            _lib.ptr(sel_t), B, C, _lib.ptr(v), _lib.ptr(dv), _lib.ptr(g), _lib.ptr(de),
                                            _lib.ptr(dq), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        if dv is None:
            return v
        grads = {n: g[self.offset_of(n) - lo:self.offset_of(n) - lo + int(np.prod(s))].view(*s)
                 for n, s in self._spec if n.startswith("att.")}
        return v, de, dq, grads


class ETAEngine(_RankingEngine):
    """``train_single_batch((seq, cand, label)) -> float``, ``backward_only``, ``train_an_epoch(loader, epoch_id)``
    (``data.CandidateLoader``), ``predict``, ``rerank``; optimizers and checkpoints through the flat-model base."""

    def __init__(self, config):
        super().__init__(config, ETA(config["model"]))

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_eta_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat ETA buffer is not laid out as libhiprec.so expects; rebuild the library")

    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 3:
            raise ValueError("an ETA batch is (seq [B, L], cand [B, C], label [B, C])")
        seq, cand, label = batch_data
        seq_t, B = m.sequences(seq)
        cand_t, C = m.candidates(cand, B)
        lab_t = torch.as_tensor(np.asarray(label) if not torch.is_tensor(label) else label).to(dev, torch.float32)
        lab_t = lab_t.reshape(-1).contiguous()
        if lab_t.numel() != B * C:
            raise ValueError(f"label must be [{B}, {C}]: one for every candidate")
        self.last_logits = torch.empty((B, C), dtype=torch.float32, device=dev)
        ws = m.workspace(lib, B, C, True)
        _lib.check(lib.hiprec_eta_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(m.hash.weight), _lib.ptr(self._g_flat), _lib.ptr(m._bn),
            int(self._update_running), _lib.ptr(seq_t), _lib.ptr(cand_t), _lib.ptr(lab_t), B, C, _lib.ptr(self.last_logits),
            _lib.ptr(self._stats), _lib.ptr(self._scratch), self._scratch.numel(), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)))
