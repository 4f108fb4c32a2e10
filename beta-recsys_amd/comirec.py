"""``ComiRec`` / ``ComiRecEngine``: the multi-interest dynamic-routing sequence model ComiRec-DR (Cen, Zhang, Zou, Zhou, Yang
and Tang, "Controllable Multi-Interest Framework for Recommendation", KDD 2020; the capsule routing of MIND, Li et al., CIKM
2019) on libhiprec.so.

There is no counterpart in the reference; the papers and ``tests/comirec_torch.py`` (a restatement in plain torch ops with
autograd) are the specification, ``include/hiprec.h`` states the contract:

* items are ``1 .. n_items`` and 0 is padding (``item_emb.weight`` row 0 is zero and stays zero); a batch is
  ``(seq [B, L <= maxlen], target [B], samples [S])``; ``seq`` is left-padded with 0 to ``maxlen``;
* ``uh[k, t] = routing.weight[t, k] item_emb[seq[t]]``; ``routing_iters`` times ``c = softmax_k(b)`` (0 at padding),
  ``s[k] = sum_t c[k, t] uh[k, t]``, ``v[k] = squash(s[k])``, ``b[k, t] += <uh[k, t], v[k]>`` with ``uh`` a constant in every
  iteration but the last; the ``num_interest`` vectors ``v`` of the last iteration are the interests;
* training reads the interest nearest the target (hard readout) and a sampled softmax over the target and the ``S`` samples
  the batch shares, with a logQ shift once ``set_item_probs`` was called; a sample equal to a row's target is left out of that
  row; ``target == 0`` marks a row as unlabelled; the loss is the mean over the labelled rows;
* the score of an item is the best of its scores against the interests.

Config keys under ``config["model"]``: ``n_items emb_dim maxlen num_interest batch_size optimizer lr`` and, optional,
``routing_iters`` (3), ``n_users``.  Not built: ComiRec-SA, the soft readout, MIND's random routing initialisation and shared
bilinear map, the diversity-controlled aggregation, ``l2_emb``.

Everything runs in ``csrc/comirec.hip`` (the logits and their gradients through the grouped GEMM of ``csrc/ncf.hip``),
``recommend_next`` ranks the catalogue through ``csrc/topk.hip`` per interest and a merge kernel.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor

MAX_SAMPLE = 8192      # kCrMaxSample


class ComiRec(_FlatModel):
    """Flat buffer in ``state_dict()`` order: ``item_emb.weight [n_items + 1, D]``, ``routing.weight [T, K, D, D]``, both
    Normal(0, 1) as published, the padding row zero."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.item_num = int(config["n_items"])
        self.hidden_units = D = int(config["emb_dim"])
        self.maxlen = T = int(config["maxlen"])
        self.num_interest = K = int(config["num_interest"])
        self.routing_iters = int(config["routing_iters"]) if "routing_iters" in config else 3
        self.batch_size = config["batch_size"] if "batch_size" in config else None
        self.shape = _lib.ComirecShape(self.item_num, D, T, K, self.routing_iters)
        lib = _lib.load()
        if lib.hiprec_comirec_param_floats(ctypes.byref(self.shape)) < 0:
            raise ValueError((lib.hiprec_last_error() or b"beyond the library's limits").decode())
        v = self._build([("item_emb.weight", (self.item_num + 1, D)), ("routing.weight", (T, K, D, D))])
        with torch.no_grad():
            self._flat.normal_(0.0, 1.0)
            v["item_emb.weight"][0].zero_()
        self.item_emb = _ParamView(v["item_emb.weight"])
        self.routing = _ParamView(v["routing.weight"])
        self._ws = None

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, batch, n_sample):
        need = lib.hiprec_comirec_workspace_bytes(ctypes.byref(self.shape), int(batch), int(n_sample))
        if need == 0:
            raise ValueError(f"unsupported step of {batch} sequences and {n_sample} samples (batch x maxlen within 2^24, "
                             f"at most {MAX_SAMPLE} samples)")
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

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

    def interests(self, seqs):
        """The eval forward: the ``num_interest`` interest vectors of every sequence, ``[B, K, D]`` on the device."""
        lib = self._require_hip()
        dev = self._flat.device
        seq_t, B = self.sequences(seqs)
        stats = self._device_stats()
        out = torch.empty((B, self.num_interest, self.hidden_units), dtype=torch.float32, device=dev)
        ws = self.workspace(lib, B, 0)
        _lib.check(lib.hiprec_comirec_grad(ctypes.byref(self.shape), _lib.ptr(self._flat), None, _lib.ptr(seq_t), None, None,
                                           B, 0, None, _lib.ptr(out), None, _lib.ptr(stats), None, 0, _lib.ptr(ws),
                                           ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def forward(self, seqs):
        return self.interests(seqs)

    def predict(self, seqs, item_indices):
        """``[B, n]`` scores of the candidate list ``item_indices`` (1-D, ids in ``0 .. n_items``): for every candidate the
        best of its scores against the sequence's interests, through the exact-fp32 MFMA GEMM."""
        lib, dev = _lib.load(), self._flat.device
        if np.ndim(item_indices) != 1:
            raise ValueError("item_indices must be 1-D: one list of candidate items for every sequence")
        idx = index_tensor(item_indices, dev)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) > self.item_num):
            raise IndexError(f"item id outside [0, {self.item_num}]")
        v = self.interests(seqs)
        B, K, D = v.shape
        n = idx.numel()
        rows = self.item_emb.weight.data[idx].contiguous()
        logits = torch.empty((B * K, n), dtype=torch.float32, device=dev)
        if n:
            _lib.check(lib.hiprec_gemm_f32(0, B * K, n, D, _lib.ptr(v), D, _lib.ptr(rows), D, _lib.ptr(logits), n, None, 0,
                                           None, 0, _lib.stream_ptr(dev)))
        return logits.view(B, K, n).amax(1)

    def routing_stage(self, e_rows, mask):
        """Projection and routing alone on explicit rows: ``e_rows [B, maxlen, D]`` (device, fp32) stand where
        ``item_emb[seq]`` does, ``mask [B, maxlen]`` marks the live slots.  Returns ``(interests [B, K, D],
        c [B, K, maxlen])`` of the last iteration."""
        lib = self._require_hip()
        dev = self._flat.device
        B, T, D = (int(n) for n in e_rows.shape)
        K = self.num_interest
        if T != self.maxlen or D != self.hidden_units or tuple(mask.shape) != (B, T):
            raise ValueError(f"routing_stage takes e_rows [B, {self.maxlen}, {self.hidden_units}] and mask [B, {self.maxlen}]")
        rows = e_rows.to(dev, torch.float32).contiguous()
        live_in = (torch.as_tensor(mask) != 0).to(dev, torch.uint8).contiguous()
        ids = torch.arange(B * T, dtype=torch.int64, device=dev)
        uh = torch.empty((B, T, K, D), dtype=torch.float32, device=dev)
        live = torch.empty((B, T), dtype=torch.uint8, device=dev)
        stats = self._device_stats()
        _lib.check(lib.hiprec_comirec_project(_lib.ptr(self.routing.weight.data), _lib.ptr(rows), B * T, _lib.ptr(ids),
                                              _lib.ptr(live_in), B, T, K, D, _lib.ptr(uh), _lib.ptr(live), _lib.ptr(stats),
                                              _lib.stream_ptr(dev)))
        v = torch.empty((B, K, D), dtype=torch.float32, device=dev)
        c = torch.empty((B, K, T), dtype=torch.float32, device=dev)
        nsq = torch.empty((B, K), dtype=torch.float32, device=dev)
        _lib.check(lib.hiprec_comirec_route(_lib.ptr(uh), _lib.ptr(live), B, T, K, D, self.routing_iters, _lib.ptr(v),
                                            _lib.ptr(c), _lib.ptr(nsq), _lib.stream_ptr(dev)))
        return v, c


class ComiRecEngine(FlatModelEngine):
    """``train_single_batch((seq, target, samples)) -> float``, ``backward_only``, ``train_an_epoch(loader, epoch_id)``,
    ``set_item_probs``, ``predict``, ``recommend_next``; optimizers and checkpoints through the flat-model base."""

    def __init__(self, config):
        self.config = config
        self.model = ComiRec(config["model"])
        self._log_q = None
        self.last_kstar = None
        super(ComiRecEngine, self).__init__(config)
        self._n_batches = 0

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_comirec_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat ComiRec buffer is not laid out as libhiprec.so expects; rebuild the library")

    def set_item_probs(self, probs):
        """``probs [n_items + 1]``, indexed by item id (entry 0 is not read): the sampler's probability of every item,
        whose logarithm the sampled softmax subtracts from that item's logit.  An item without support has no finite shift:
        it must be neither a target nor a sample."""
        p = torch.as_tensor(np.asarray(probs, dtype=np.float64)).reshape(-1)
        if p.numel() != self.model.item_num + 1:
            raise ValueError(f"{p.numel()} item probabilities for ids 0 .. {self.model.item_num}")
        if float(p[1:].min()) < 0.0:
            raise ValueError("item probabilities must be >= 0")
        p[0] = 1.0
        self._log_q = torch.log(p).to(torch.float32).to(self.model.flat.device)

    # ---- the step ----------------------------------------------------------------------------------------------
    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        m = self.model
        dev = m.flat.device
        if len(batch_data) != 3:
            raise ValueError("a ComiRec batch is (seq [B, L], target [B], samples [S])")
        seq, target, samples = batch_data
        seq_t, B = m.sequences(seq)
        tgt_t, smp_t = index_tensor(target, dev), index_tensor(samples, dev)
        if tgt_t.numel() != B:
            raise ValueError(f"target must be [{B}]: one label for every sequence")
        S = int(smp_t.numel())
        if not 1 <= S <= MAX_SAMPLE:
            raise ValueError(f"a step takes 1..{MAX_SAMPLE} samples, got {S}")
        if self._log_q is not None and self._log_q.device != dev:
            self._log_q = self._log_q.to(dev)
        self.last_kstar = torch.empty(B, dtype=torch.int32, device=dev)
        ws = m.workspace(lib, B, S)
        _lib.check(lib.hiprec_comirec_grad(
            ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(seq_t), _lib.ptr(tgt_t), _lib.ptr(smp_t),
            B, S, _lib.ptr(self._log_q), None, _lib.ptr(self.last_kstar), _lib.ptr(self._stats), _lib.ptr(self._scratch),
            self._scratch.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))

    def train_single_batch(self, batch_data, ratings=None):
        """One step on ``(seq, target, samples)``: the loss (the mean over the labelled rows)."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_grad(batch_data)
        self._enqueue_opt()
        return self._sync_stats().loss

    def _epoch_step(self, batch):
        self._n_batches += 1
        self._enqueue_step(batch)

    def train_an_epoch(self, train_loader, epoch_id):
        """Every batch of the loader (``data.MultiInterestLoader``) enqueued back to back with ONE host sync at the end;
        returns the mean of the per-step losses and writes it to the writer."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._n_batches = 0
        st = self._run_epoch(train_loader)
        mean_loss = st.loss_sum / max(self._n_batches, 1)
        print("[Training Epoch {}], Loss {:.6f}".format(epoch_id, mean_loss))
        self.writer.add_scalar("model/loss", mean_loss, epoch_id)
        return mean_loss

    # ---- inference ---------------------------------------------------------------------------------------------
    def predict(self, seqs, item_indices):
        """Eval-mode scores ``[B, n]`` of the candidate list ``item_indices [n]``: the best over the interests."""
        self.model.eval()
        return self.model.predict(seqs, item_indices)

    def recommend_next(self, seqs, k, seen=None):
        """The ``k`` best next items for every sequence of ``seqs [n, L]`` by ``max_k <v[k], item_emb[i]>``:
        ``hiprec_topk_recommend`` on the ``n * K`` interest rows against ``item_emb.weight[1:]`` (each sequence's seen items
        hold for all its interests), then the merge kernel keeps per sequence the ``k`` best distinct items -- exact, because
        the top ``k`` by the best score lie within the union of the per-interest top ``k``.  The padding id is never
        returned.  ``seen``: None, or a ``(rows, items)`` pair of equally long id columns (an item 0 is ignored).  Returns
        ``(items [n, k] int64, scores [n, k] fp32)`` on the device, ``-1`` / ``-inf`` in a tail with nothing left."""
        from .recommend import topk_factors

        self.model.eval()
        v = self.model.interests(seqs)
        n, K, D = v.shape
        dev = v.device
        if seen is not None:
            rows, items = (index_tensor(x, dev) for x in seen)
            if rows.numel() != items.numel():
                raise ValueError("seen must be a (rows, items) pair of equally long id columns")
            if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
                raise ValueError(f"seen: a row outside [0, {n})")
            keep = items != 0
            rows, items = rows[keep], items[keep] - 1
            steps = torch.arange(K, device=dev)
            seen = ((rows[:, None] * K + steps[None, :]).reshape(-1), items[:, None].expand(-1, K).reshape(-1))
        table = self.model.item_emb.weight.data[1:]
        per_items, per_scores = topk_factors(v.view(n * K, D), table, 1.0, None, torch.arange(n * K, device=dev), k, seen)
        out_items = torch.empty((n, int(k)), dtype=torch.int64, device=dev)
        out_scores = torch.empty((n, int(k)), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().hiprec_comirec_merge(_lib.ptr(per_items), _lib.ptr(per_scores), n, K, int(k),
                                                    _lib.ptr(out_items), _lib.ptr(out_scores), _lib.stream_ptr(dev)))
        return torch.where(out_items >= 0, out_items + 1, out_items), out_scores
