"""Drop-in ``TVBR`` / ``TVBREngine`` for beta_rec/models/tvbr.py on libhiprec.so.

Interface parity (file:line = beta_rec/models/tvbr.py): ``TVBR(config)`` :11-412 (``forward(batch) -> loss``,
``predict(users, items)``, ``kl_loss`` / ``rec_loss`` set by every forward), ``TVBREngine(config)`` :415-571
(``train_single_batch(batch) -> float``, ``train_an_epoch(triple_df, epoch_id)`` which walks the time steps and draws the
negatives from ``engine.data``'s samplers).  Same config keys (``n_users n_items late_dim emb_dim n_neg batch_size alpha
time_step activator optimizer lr device_str`` under ``config["model"]``, ``user_fea`` / ``item_fea`` at top level), same
``state_dict`` keys and order -- ``time_embdding`` spelt as the reference spells it, ``time2mean_u.0.weight`` and the
rest, plus the four ``.1.weight`` slopes under ``prelu`` -- and the same constructed weights for the same torch seed: the
constructor builds the reference's torch modules in ``init_layers``' order and copies them into the flat buffer.

A batch is the reference's eight-tuple ``(pos_u, pos_i_1, pos_i_2 [B], neg_u, neg_i_1, neg_i_2 [B, n_neg], pos_batch_t
[B], neg_batch_t [B n_neg])``; every row carries its own ``t`` in ``[0, time_step)``: the prior reads row ``t`` of the
time table, the posterior row ``t + 1``.

Kept from the reference on purpose:
* ``std = exp(0.5 act(lin))``, and ``reparameterize`` is handed that ``std`` as if it were a log-variance, so
  ``z = mean + eps exp(0.5 std)`` (tvbr.py:148-152, 199-201, 281);
* ``kl_div(prior, posterior)`` takes ``var = std^2 + 1e-10`` and is always called in its ``neg=False`` form: each of the
  six terms is a mean over the rows of its own group, ``B`` or ``B n_neg`` (tvbr.py:217-231, 282-321);
* ``kl_loss = -0.5 x`` the sum of the six KL terms, not divided by anything (tvbr.py:365);
* ``rec_loss`` is divided by ``3 x`` the CONFIG batch size, also for a short batch (tvbr.py:364);
* ``user_mean`` starts as ones and ``user_std`` as zeros while the item tables are re-drawn uniform (tvbr.py:79-94);
* ``late_dim`` is read nowhere.

Where the reference cannot run, the constructor or the call raises ``ValueError``: an activator outside ``tanh hardtanh
logsigmoid sigmoid relu lrelu prelu`` (``init_layers`` calls a one-argument lambda with none), a batch of ONE triple
(``.squeeze()`` drops the batch dimension, tvbr.py:339-343), negatives whose width is not the config's ``n_neg``, and
shapes beyond the library's limits (``MAX_DIM``, ``MAX_FEA``, ``MAX_TIME``).  A time step without a single triple is
skipped by ``train_an_epoch`` (the reference's shuffling ``DataLoader`` raises on an empty slice).  An id outside its
table or a ``t`` outside ``[0, time_step)`` raises ``IndexError`` and leaves the engine usable.

The noise of ``reparameterize`` comes from :func:`vbcar.draw_noise` (six ``torch.randn`` in the reference's call order,
so a CPU run of the reference under the same seed sees the same ``eps``); ``model.next_noise`` (six tensors, or one
stacked ``[3 B (1 + n_neg), D]``) overrides the draw for one step; ``model.last_noise`` keeps what a step used.
``config["model"]["noise_rng"] = "device"`` draws the stacked block with ONE ``torch.randn`` on the GPU instead; the
default is ``"torch_cpu"``.

Forward, loss and backward run in ``csrc/tvbr.hip`` (the encoders through the grouped GEMM of ``csrc/ncf.hip``), the
optimizer is the shared dense sweep.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor
from .triple2vec import _batch_tensors
from .vbcar import _features, draw_noise

MAX_DIM, MAX_FEA, MAX_TIME = 128, 1 << 16, 255
# HIPREC_TVBR_ACT_*: the seven names the reference's constructor knows
ACTIVATORS = {"tanh": 1, "hardtanh": 2, "logsigmoid": 3, "sigmoid": 4, "relu": 5, "lrelu": 6, "prelu": 7}
ENCODERS = ("time2mean_u", "time2std_u", "time2mean_i", "time2std_i")


def _spec(U, I, D, T, Fu, Fi, prelu):
    T1 = T + 1
    spec = [("user_emb.weight", (U, D)), ("item_emb.weight", (I, D)), ("time_embdding.weight", (T1, T1)),
            ("user_mean.weight", (U, D)), ("user_std.weight", (U, D)),
            ("item_mean.weight", (I, D)), ("item_std.weight", (I, D))]
    for name, F in zip(ENCODERS, (Fu, Fu, Fi, Fi)):
        spec += [(name + ".0.weight", (D, D + T1 + F)), (name + ".0.bias", (D,))]
        if prelu:
            spec.append((name + ".1.weight", (1,)))
    return spec


class TVBR(_FlatModel):
    """models/tvbr.py:11-412.  ``TVBR(config["model"], user_fea, item_fea)``: the reference's ``TVBR(config)`` +
    ``init_feature`` + ``init_layers`` in one.  Flat buffer in ``state_dict()`` order (``_spec``)."""

    def __init__(self, config, user_fea, item_fea):
        super().__init__()
        self.config = config
        self.n_users = int(config["n_users"])
        self.n_items = int(config["n_items"])
        self.late_dim = config["late_dim"] if "late_dim" in config else None
        self.emb_dim = int(config["emb_dim"])
        self.n_neg = int(config["n_neg"])
        self.batch_size = config["batch_size"]
        self.alpha = config["alpha"]
        self.time_step = int(config["time_step"])
        self.esp = 1e-10
        self.activator = config["activator"]
        self.noise_rng = config["noise_rng"] if "noise_rng" in config else "torch_cpu"
        if self.noise_rng not in ("torch_cpu", "device"):
            raise ValueError(f"unknown noise_rng {self.noise_rng!r}: 'torch_cpu' or 'device'")
        if self.activator not in ACTIVATORS:
            raise ValueError(f"activator {self.activator!r} cannot run in the reference: one of {', '.join(ACTIVATORS)}")
        U, I, D, T = self.n_users, self.n_items, self.emb_dim, self.time_step
        if U < 1 or I < 1:
            raise ValueError("TVBR needs n_users >= 1 and n_items >= 1")
        if not 1 <= D <= MAX_DIM:
            raise ValueError(f"emb_dim must be in 1..{MAX_DIM}, got {D}")
        if not 1 <= T <= MAX_TIME:
            raise ValueError(f"time_step must be in 1..{MAX_TIME}, got {T}")
        if self.n_neg < 1:
            raise ValueError(f"n_neg must be >= 1, got {self.n_neg}")
        self.user_fea = _features(user_fea, U, "user_fea")
        self.item_fea = _features(item_fea, I, "item_fea")
        self.user_fea_dim, self.item_fea_dim = int(self.user_fea.shape[1]), int(self.item_fea.shape[1])
        for what, F in (("user_fea", self.user_fea_dim), ("item_fea", self.item_fea_dim)):
            if F > MAX_FEA:
                raise ValueError(f"{what} is {F} wide; the limit is {MAX_FEA}")
        Fu, Fi = self.user_fea_dim, self.item_fea_dim
        prelu = self.activator == "prelu"
        self.shape = _lib.TvbrShape(U, I, D, T, Fu, Fi, ACTIVATORS[self.activator], 0)
        v = self._build(_spec(U, I, D, T, Fu, Fi, prelu))
        # the reference's init_layers, module by module, for its RNG order (tvbr.py:67-119)
        mods = {"user_emb": nn.Embedding(U, D), "item_emb": nn.Embedding(I, D)}
        init_range = 0.1 * D ** (-1 / 2)
        mods["user_emb"].weight.data.uniform_(-init_range, init_range)
        mods["item_emb"].weight.data.uniform_(-init_range, init_range)
        mods["time_embdding"] = nn.Embedding(T + 1, T + 1, _weight=torch.eye(T + 1, T + 1))
        mods["user_mean"] = nn.Embedding(U, D, _weight=torch.ones(U, D))
        mods["user_std"] = nn.Embedding(U, D, _weight=torch.zeros(U, D))
        mods["item_mean"] = nn.Embedding(I, D, _weight=torch.ones(I, D))
        mods["item_std"] = nn.Embedding(I, D, _weight=torch.zeros(I, D))
        mods["item_mean"].weight.data.uniform_(-init_range, init_range)
        mods["item_std"].weight.data.uniform_(-init_range, init_range)
        for name, F in zip(ENCODERS, (Fu, Fu, Fi, Fi)):
            mods[name] = nn.Sequential(nn.Linear(D + T + 1 + F, D), nn.PReLU() if prelu else nn.Identity())
        built = nn.ModuleDict(mods)
        for name, view in v.items():
            view.copy_(built.get_parameter(name).data)
        for n in ("user_emb", "item_emb", "time_embdding", "user_mean", "user_std", "item_mean", "item_std"):
            setattr(self, n, _ParamView(v[n + ".weight"]))
        for n in ENCODERS:
            second = _ParamView(v[n + ".1.weight"]) if prelu else nn.Identity()
            setattr(self, n, nn.Sequential(_ParamView(v[n + ".0.weight"], v[n + ".0.bias"]), second))
        self.kl_loss = self.rec_loss = None
        self.next_noise = None
        self.last_noise = None
        self._ws = None
        self._fwd = None

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        dev = self._flat.device
        if self.user_fea.device != dev:          # the features travel with the parameters (they are no parameters)
            self.user_fea = self.user_fea.to(dev).contiguous()
            self.item_fea = self.item_fea.to(dev).contiguous()
        return self

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, need):
        if need == 0:
            raise ValueError("unsupported batch: " + (lib.hiprec_last_error() or b"beyond the library's limits").decode())
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def _noise(self, B, n_neg):
        """The step's ``eps`` as one ``[3 B (1 + n_neg), D]`` fp32 device tensor: ``next_noise`` once, else a draw."""
        dev, D = self._flat.device, self.emb_dim
        given, self.next_noise = self.next_noise, None
        if given is None and self.noise_rng == "device":
            noise = torch.randn((3 * B * (1 + n_neg), D), dtype=torch.float32, device=dev)
        elif given is None:
            noise = draw_noise(B, n_neg, D, dev)
        else:
            if not torch.is_tensor(given):
                given = torch.cat([torch.as_tensor(np.asarray(x.cpu() if torch.is_tensor(x) else x)).reshape(-1, D)
                                   for x in given])
            noise = given.to(dev, torch.float32).reshape(-1, D).contiguous()
            if noise.shape[0] != 3 * B * (1 + n_neg):
                raise ValueError(f"noise of {noise.shape[0]} rows where {3 * B * (1 + n_neg)} are expected")
        self.last_noise = noise
        return noise

    def enqueue_grad(self, lib, g_flat, batch_data, stats, scratch):
        """zero_grad + forward + loss + backward of one eight-tuple into ``g_flat`` (zero on entry), enqueued."""
        if len(batch_data) != 8:
            raise ValueError("TVBR batches are (pos_u, pos_i_1, pos_i_2, neg_u, neg_i_1, neg_i_2, pos_batch_t, neg_batch_t)")
        t, B, n_neg = _batch_tensors(self, batch_data[:6])
        if B == 1:
            raise ValueError("a TVBR batch needs at least 2 triples (the reference's .squeeze() drops the batch dimension)")
        if n_neg != self.n_neg:
            raise ValueError(f"negatives must be [batch, n_neg = {self.n_neg}], got n_neg = {n_neg}")
        dev = self._flat.device
        pos_t, neg_t = index_tensor(batch_data[6], dev), index_tensor(batch_data[7], dev)
        if pos_t.numel() != B or neg_t.numel() != B * n_neg:
            raise ValueError(f"pos_batch_t must hold {B} and neg_batch_t {B * n_neg} time steps, got {pos_t.numel()} and "
                             f"{neg_t.numel()}")
        noise = self._noise(B, n_neg)
        ws = self.workspace(lib, lib.hiprec_tvbr_workspace_bytes(ctypes.byref(self.shape), B, n_neg))
        _lib.check(lib.hiprec_tvbr_grad(
            ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(g_flat), _lib.ptr(self.user_fea),
            _lib.ptr(self.item_fea), *(_lib.ptr(x) for x in t), _lib.ptr(pos_t), _lib.ptr(neg_t), B, n_neg,
            _lib.ptr(noise), float(self.alpha), 1.0 / (3 * self.batch_size), _lib.ptr(stats), _lib.ptr(scratch),
            scratch.numel(), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))

    def total_loss(self, rec, kl):
        """tvbr.py:369."""
        return (1 - self.alpha) * rec + self.alpha * kl

    def _set_losses(self, st):
        self.kl_loss, self.rec_loss = st.reg, st.loss
        return self.total_loss(st.loss, st.reg)

    # ---- reference API -----------------------------------------------------------------------------------------
    def forward(self, batch_data):
        """tvbr.py:242-369: the batch loss as a 0-dim tensor, ``kl_loss`` / ``rec_loss`` set (no autograd graph:
        training goes through ``TVBREngine.train_single_batch``, which keeps the gradient this call discards)."""
        lib = self._require_hip()
        dev = self._flat.device
        stats = self._device_stats()
        if self._fwd is None or self._fwd[0].device != dev:
            self._fwd = (torch.zeros_like(self._flat),
                         torch.zeros(lib.hiprec_scratch_bytes(0), dtype=torch.uint8, device=dev))
        g, scratch = self._fwd
        g.zero_()
        self.enqueue_grad(lib, g, batch_data, stats, scratch)
        _lib.check(lib.hiprec_finalize_stats(_lib.ptr(stats), _lib.ptr(scratch), None, None, _lib.stream_ptr(dev)))
        return torch.tensor(self._set_losses(self._check_status()), device=dev)

    def encode(self, ids, side):
        """``[posterior mean(id) at t = time_step | emb[id]]`` as ``[n, 2 emb_dim]`` on the device: ``side`` ``"user"``
        or ``"item"`` (what ``predict`` multiplies, tvbr.py:380-407)."""
        lib = self._require_hip()
        dev = self._flat.device
        if side not in ("user", "item"):
            raise ValueError("side is 'user' or 'item'")
        ids_t = index_tensor(ids, dev)
        n = ids_t.numel()
        out = torch.empty((n, 2 * self.emb_dim), dtype=torch.float32, device=dev)
        if n == 0:
            return out
        stats = self._device_stats()
        ws = self.workspace(lib, lib.hiprec_tvbr_encode_workspace_bytes(ctypes.byref(self.shape), n, 0))
        _lib.check(lib.hiprec_tvbr_encode(
            ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(self.user_fea if side == "user" else self.item_fea),
            _lib.ptr(ids_t), n, 0 if side == "user" else 1, _lib.ptr(out), _lib.ptr(stats), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)))
        self._check_status()
        return out

    def ranking_factors(self):
        """``(U, I, 1.0, None)`` for full-catalogue ranking (``recommend.recommend``, ``eval.evaluate_full``): every
        user and every item encoded; ``predict`` is their dot product."""
        dev = self._flat.device
        return (self.encode(torch.arange(self.n_users, device=dev), "user"),
                self.encode(torch.arange(self.n_items, device=dev), "item"), 1.0, None)

    def predict(self, users, items):
        """tvbr.py:371-412."""
        lib = self._require_hip()
        dev = self._flat.device
        users_t, items_t = index_tensor(users, dev), index_tensor(items, dev)
        if users_t.numel() != items_t.numel():
            raise ValueError("users and items differ in length")
        n = users_t.numel()
        scores = torch.empty(n, dtype=torch.float32, device=dev)
        if n == 0:
            return scores
        stats = self._device_stats()
        ws = self.workspace(lib, lib.hiprec_tvbr_encode_workspace_bytes(ctypes.byref(self.shape), n, 1))
        _lib.check(lib.hiprec_tvbr_predict(
            ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(self.user_fea), _lib.ptr(self.item_fea),
            _lib.ptr(users_t), _lib.ptr(items_t), n, _lib.ptr(scores), _lib.ptr(stats), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)))
        self._check_status()
        return scores


class TVBREngine(FlatModelEngine):
    """models/tvbr.py:415-571."""

    def __init__(self, config):
        self.config = config
        self.time_step = config["model"]["time_step"]
        self.batch_size = config["model"]["batch_size"]
        self.n_neg = config["model"]["n_neg"]
        self.model = TVBR(config["model"], config["user_fea"], config["item_fea"])
        super(TVBREngine, self).__init__(config)

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_tvbr_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat TVBR buffer is not laid out as libhiprec.so expects; rebuild the library")

    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        self.model.enqueue_grad(lib, self._g_flat, batch_data, self._stats, self._scratch)

    def backward_only(self, batch_data):
        """zero_grad + forward + loss + backward without the optimizer step: ``(loss, grads)``; ``model.kl_loss`` and
        ``model.rec_loss`` are set."""
        self._enqueue_grad(batch_data)
        st, grads = self._finish_backward_only()
        return self.model._set_losses(st), grads

    def train_single_batch(self, batch_data, ratings=None):
        """tvbr.py:449-465: one step, returns ``loss.item()``."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_step(batch_data)
        return self.model._set_losses(self._sync_stats())

    def _time_slices(self, triple_df):
        """tvbr.py:480-488: per time step, the rows with ``T == t`` through the reference's own ``DataLoader``."""
        for t in range(self.time_step):
            t_triple_df = triple_df[triple_df["T"] == t]
            if len(t_triple_df) == 0:            # shuffle=True raises on an empty dataset; such a time step gives no step
                continue
            train_loader = DataLoader(torch.tensor(t_triple_df.to_numpy()), batch_size=self.batch_size, shuffle=True,
                                      drop_last=True)
            for sample in train_loader:
                yield t, sample

    def _epoch_step(self, item):
        """One iteration of tvbr.py:488-550: a ``[B, >= 3]`` block of (u, i1, i2, ...) rows of time step ``t``; the
        negatives come from ``engine.data``'s samplers in the reference's order (users, items, items)."""
        t, sample = item
        m = self.model
        dev = m.flat.device
        sample = torch.as_tensor(sample).to(torch.int64)
        n = sample.shape[0]
        neg = [torch.tensor(s.sample(m.n_neg, n), dtype=torch.int64, device=dev).reshape(n, -1)
               for s in (self.data.user_sampler, self.data.item_sampler, self.data.item_sampler)]
        pos_t = torch.full((self.batch_size,), t, dtype=torch.int64, device=dev)
        neg_t = torch.full((self.batch_size * self.n_neg,), t, dtype=torch.int64, device=dev)
        self._enqueue_step((sample[:, 0], sample[:, 1], sample[:, 2], *neg, pos_t, neg_t))

    def train_an_epoch(self, triple_df, epoch_id):
        """tvbr.py:468-571: every step enqueued back to back with ONE host sync at the end; the three epoch totals are
        divided by the config batch size, printed and logged as the reference does."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        m = self.model
        st = self._run_epoch(self._time_slices(triple_df))
        m._set_losses(st)                       # the last batch's, as the reference leaves them
        bs = self.config["model"]["batch_size"]
        total_loss = m.total_loss(st.loss_sum, st.reg_sum) / bs
        rec_loss = st.loss_sum / bs
        kl_loss = st.reg_sum / bs
        print("[Training Epoch {}], log_like_loss {} kl_loss: {} alpha: {} lr: {}".format(
            epoch_id, rec_loss, kl_loss, m.alpha, self.config["model"]["lr"]))
        self.writer.add_scalars(
            "model/loss", {"total_loss": total_loss, "rec_loss": total_loss - kl_loss, "kl_loss": kl_loss}, epoch_id)
