"""Drop-in ``VBCAR`` / ``VBCAREngine`` for beta_rec/models/vbcar.py on libhiprec.so.

Interface parity (file:line = beta_rec/models/vbcar.py): ``VBCAR(config)`` :9-193 (``forward(batch) -> loss``,
``predict(users, items)``, ``kl_loss`` / ``rec_loss`` set by every forward), ``VBCAREngine(config)`` :196-301
(``train_single_batch(batch) -> float``, ``train_an_epoch(loader, epoch_id)`` which draws the negatives from
``engine.data``'s alias samplers).  Same config keys (``n_users n_items late_dim emb_dim n_neg batch_size alpha activator
optimizer lr device_str`` under ``config["model"]``, ``user_fea`` / ``item_fea`` at top level), same ``state_dict`` keys
and order (the features are no parameters and not in it), and the same constructed weights for the same torch seed: the
constructor builds the reference's torch modules in ``init_layers``' order and copies them into the flat buffer.

Kept from the reference on purpose:
* the KL term takes ``var1 = s^2 + 1e-10`` from the RAW second half of the encoder output, while ``reparameterize`` uses
  ``exp(0.5 s)`` (vbcar.py:74, 86);
* ``user_emb`` keeps ``nn.Embedding``'s N(0, 1); only ``item_emb`` is re-drawn uniform (vbcar.py:39-42);
* GEN and KLD are divided by ``3 * config batch_size`` also for a short last batch (vbcar.py:166, 174), each of the six KL
  terms being a mean over its own rows;
* any activator string the reference does not know means identity (vbcar.py:34-35).

Where the reference cannot run, the constructor or the call raises ``ValueError``: ``activator == "prelu"``
(``F.prelu`` without a weight), a batch of ONE triple (``.squeeze()`` drops the batch dimension, vbcar.py:138-139), and
shapes beyond the library's limits (``MAX_DIM``, ``MAX_LATE``, ``MAX_FEA``).

The noise of ``reparameterize`` is drawn on the host by :func:`draw_noise` (six ``torch.randn`` in the reference's call
order, so a CPU run of the reference under the same seed sees the same ``eps``); ``model.next_noise`` (six tensors, or
one stacked ``[3 B (1 + n_neg), D]``) overrides the draw for one step.  ``config["model"]["noise_rng"] = "device"`` draws
the stacked block with ONE ``torch.randn`` on the GPU instead (no host draw, no copy; another stream than the
reference's); the default is ``"torch_cpu"``.

Forward, loss and backward run in ``csrc/vbcar.hip`` (the four ``Linear`` layers through the grouped GEMM of
``csrc/ncf.hip``), the optimizer is the shared dense sweep.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor
from .triple2vec import _batch_tensors

MAX_DIM, MAX_LATE, MAX_FEA = 128, 512, 1 << 16
ACTIVATORS = {"tanh": 1, "sigmoid": 2, "relu": 3, "lrelu": 4}      # HIPREC_VBCAR_ACT_*; anything else: identity (0)


def draw_noise(B, n_neg, D, device):
    """``reparameterize``'s ``eps`` of one forward, stacked ``[3 B (1 + n_neg), D]`` on ``device``: six ``torch.randn``
    on the CPU generator in the reference's call order (pos_u, pos_i_1, pos_i_2, neg_u, neg_i_1, neg_i_2)."""
    blocks = [torch.randn(B, D) for _ in range(3)] + [torch.randn(B * n_neg, D) for _ in range(3)]
    return torch.cat(blocks).to(device)


def _spec(U, I, D, L, Fu, Fi):
    return [("user_emb.weight", (U, D)), ("item_emb.weight", (I, D)),
            ("fc_u_1_mu.weight", (L, Fu)), ("fc_u_1_mu.bias", (L,)),
            ("fc_u_2_mu.weight", (2 * D, L)), ("fc_u_2_mu.bias", (2 * D,)),
            ("fc_i_1_mu.weight", (L, Fi)), ("fc_i_1_mu.bias", (L,)),
            ("fc_i_2_mu.weight", (2 * D, L)), ("fc_i_2_mu.bias", (2 * D,))]


def _features(x, rows, what):
    t = torch.as_tensor(np.asarray(x.cpu() if torch.is_tensor(x) else x)).to(torch.float32)
    if t.dim() != 2 or t.shape[0] != rows or t.shape[1] < 1:
        raise ValueError(f"{what} must be [{rows}, width >= 1], got {tuple(t.shape)}")
    return t.contiguous()


class VBCAR(_FlatModel):
    """models/vbcar.py:9-193.  ``VBCAR(config["model"], user_fea, item_fea)``: the reference's ``VBCAR(config)`` +
    ``init_feature`` + ``init_layers`` in one.  Flat buffer in ``state_dict()`` order (``_spec``)."""

    def __init__(self, config, user_fea, item_fea):
        super().__init__()
        self.config = config
        self.n_users = int(config["n_users"])
        self.n_items = int(config["n_items"])
        self.late_dim = int(config["late_dim"])
        self.emb_dim = int(config["emb_dim"])
        self.n_neg = int(config["n_neg"])
        self.batch_size = config["batch_size"]
        self.alpha = config["alpha"]
        self.esp = 1e-10
        self.activator = config["activator"]
        self.noise_rng = config["noise_rng"] if "noise_rng" in config else "torch_cpu"
        if self.noise_rng not in ("torch_cpu", "device"):
            raise ValueError(f"unknown noise_rng {self.noise_rng!r}: 'torch_cpu' or 'device'")
        if self.activator == "prelu":
            raise ValueError("activator 'prelu' cannot run: the reference calls F.prelu without a weight")
        U, I, D, L = self.n_users, self.n_items, self.emb_dim, self.late_dim
        if U < 1 or I < 1:
            raise ValueError("VBCAR needs n_users >= 1 and n_items >= 1")
        if not 1 <= D <= MAX_DIM:
            raise ValueError(f"emb_dim must be in 1..{MAX_DIM}, got {D}")
        if not 1 <= L <= MAX_LATE:
            raise ValueError(f"late_dim must be in 1..{MAX_LATE}, got {L}")
        if self.n_neg < 1:
            raise ValueError(f"n_neg must be >= 1, got {self.n_neg}")
        self.user_fea = _features(user_fea, U, "user_fea")
        self.item_fea = _features(item_fea, I, "item_fea")
        self.user_fea_dim, self.item_fea_dim = int(self.user_fea.shape[1]), int(self.item_fea.shape[1])
        for what, F in (("user_fea", self.user_fea_dim), ("item_fea", self.item_fea_dim)):
            if F > MAX_FEA:
                raise ValueError(f"{what} is {F} wide; the limit is {MAX_FEA}")
        Fu, Fi = self.user_fea_dim, self.item_fea_dim
        self.shape = _lib.VbcarShape(U, I, D, L, Fu, Fi, ACTIVATORS.get(self.activator, 0), 0)
        v = self._build(_spec(U, I, D, L, Fu, Fi))
        # the reference's init_layers, module by module, for its RNG order (vbcar.py:39-46)
        mods = {"user_emb": nn.Embedding(U, D), "item_emb": nn.Embedding(I, D)}
        init_range = 0.1 * D ** (-1 / 2)
        mods["item_emb"].weight.data.uniform_(-init_range, init_range)
        mods["fc_u_1_mu"] = nn.Linear(Fu, L)
        mods["fc_u_2_mu"] = nn.Linear(L, 2 * D)
        mods["fc_i_1_mu"] = nn.Linear(Fi, L)
        mods["fc_i_2_mu"] = nn.Linear(L, 2 * D)
        for name, view in v.items():
            mod, attr = name.split(".")
            view.copy_(getattr(mods[mod], attr).data)
        self.user_emb = _ParamView(v["user_emb.weight"])
        self.item_emb = _ParamView(v["item_emb.weight"])
        for n in ("fc_u_1_mu", "fc_u_2_mu", "fc_i_1_mu", "fc_i_2_mu"):
            setattr(self, n, _ParamView(v[n + ".weight"], v[n + ".bias"]))
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
        """zero_grad + forward + loss + backward of one batch into ``g_flat`` (zero on entry), enqueued."""
        t, B, n_neg = _batch_tensors(self, batch_data)
        if B == 1:
            raise ValueError("a VBCAR batch needs at least 2 triples (the reference's .squeeze() drops the batch dimension)")
        if n_neg != self.n_neg:
            raise ValueError(f"negatives must be [batch, n_neg = {self.n_neg}], got n_neg = {n_neg}")
        noise = self._noise(B, n_neg)
        ws = self.workspace(lib, lib.hiprec_vbcar_workspace_bytes(ctypes.byref(self.shape), B, n_neg))
        _lib.check(lib.hiprec_vbcar_grad(
            ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(g_flat), _lib.ptr(self.user_fea),
            _lib.ptr(self.item_fea), *(_lib.ptr(x) for x in t), B, n_neg, _lib.ptr(noise), float(self.alpha),
            1.0 / (3 * self.batch_size), _lib.ptr(stats), _lib.ptr(scratch), scratch.numel(), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(self._flat.device)))

    def total_loss(self, gen, kld):
        """vbcar.py:178."""
        return (1 - self.alpha) * gen + self.alpha * kld

    def _set_losses(self, st):
        self.kl_loss, self.rec_loss = st.reg, st.loss
        return self.total_loss(st.loss, st.reg)

    # ---- reference API -----------------------------------------------------------------------------------------
    def forward(self, batch_data):
        """vbcar.py:111-178: the batch loss as a 0-dim tensor, ``kl_loss`` / ``rec_loss`` set (no autograd graph:
        training goes through ``VBCAREngine.train_single_batch``, which keeps the gradient this call discards)."""
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
        """``[mu(id) | emb[id]]`` as ``[n, 2 emb_dim]`` on the device: ``side`` ``"user"`` or ``"item"`` (what ``predict``
        multiplies, vbcar.py:185-191)."""
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
        ws = self.workspace(lib, lib.hiprec_vbcar_encode_workspace_bytes(ctypes.byref(self.shape), n, 0))
        _lib.check(lib.hiprec_vbcar_encode(
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
        """vbcar.py:180-193."""
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
        ws = self.workspace(lib, lib.hiprec_vbcar_encode_workspace_bytes(ctypes.byref(self.shape), n, 1))
        _lib.check(lib.hiprec_vbcar_predict(
            ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(self.user_fea), _lib.ptr(self.item_fea),
            _lib.ptr(users_t), _lib.ptr(items_t), n, _lib.ptr(scores), _lib.ptr(stats), _lib.ptr(ws), ws.numel(),
            _lib.stream_ptr(dev)))
        self._check_status()
        return scores


class VBCAREngine(FlatModelEngine):
    """models/vbcar.py:196-301."""

    def __init__(self, config):
        self.config = config
        self.model = VBCAR(config["model"], config["user_fea"], config["item_fea"])
        super(VBCAREngine, self).__init__(config)

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_vbcar_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat VBCAR buffer is not laid out as libhiprec.so expects; rebuild the library")

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
        """vbcar.py:219-227: one step, returns ``loss.item()``."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_step(batch_data)
        return self.model._set_losses(self._sync_stats())

    def _epoch_step(self, sample):
        """One iteration of vbcar.py:238-280: a ``[B, 3]`` block of (u, i1, i2) triples; the negatives come from
        ``engine.data``'s alias samplers in the reference's order (users, items, items)."""
        m = self.model
        dev = m.flat.device
        sample = torch.as_tensor(sample).to(torch.int64).reshape(-1, 3)
        n = sample.shape[0]
        neg = [torch.tensor(s.sample(m.n_neg, n), dtype=torch.int64, device=dev).reshape(n, -1)
               for s in (self.data.user_sampler, self.data.item_sampler, self.data.item_sampler)]
        self._enqueue_step((sample[:, 0], sample[:, 1], sample[:, 2], *neg))

    def train_an_epoch(self, train_loader, epoch_id):
        """vbcar.py:230-301: every step enqueued back to back with ONE host sync at the end; the three epoch totals are
        divided by the config batch size, printed and logged as the reference does."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        m = self.model
        st = self._run_epoch(train_loader)
        m._set_losses(st)                       # the last batch's, as the reference leaves them
        bs = self.config["model"]["batch_size"]
        total_loss = m.total_loss(st.loss_sum, st.reg_sum) / bs
        rec_loss = st.loss_sum / bs
        kl_loss = st.reg_sum / bs
        print("[Training Epoch {}], log_like_loss {} kl_loss: {} alpha: {} lr: {}".format(
            epoch_id, rec_loss, kl_loss, m.alpha, self.config["model"]["lr"]))
        self.writer.add_scalars(
            "model/loss", {"total_loss": total_loss, "rec_loss": total_loss - kl_loss, "kl_loss": kl_loss}, epoch_id)
