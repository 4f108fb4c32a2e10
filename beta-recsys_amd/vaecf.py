"""Drop-in ``VAE`` / ``VAECFEngine`` for beta_rec/models/vaecf.py (Mult-VAE) on libhiprec.so.

Interface parity (file:line = beta_rec/models/vaecf.py): ``VAE(z_dim, ae_structure, config)`` :9-108 (``encode``,
``decode``, ``reparameterize``, ``forward``, ``predict``), ``VAECFEngine(config)`` :111-167 (``train_single_batch(batch)
-> float``, ``train_an_epoch((user_indices, matrix), epoch_id)``).  Same config keys (``n_users n_items activation
likelihood batch_size lr beta weight_decay device_str`` under ``config["model"]``), same ``state_dict`` keys and order
(``encoder.fc{i}``, ``enc_mu``, ``enc_logvar``, ``decoder.fc{i}``) and the same constructed weights for the same torch
seed: the constructor builds the reference's ``nn.Linear`` modules in its order and copies them into the flat buffer.

Kept from the reference on purpose:
* ``predict(user_idx, item_idx)`` builds ``x_u`` from the query pairs themselves (duplicates summed) and returns
  ``decode(mu(x_u)).flatten()[item_idx]`` (vaecf.py:98-106): because of the flatten that is ROW 0's probabilities at
  ``item_idx``, whatever users were asked for.  :meth:`VAE.score` is the per-pair score from each user's history;
* ``EPS = 1e-10`` sits inside the logs exactly where the reference puts it, also where fp32 absorbs it (``1 - p + EPS``);
* the KL term is written with ``std = exp(0.5 logvar)`` and ``2 log(std)`` (vaecf.py:83-85);
* the loss is the mean over the rows of the batch at hand, also for a short last batch (vaecf.py:87);
* the epoch loop binarises the matrix and prints / logs the SUM of the batch losses (vaecf.py:160-167).

One deliberate difference: the optimizer is always vaecf.py:128-130's ``Adam(lr, weight_decay)``, the decay being torch's
L2 into the gradient, whatever ``config["model"]["optimizer"]`` says.  The reference's base class goes on to replace that
optimizer by the config's at ``lr`` alone when the string is sgd / adam / rmsprop (torch_engine.py:16, 23-39), which drops
the decay; with the default config (adam, decay 0) the two are the same.

Extensions whose default is the reference's: ``config["model"]["z_dim"]`` (10) and ``["hidden"]`` (``[20]``) size the
network the engine builds; ``["noise_rng"]`` is ``"torch_cpu"`` (one ``torch.randn`` on the CPU generator per step: a CPU
run of the reference under the same seed sees the same ``eps``) or ``"device"``; ``model.next_noise`` overrides the draw
for one step; ``["w0_gather"]`` is ``"strided"`` or ``"shadow"`` (csrc/vaecf.hip).

Where the reference cannot run, the constructor raises ``ValueError``: an activation outside sigmoid / tanh / relu / relu6
(the reference dies on a missing ``act_fn``), an unknown likelihood, shapes beyond the library's limits.

A batch is the reference's dense ``[B, n_items]`` tensor (turned into CSR on the device, values kept) or a ``(row_ptr,
items[, values])`` triple with items unique within a row.  No ``[B, n_items]`` buffer exists on the compute path: forward,
loss and backward run in ``csrc/vaecf.hip``, the optimizer is the shared dense sweep.  There is no CPU path.
"""
import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .flat_engine import FlatModelEngine, _FlatModel, _ParamView, index_tensor
from .torch_engine import HipOptimizer

MAX_Z, MAX_HIDDEN, MAX_LAYERS = 256, 512, 3
ACTIVATIONS = {"sigmoid": 0, "tanh": 1, "relu": 2, "relu6": 3}      # HIPREC_VAECF_ACT_*
LIKELIHOODS = {"mult": 0, "bern": 1, "gaus": 2, "pois": 3}          # HIPREC_VAECF_LIK_*


def draw_noise(B, z_dim, device):
    """``reparameterize``'s ``eps`` of one forward, ``[B, z_dim]`` on ``device``: one ``torch.randn`` on the CPU generator
    (what the reference's ``randn_like(mu)`` draws on the CPU under the same seed)."""
    return torch.randn(B, z_dim).to(device)


def _spec(ae_structure, z_dim):
    enc = list(ae_structure)
    dec = [z_dim] + enc[::-1]
    spec = []
    for l in range(len(enc) - 1):
        spec += [(f"encoder.fc{l}.weight", (enc[l + 1], enc[l])), (f"encoder.fc{l}.bias", (enc[l + 1],))]
    for name in ("enc_mu", "enc_logvar"):
        spec += [(name + ".weight", (z_dim, enc[-1])), (name + ".bias", (z_dim,))]
    for l in range(len(dec) - 1):
        spec += [(f"decoder.fc{l}.weight", (dec[l + 1], dec[l])), (f"decoder.fc{l}.bias", (dec[l + 1],))]
    return spec


def _get(config, key, default):
    return config[key] if key in config else default


class _Layers(nn.Module):
    """Stands where the reference has an ``nn.Sequential`` of ``fc{i}`` / ``act{i}``: holds the ``fc{i}`` views."""


def _as_csr(batch, n_items, device):
    """``(row_ptr, items, values, B, nnz)`` on ``device`` from a dense ``[B, n_items]`` tensor / array or a ``(row_ptr,
    items[, values])`` triple."""
    if isinstance(batch, (tuple, list)):
        if len(batch) not in (2, 3):
            raise ValueError("a CSR batch is (row_ptr, items) or (row_ptr, items, values)")
        row_ptr, items = index_tensor(batch[0], device), index_tensor(batch[1], device)
        if row_ptr.numel() < 2:
            raise ValueError("row_ptr needs at least two entries (one row)")
        if len(batch) == 3:
            v = batch[2]
            values = (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(device, torch.float32).reshape(-1)
            values = values.contiguous()
        else:
            values = torch.ones(items.numel(), dtype=torch.float32, device=device)
        if values.numel() != items.numel():
            raise ValueError("items and values differ in length")
        return row_ptr, items, values, row_ptr.numel() - 1, items.numel()
    x = batch if torch.is_tensor(batch) else torch.as_tensor(np.asarray(batch))
    if x.dim() != 2 or x.shape[1] != n_items or x.shape[0] < 1:
        raise ValueError(f"a dense batch must be [B >= 1, n_items = {n_items}], got {tuple(x.shape)}")
    x = x.to(device, torch.float32)
    nz = x != 0
    row_ptr = torch.zeros(x.shape[0] + 1, dtype=torch.int64, device=device)
    row_ptr[1:] = torch.cumsum(nz.sum(1), 0)
    items = nz.nonzero()[:, 1].contiguous()
    return row_ptr, items, x[nz].contiguous(), x.shape[0], items.numel()


def _history_csr(history, n_users, device, binarise=True):
    """``(user_ptr, items, values)`` on ``device`` from a scipy sparse matrix or a ``(user_ptr, items[, values])``
    tuple covering every user."""
    if hasattr(history, "tocsr"):
        m = history.tocsr().copy()
        m.sum_duplicates()
        ptr, items = index_tensor(m.indptr, device), index_tensor(m.indices, device)
        values = torch.as_tensor(np.asarray(m.data, dtype=np.float32)).to(device)
    else:
        ptr, items = index_tensor(history[0], device), index_tensor(history[1], device)
        values = (torch.as_tensor(np.asarray(history[2], dtype=np.float32)).to(device) if len(history) == 3
                  else torch.ones(items.numel(), dtype=torch.float32, device=device))
    if ptr.numel() != n_users + 1:
        raise ValueError(f"the history must hold one row per user ({n_users}), got {ptr.numel() - 1}")
    if binarise:
        values = torch.ones_like(values)
    return ptr, items, values.contiguous()


class VAE(_FlatModel):
    """models/vaecf.py:9-108.  Flat buffer in ``state_dict()`` order (``_spec``)."""

    def __init__(self, z_dim, ae_structure, config):
        super().__init__()
        self.config = config
        self.z_dim = int(z_dim)
        self.ae_structure = [int(x) for x in ae_structure]
        self.activation = config["activation"]
        self.likelihood = config["likelihood"]
        self.EPS = 1e-10
        self.noise_rng = _get(config, "noise_rng", "torch_cpu")
        self.w0_gather = _get(config, "w0_gather", "strided")
        if self.activation not in ACTIVATIONS:
            raise ValueError(f"activation {self.activation!r} cannot run: the reference knows {sorted(ACTIVATIONS)}")
        if self.likelihood not in LIKELIHOODS:
            raise ValueError(f"Supported likelihoods: {sorted(LIKELIHOODS)}")
        if self.noise_rng not in ("torch_cpu", "device"):
            raise ValueError(f"unknown noise_rng {self.noise_rng!r}: 'torch_cpu' or 'device'")
        if self.w0_gather not in ("strided", "shadow"):
            raise ValueError(f"unknown w0_gather {self.w0_gather!r}: 'strided' or 'shadow'")
        hidden = self.ae_structure[1:]
        self.n_items = self.ae_structure[0] if self.ae_structure else 0
        self.n_users = int(_get(config, "n_users", 1))
        if "n_items" in config and int(config["n_items"]) != self.n_items:
            raise ValueError("ae_structure[0] must be n_items")
        if self.n_items < 1 or self.n_users < 1:
            raise ValueError("VAECF needs n_users >= 1 and n_items >= 1")
        if not 1 <= self.z_dim <= MAX_Z:
            raise ValueError(f"z_dim must be in 1..{MAX_Z}, got {self.z_dim}")
        if not 1 <= len(hidden) <= MAX_LAYERS:
            raise ValueError(f"ae_structure needs 1..{MAX_LAYERS} hidden layers, got {len(hidden)}")
        if any(not 1 <= h <= MAX_HIDDEN for h in hidden):
            raise ValueError(f"hidden widths must be in 1..{MAX_HIDDEN}, got {hidden}")
        self.hidden = hidden
        self.shape = _lib.VaecfShape(self.n_users, self.n_items, self.z_dim, len(hidden),
                                     (ctypes.c_int32 * 3)(*(hidden + [0] * (3 - len(hidden)))),
                                     ACTIVATIONS[self.activation], LIKELIHOODS[self.likelihood],
                                     1 if self.w0_gather == "shadow" else 0)
        spec = _spec(self.ae_structure, self.z_dim)
        v = self._build(spec)
        # the reference's modules in its order of construction, for its RNG order (vaecf.py:26-43)
        mods = {}
        enc = self.ae_structure
        for l in range(len(enc) - 1):
            mods[f"encoder.fc{l}"] = nn.Linear(enc[l], enc[l + 1])
        mods["enc_mu"] = nn.Linear(enc[-1], self.z_dim)
        mods["enc_logvar"] = nn.Linear(enc[-1], self.z_dim)
        dec = [self.z_dim] + enc[::-1]
        for l in range(len(dec) - 1):
            mods[f"decoder.fc{l}"] = nn.Linear(dec[l], dec[l + 1])
        for name, view in v.items():
            mod, attr = name.rsplit(".", 1)
            view.copy_(getattr(mods[mod], attr).data)
        self.encoder = _Layers()
        for l in range(len(enc) - 1):
            self.encoder.add_module(f"fc{l}", _ParamView(v[f"encoder.fc{l}.weight"], v[f"encoder.fc{l}.bias"]))
        self.enc_mu = _ParamView(v["enc_mu.weight"], v["enc_mu.bias"])
        self.enc_logvar = _ParamView(v["enc_logvar.weight"], v["enc_logvar.bias"])
        self.decoder = _Layers()
        for l in range(len(dec) - 1):
            self.decoder.add_module(f"fc{l}", _ParamView(v[f"decoder.fc{l}.weight"], v[f"decoder.fc{l}.bias"]))
        self.next_noise = None
        self.last_noise = None
        self.kld = self.ll = None
        self._ws = None
        self._fwd = None
        self._history = None

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        if self._history is not None and self._history[0].device != self._flat.device:
            self._history = tuple(t.to(self._flat.device) for t in self._history)
        return self

    # ---- device-side plumbing --------------------------------------------------------------------------------
    def workspace(self, lib, need):
        if need == 0:
            raise ValueError("unsupported batch: " + (lib.hiprec_last_error() or b"beyond the library's limits").decode())
        self._ws = _lib.grow(self._ws, need, torch.uint8, self._flat.device)
        return self._ws

    def _noise(self, B):
        """The step's ``eps`` as one ``[B, z_dim]`` fp32 device tensor: ``next_noise`` once, else a draw."""
        dev, Z = self._flat.device, self.z_dim
        given, self.next_noise = self.next_noise, None
        if given is None and self.noise_rng == "device":
            noise = torch.randn((B, Z), dtype=torch.float32, device=dev)
        elif given is None:
            noise = draw_noise(B, Z, dev)
        else:
            given = given if torch.is_tensor(given) else torch.as_tensor(np.asarray(given))
            noise = given.to(dev, torch.float32).contiguous()
            if tuple(noise.shape) != (B, Z):
                raise ValueError(f"noise of shape {tuple(noise.shape)} where {(B, Z)} is expected")
        self.last_noise = noise
        return noise

    def enqueue_grad(self, lib, g_flat, batch, beta, stats, scratch):
        """zero_grad + forward + loss + backward of one batch into ``g_flat`` (zero on entry), enqueued."""
        if not isinstance(batch, _Csr):
            batch = _as_csr(batch, self.n_items, self._flat.device)
        row_ptr, items, values, B, nnz = batch
        noise = self._noise(B)
        ws = self.workspace(lib, lib.hiprec_vaecf_workspace_bytes(ctypes.byref(self.shape), B, nnz))
        _lib.check(lib.hiprec_vaecf_grad(
            ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(g_flat), _lib.ptr(row_ptr), _lib.ptr(items),
            _lib.ptr(values), B, nnz, _lib.ptr(noise), float(beta), _lib.ptr(stats), _lib.ptr(scratch), scratch.numel(),
            _lib.ptr(ws), ws.numel(), _lib.stream_ptr(self._flat.device)))

    def total_loss(self, ll, kld, beta):
        """vaecf.py:87 from its two means."""
        return beta * kld - ll

    def _set_losses(self, st, beta):
        self.ll, self.kld = st.loss, st.reg
        return self.total_loss(st.loss, st.reg, beta)

    def _encode_csr(self, row_ptr, items, values, n_rows, nnz):
        """``(mu [n, z_dim], Hd(mu) [n, hidden[0]])`` of CSR rows, on the device."""
        lib = self._require_hip()
        dev = self._flat.device
        mu = torch.empty((n_rows, self.z_dim), dtype=torch.float32, device=dev)
        hd = torch.empty((n_rows, self.hidden[0]), dtype=torch.float32, device=dev)
        if n_rows == 0:
            return mu, hd
        stats = self._device_stats()
        ws = self.workspace(lib, lib.hiprec_vaecf_encode_workspace_bytes(ctypes.byref(self.shape), n_rows))
        _lib.check(lib.hiprec_vaecf_encode(
            ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(row_ptr), _lib.ptr(items), _lib.ptr(values), n_rows,
            nnz, _lib.ptr(mu), _lib.ptr(hd), _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return mu, hd

    def _decode_at(self, hd, rows, items):
        """The decoded probability at ``(rows[k], items[k])`` of ``hd``'s rows."""
        lib = self._require_hip()
        dev = self._flat.device
        rows_t, items_t = index_tensor(rows, dev), index_tensor(items, dev)
        if rows_t.numel() != items_t.numel():
            raise ValueError("rows and items differ in length")
        n, n_rows = rows_t.numel(), hd.shape[0]
        out = torch.empty(n, dtype=torch.float32, device=dev)
        if n == 0:
            return out
        stats = self._device_stats()
        ws = self.workspace(lib, lib.hiprec_vaecf_decode_workspace_bytes(ctypes.byref(self.shape), n_rows))
        _lib.check(lib.hiprec_vaecf_decode_at(
            ctypes.byref(self.shape), _lib.ptr(self._flat), _lib.ptr(hd), n_rows, _lib.ptr(rows_t), _lib.ptr(items_t), n,
            _lib.ptr(out), None, _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)))
        self._check_status()
        return out

    # ---- reference API -----------------------------------------------------------------------------------------
    def encode(self, x):
        """vaecf.py:45-47 on a dense batch or a CSR triple: ``mu`` ``[B, z_dim]`` and the decoder's last hidden
        activation at ``z = mu``, ``[B, hidden[0]]`` (where the reference returns ``logvar``, which inference never
        uses: a training step keeps it on the device)."""
        row_ptr, items, values, B, nnz = _as_csr(x, self.n_items, self._flat.device)
        return self._encode_csr(row_ptr, items, values, B, nnz)

    def decode(self, hd, rows, items):
        """The entries ``(rows[k], items[k])`` of what vaecf.py:49-54 returns as a dense matrix, from ``hd =
        encode(x)[1]``: softmax over the catalogue for ``mult``, sigmoid otherwise."""
        return self._decode_at(hd, rows, items)

    def reparameterize(self, mu, logvar):
        """vaecf.py:56-59 with this model's noise source (``next_noise``, ``noise_rng``)."""
        eps = self._noise(mu.shape[0]).to(mu.device)
        return mu + eps * torch.exp(0.5 * logvar)

    def forward(self, x, beta=1.0):
        """The batch loss ``mean(beta kld - ll)`` as a 0-dim tensor, ``kld`` / ``ll`` set (no autograd graph and no
        dense reconstruction: training goes through ``VAECFEngine.train_single_batch``)."""
        lib = self._require_hip()
        dev = self._flat.device
        stats = self._device_stats()
        if self._fwd is None or self._fwd[0].device != dev:
            self._fwd = (torch.zeros_like(self._flat),
                         torch.zeros(lib.hiprec_scratch_bytes(0), dtype=torch.uint8, device=dev))
        g, scratch = self._fwd
        g.zero_()
        self.enqueue_grad(lib, g, x, beta, stats, scratch)
        _lib.check(lib.hiprec_finalize_stats(_lib.ptr(stats), _lib.ptr(scratch), None, None, _lib.stream_ptr(dev)))
        return torch.tensor(self._set_losses(self._check_status(), beta), device=dev)

    def set_history(self, history, binarise=True):
        """Each user's interaction row, for ``score`` / ``ranking_factors``: a scipy sparse ``[n_users, n_items]`` matrix
        or ``(user_ptr, items[, values])``."""
        self._history = _history_csr(history, self.n_users, self._flat.device, binarise)

    def _require_history(self):
        if self._history is None:
            raise NotImplementedError("VAECF ranks a user from the user's interaction row: call set_history(matrix) or "
                                      "train an epoch first")
        return self._history

    def ranking_factors(self):
        """``(Hd(mu(x_u)) for every user, decoder's last weight, 1.0, its bias)`` for full-catalogue ranking
        (``recommend.recommend``, ``eval.evaluate_full``): ranking by logit is ranking by softmax or sigmoid."""
        ptr, items, values = self._require_history()
        _, hd = self._encode_csr(ptr, items, values, self.n_users, items.numel())
        last = getattr(self.decoder, f"fc{len(self.hidden)}")
        return hd, last.weight.data, 1.0, last.bias.data

    def score(self, users, items):
        """The decoded probability of ``items[k]`` for ``users[k]``, each user encoded from the history row."""
        ptr, h_items, h_values = self._require_history()
        dev = self._flat.device
        users_t, items_t = index_tensor(users, dev), index_tensor(items, dev)
        if users_t.numel() != items_t.numel():
            raise ValueError("users and items differ in length")
        if users_t.numel() == 0:
            return torch.empty(0, dtype=torch.float32, device=dev)
        if int(users_t.min()) < 0 or int(users_t.max()) >= self.n_users:
            raise IndexError("index out of range in self (user index)")
        uniq, inverse = torch.unique(users_t, return_inverse=True)
        starts, lens = ptr[uniq], ptr[uniq + 1] - ptr[uniq]
        row_ptr = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=dev)
        row_ptr[1:] = torch.cumsum(lens, 0)
        take = (torch.arange(int(row_ptr[-1]), device=dev) - torch.repeat_interleave(row_ptr[:-1], lens)
                + torch.repeat_interleave(starts, lens))
        sub_items, sub_values = h_items[take].contiguous(), h_values[take].contiguous()
        _, hd = self._encode_csr(row_ptr, sub_items, sub_values, uniq.numel(), sub_items.numel())
        return self._decode_at(hd, inverse, items_t)

    def predict(self, user_idx, item_idx):
        """vaecf.py:89-108, literally (see "kept on purpose"): row 0 of ``x_u`` holds the query pairs of user 0,
        duplicates summed; the result is row 0's decoded probabilities at ``item_idx``."""
        dev = self._flat.device
        users = np.asarray(user_idx.cpu() if torch.is_tensor(user_idx) else user_idx, dtype=np.int64).reshape(-1)
        items = np.asarray(item_idx.cpu() if torch.is_tensor(item_idx) else item_idx, dtype=np.int64).reshape(-1)
        if users.shape != items.shape:
            raise ValueError("user_idx and item_idx differ in length")
        if users.size and (users.min() < 0 or users.max() >= self.n_users):
            raise IndexError("index out of range in self (user index)")
        if items.size and (items.min() < 0 or items.max() >= self.n_items):
            raise IndexError("index out of range in self (item index)")
        row0, counts = np.unique(items[users == 0], return_counts=True)
        _, hd = self._encode_csr(torch.tensor([0, len(row0)], dtype=torch.int64, device=dev),
                                 torch.as_tensor(row0, dtype=torch.int64).to(dev),
                                 torch.as_tensor(counts.astype(np.float32)).to(dev), 1, len(row0))
        return self._decode_at(hd, np.zeros(len(items), dtype=np.int64), items)


class _Csr(tuple):
    """A batch already on the device: ``(row_ptr, items, values, B, nnz)``."""

    def __new__(cls, *fields):
        return super().__new__(cls, fields)


class VAECFEngine(FlatModelEngine):
    """models/vaecf.py:111-167."""

    def __init__(self, config):
        self.config = config
        mc = config["model"]
        hidden = [int(h) for h in _get(mc, "hidden", [20])]
        self.model = VAE(z_dim=int(_get(mc, "z_dim", 10)), ae_structure=[mc["n_items"]] + hidden, config=mc)
        self.batch_size = mc["batch_size"]
        self.n_users = mc["n_users"]
        self.n_items = mc["n_items"]
        self.lr = mc["lr"]
        self.beta = mc["beta"]
        self.wd = mc["weight_decay"]
        self._epoch_cache = None
        super(VAECFEngine, self).__init__(config)

    def set_optimizer(self):
        """vaecf.py:128-130: Adam(lr, weight_decay), whatever ``config["model"]["optimizer"]`` says."""
        self.optimizer = HipOptimizer("adam", self.lr)
        self.optimizer.defaults["weight_decay"] = self.wd
        self.optimizer.param_groups = [dict(self.optimizer.defaults)]

    def _alloc_extra(self, lib, dev):
        m = self.model
        if lib.hiprec_vaecf_param_floats(ctypes.byref(m.shape)) != m.flat.numel():
            raise RuntimeError("the flat VAECF buffer is not laid out as libhiprec.so expects; rebuild the library")
        self._sumsq_ws = torch.zeros(lib.hiprec_sumsq_workspace_bytes() // 8, dtype=torch.float64, device=dev)

    def _enqueue_grad(self, batch_data):
        lib = self._setup()
        self.model.enqueue_grad(lib, self._g_flat, batch_data, self.beta, self._stats, self._scratch)

    def _enqueue_opt(self, fold_partials=True):
        """optimizer.step(): the plain sweep, or with ``weight_decay * w`` added to every element's gradient inside it
        (torch.optim.Adam's L2 form)."""
        if not self.wd:
            return super()._enqueue_opt(fold_partials)
        lib, m, opt = _lib.load(), self.model, self.optimizer
        _lib.check(lib.hiprec_opt_dense_step_decay(
            opt.kind, _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(opt.exp_avg), _lib.ptr(opt.exp_avg_sq),
            m.flat.numel(), opt.lr, opt.beta1, opt.beta2, opt.eps, _lib.ptr(self._stats),
            _lib.ptr(self._scratch) if fold_partials else None, float(self.wd), _lib.ptr(self._sumsq_ws),
            self._sumsq_ws.numel() * 8, _lib.stream_ptr(m.flat.device)))

    def backward_only(self, batch_data):
        """zero_grad + forward + loss + backward without the optimizer step: ``(loss, grads)`` -- the gradients as they
        stand at ``optimizer.step`` (the weight decay is the optimizer's); ``model.ll`` and ``model.kld`` are set."""
        self._enqueue_grad(batch_data)
        st, grads = self._finish_backward_only()
        return self.model._set_losses(st, self.beta), grads

    def forward(self, batch_data):
        return self.model.forward(batch_data, self.beta)

    def encode(self, x):
        return self.model.encode(x)

    def decode(self, hd, rows, items):
        return self.model.decode(hd, rows, items)

    def reparameterize(self, mu, logvar):
        return self.model.reparameterize(mu, logvar)

    def train_single_batch(self, batch_data, ratings=None):
        """vaecf.py:134-142: one step, returns ``batch_loss.item()``."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        self._enqueue_step(batch_data)
        return self.model._set_losses(self._sync_stats(), self.beta)

    def _epoch_rows(self, user_indices, matrix):
        """The epoch's rows in visiting order as ONE device CSR, uploaded once per matrix object."""
        m = self.model
        dev = m.flat.device
        uids = np.asarray(user_indices, dtype=np.int64).reshape(-1)
        c = self._epoch_cache
        if c is None or c[0] is not matrix or c[1].device != dev:
            history = _history_csr(matrix, m.n_users, dev)
            c = self._epoch_cache = (matrix, history[0], history, None, None)
            m._history = history                       # remembered as the model's history
        if c[3] is None or not np.array_equal(c[3], uids):
            ptr, items, values = c[2]
            if uids.size and (uids.min() < 0 or uids.max() >= m.n_users):
                raise IndexError("index out of range in self (user index)")
            if np.array_equal(uids, np.arange(m.n_users)):
                rows = (ptr, items, values)
            else:
                u = torch.as_tensor(uids).to(dev)
                starts, lens = ptr[u], ptr[u + 1] - ptr[u]
                row_ptr = torch.zeros(u.numel() + 1, dtype=torch.int64, device=dev)
                row_ptr[1:] = torch.cumsum(lens, 0)
                take = (torch.arange(int(row_ptr[-1]), device=dev) - torch.repeat_interleave(row_ptr[:-1], lens)
                        + torch.repeat_interleave(starts, lens))
                rows = (row_ptr, items[take].contiguous(), values[take].contiguous())
            c = self._epoch_cache = (c[0], c[1], c[2], uids.copy(), rows)
        return c[4]

    def train_an_epoch(self, train_loader, epoch_id):
        """vaecf.py:144-167: contiguous batches of ``user_indices``, the matrix binarised, every step enqueued back to
        back with ONE host sync at the end; prints and logs the sum of the batch losses as the reference does."""
        assert hasattr(self, "model"), "Please specify the exact model !"
        user_indices, matrix = train_loader
        row_ptr, items, values = self._epoch_rows(user_indices, matrix)
        n, nnz = row_ptr.numel() - 1, items.numel()
        batches = [_Csr(row_ptr[s:min(s + self.batch_size, n) + 1], items, values, min(s + self.batch_size, n) - s, nnz)
                   for s in range(0, n, self.batch_size)]
        st = self._run_epoch(batches)
        self.model._set_losses(st, self.beta)              # the last batch's
        total_loss = self.beta * st.reg_sum - st.loss_sum
        print(f"[Training Epoch {epoch_id}], Loss {total_loss}")
        self.writer.add_scalar("model/loss", total_loss, epoch_id)
