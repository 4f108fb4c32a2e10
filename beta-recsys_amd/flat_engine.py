"""The flat-parameter model base and the engine plumbing built around it.

``_FlatModel`` keeps every parameter of a model in ONE flat fp32 buffer; ``FlatModelEngine`` serves the engines that
train such a model: LightGCN, NGCF, PairwiseGMF, Triple2vec and UltraGCN, whose step is ``<model>_grad`` + a dense
optimizer sweep over that buffer, NeuMF / GMF / MLP (``ncf.py``), whose step is the one call ``hiprec_ncf_step``, and
MF (``mf.py``), which adds its resident-epoch drivers, the touched-rows SGD and the lazy Adam / RMSprop state.

Nothing here has a counterpart in the reference (it has no such layer): the subclasses mirror
``beta_rec.models.*Engine``; this base only owns the device-side step state (dense gradient, optimizer
moments, ``hiprec_stats``, scratch) and the things every one of them does with it.
"""
import numpy as np
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import _lib
from ._stats import _new_stats, clear_status, raise_on_status, read_stats
from .torch_engine import ModelEngine


def index_tensor(x, device):
    """Ids as the kernels take them: a contiguous 1-D int64 tensor on ``device``, from a list, a numpy array of any
    integer dtype or a tensor on any device (flattened; a caller that needs ``[B, N]`` reshapes afterwards)."""
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x), dtype=torch.int64)
    return x.to(device, torch.int64).reshape(-1).contiguous()


class _ParamView(nn.Module):
    """A module whose parameters (``weight`` and optionally ``bias``) are views of a flat buffer."""

    def __init__(self, weight, bias=None):
        super().__init__()
        self.weight = Parameter(weight, requires_grad=False)
        if bias is not None:
            self.bias = Parameter(bias, requires_grad=False)

    def extra_repr(self):
        return "x".join(str(s) for s in self.weight.shape)


class _FlatModel(nn.Module):
    """Base: named parameter views over ONE flat fp32 buffer (tables first, dense layers after)."""

    _stats = None   # hiprec_stats of the model's own calls (forward / predict), made on first use

    def _build(self, spec):
        """spec: list of (name, shape); allocates the flat buffer and returns the views by name."""
        self._spec = [(n, tuple(s)) for n, s in spec]
        sizes = [int(np.prod(s)) for _, s in self._spec]
        self._offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self._flat = torch.zeros(int(self._offsets[-1]), dtype=torch.float32)
        return self.views()

    def views(self, flat=None):
        flat = self._flat if flat is None else flat
        return {n: flat[self._offsets[k]:self._offsets[k + 1]].view(*s)
                for k, (n, s) in enumerate(self._spec)}

    def offset_of(self, name):
        return int(self._offsets[[n for n, _ in self._spec].index(name)])

    def _owner(self, name):
        mod = self
        parts = name.split(".")
        for p in parts[:-1]:
            mod = getattr(mod, p) if not p.isdigit() else mod[int(p)]
        return mod, parts[-1]

    def _rebind(self, flat):
        self._flat = flat
        for name, view in self.views(flat).items():
            mod, attr = self._owner(name)
            getattr(mod, attr).data = view

    def _apply(self, fn, recurse=True):
        new_flat = fn(self._flat)
        if new_flat.dtype != torch.float32:
            raise TypeError("hiprec models keep fp32 parameters (the reference trains in fp32)")
        if new_flat is not self._flat:
            self._rebind(new_flat.contiguous())
        return self

    @property
    def flat(self):
        return self._flat

    def _require_hip(self):
        if self._flat.device.type != "cuda":
            raise RuntimeError(
                "hiprec models compute on an MI355X through libhiprec.so only; parameters are "
                f"on {self._flat.device} and there is deliberately no CPU fallback")
        return _lib.load()

    def _device_stats(self):
        """The stats block on the flat buffer's device (a new one when the model has moved)."""
        dev = self._flat.device
        if self._stats is None or self._stats.device != dev:
            self._stats = _new_stats(dev)
        return self._stats

    def _check_status(self):
        """The host sync of a model call; out-of-range ids surface here as IndexError (the block with the raised
        status word is dropped, so the next call starts from a clean one)."""
        s = read_stats(self._stats)
        if s.status:
            self._stats = None
            raise_on_status(s.status)
        return s


class FlatModelEngine(ModelEngine):
    """Subclasses implement ``_enqueue_grad(batch)`` (zero_grad + forward + loss + backward into
    ``self._g_flat``, loss partials into ``self._scratch``), or replace ``_enqueue_step`` as a whole."""

    _ready = False
    # data-parallel replicas (replicated.replicated_flat_engine) set these: every rank works on its share of the
    # global batch, and a batch MEAN becomes 1 / (local batch x world) so that the sum over ranks is the reference's
    # gradient on the whole batch
    _dp_world = 1
    _dp_rank = 0

    def _batch_share(self):
        return 1.0 / self._dp_world

    def _alloc_extra(self, lib, device):
        """Hook: model-specific workspaces (called once per device, after the common buffers exist)."""

    def _setup(self):
        lib = self.require_hip()
        flat = self.model.flat
        if self._ready and self._g_flat.device == flat.device:
            return lib
        dev = flat.device
        self._g_flat = torch.zeros_like(flat)
        self.optimizer.allocate_state(flat)
        self._scratch = torch.zeros(lib.hiprec_scratch_bytes(0), dtype=torch.uint8, device=dev)
        self._stats = _new_stats(dev, self.optimizer.beta1 or 0.9, self.optimizer.beta2 or 0.999)
        self._alloc_extra(lib, dev)
        self._ready = True
        return lib

    def _sweep_floats(self):
        """How many leading floats of the flat buffers the optimizer moves (all of them by default)."""
        return self.model.flat.numel()

    def _enqueue_opt(self, fold_partials=True, scalar_index=-1):
        """optimizer.step(): the dense sweep, which also folds the loss partials into the stats (unless the caller
        has done that already) and leaves the gradient cleared.  ``scalar_index``: the element whose gradient travels
        in those partials (MF's ``global_bias``), -1 for none."""
        lib, m, opt = _lib.load(), self.model, self.optimizer
        _lib.check(lib.hiprec_opt_dense_step(
            opt.kind, _lib.ptr(m.flat), _lib.ptr(self._g_flat), _lib.ptr(opt.exp_avg),
            _lib.ptr(opt.exp_avg_sq), self._sweep_floats(), opt.lr, opt.beta1, opt.beta2, opt.eps,
            _lib.ptr(self._stats), _lib.ptr(self._scratch) if fold_partials else None, scalar_index,
            _lib.stream_ptr(m.flat.device)))

    def _enqueue_step(self, batch_data):
        self._enqueue_grad(batch_data)
        self._enqueue_opt()

    def _drop_step_state(self):
        """What a step that skipped flagged rows leaves half-done: the partially accumulated gradient."""
        self._g_flat.zero_()

    def _sync_stats(self):
        """The one host sync of a step / epoch; out-of-range ids surface here as IndexError (the sticky
        status word is cleared and a partially accumulated gradient dropped, so the engine stays usable)."""
        st = read_stats(self._stats)
        if st.status:
            clear_status(self._stats)
            self._drop_step_state()
            raise_on_status(st.status)
        return st

    def _finish_backward_only(self, partial_grad=None):
        """After ``_enqueue_grad``: reduce the loss partials without an optimizer call, hand out a copy of
        the gradient and clear it.  Returns ``(stats, grads)``.  ``partial_grad``: pointer to the gradient slot of a
        parameter whose gradient travels in the scratch partials (NCF's ``affine_output.bias``)."""
        lib = _lib.load()
        _lib.check(lib.hiprec_finalize_stats(_lib.ptr(self._stats), _lib.ptr(self._scratch), partial_grad, None,
                                             _lib.stream_ptr(self.model.flat.device)))
        st = self._sync_stats()
        grads = {k: v.clone() for k, v in self.model.views(self._g_flat).items()}
        self._g_flat.zero_()
        return st, grads

    def backward_only(self, batch_data):
        """zero_grad + forward + loss + backward without the optimizer step: ``(loss, grads)``."""
        self._enqueue_grad(batch_data)
        st, grads = self._finish_backward_only()
        return st.loss, grads

    def _epoch_step(self, batch):
        """Hook: one step of the python-looped epoch from one item of the loader."""
        self._enqueue_step(batch)

    def _run_epoch(self, train_loader):
        """The python-looped epoch: every step enqueued back to back, ONE host sync at the end.  Returns the stats
        (``loss``: the last batch's, ``loss_sum``: the epoch's)."""
        self.model.train()
        lib = self._setup()
        _lib.check(lib.hiprec_stats_begin_epoch(_lib.ptr(self._stats), _lib.stream_ptr(self.model.flat.device)))
        for batch in train_loader:
            self._epoch_step(batch)
        return self._sync_stats()

    @staticmethod
    def _check_blocks(sizes, batch_size, what="batch_size triples"):
        """The C epoch drivers cut a resident epoch into steps of ``batch_size`` rows, so the collected batches must
        tile it the same way: every batch but the last holds ``batch_size`` rows, the last no more."""
        if any(n != batch_size for n in sizes[:-1]) or sizes[-1] > batch_size:
            raise ValueError(f"every batch but the last must hold {what}")

    def load_optimizer_state(self, step, exp_avg=None, exp_avg_sq=None):
        """Resume from a reference optimizer state: step count + per-parameter moment dicts keyed like
        ``state_dict`` (``exp_avg_sq`` doubles as RMSprop's ``square_avg``); ``None`` zeroes a moment."""
        lib = self._setup()
        opt, m = self.optimizer, self.model
        dev = m.flat.device
        _lib.check(lib.hiprec_stats_reset(_lib.ptr(self._stats), opt.beta1 or 0.9, opt.beta2 or 0.999,
                                          _lib.stream_ptr(dev)))
        _lib.check(lib.hiprec_stats_set_step(_lib.ptr(self._stats), int(step), opt.beta1 or 0.9,
                                             opt.beta2 or 0.999, _lib.stream_ptr(dev)))
        for buf, src in ((opt.exp_avg, exp_avg), (opt.exp_avg_sq, exp_avg_sq)):
            if buf is None:
                continue
            if src is None:
                buf.zero_()
                continue
            for name, view in m.views(buf).items():
                view.copy_(torch.as_tensor(src[name], dtype=torch.float32).reshape(view.shape))
