"""The device ``hiprec_stats`` block as the host sees it: make one, read it back, clear or raise its status word.

Every model, engine and stand-alone kernel wrapper of the package goes through these four; they depend on ``_lib``
alone, so the model / engine modules can import them without importing each other.
"""
import ctypes

import torch

from . import _lib


def _new_stats(device, beta1=0.9, beta2=0.999):
    lib = _lib.load()
    stats = torch.zeros(ctypes.sizeof(_lib.Stats), dtype=torch.uint8, device=device)
    _lib.check(lib.hiprec_stats_reset(_lib.ptr(stats), beta1, beta2, _lib.stream_ptr(device)))
    return stats


def read_stats(stats_tensor):
    """Copy the device hiprec_stats block to the host (synchronises) and decode it."""
    raw = stats_tensor.cpu().numpy().tobytes()
    return _lib.Stats.from_buffer_copy(raw)


def clear_status(stats):
    """Zero the 4-byte status word of a device hiprec_stats -- and only that: the struct also holds the optimizer
    clock and the epoch sums, which kernels of other streams may be advancing (writing back a host copy of
    the whole struct raced them)."""
    off = _lib.Stats.status.offset
    stats[off:off + 4].zero_()


def raise_on_status(status):
    """Turn sticky device status bits into the IndexError PyTorch would have raised."""
    if status:
        which = []
        if status & _lib.STATUS_USER_OOB:
            which.append("user")
        if status & _lib.STATUS_ITEM_OOB:
            which.append("item")
        if status & _lib.STATUS_ROW_OOB:
            which.append("row")
        if status & _lib.STATUS_TIME_OOB:
            which.append("time step")
        if status & _lib.STATUS_NEG_EXHAUSTED:
            raise ValueError("Sample larger than population or is negative")  # random.sample's message
        if status & _lib.STATUS_LAZY_TABLE:
            raise RuntimeError(
                "lazy Adam: the optimizer ran past the bias-correction table while the corrections still moved "
                "(non-default betas?): use config['model']['dense_opt'] = 'sweep'")
        if status & _lib.STATUS_TABLE_FULL:
            raise RuntimeError(
                "a batch's row-contribution hash partition overflowed while the epoch was staged: the step's lists are "
                "incomplete (should be impossible at >= 4 table entries per triple; please report the batch)")
        if status & _lib.STATUS_ROUTE_OVERFLOW:
            raise RuntimeError(
                "a fixed-capacity all-to-all bucket overflowed: raise the sharded engine's "
                "`route_slack` (config['model']['route_slack'])")
        raise IndexError("index out of range in self (" + "/".join(which) + " index)")
