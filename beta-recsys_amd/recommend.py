"""Top-K recommendation over the whole catalogue (csrc/topk.hip).

``recommend(model, users, k, seen=None)`` turns a trained model into ranked lists: every item is scored against the
query users in one fused pass (``hiprec_topk_recommend``), the items a user has already interacted with are masked, and
only the ``k`` best per user ever leave the CU -- the dense ``[users, items]`` score matrix is never built.  It serves
the models whose score is bilinear in a user row and an item row, through their ``ranking_factors()`` hook.

There is no counterpart in the reference (its only scoring entry point is ``predict(users, items)``), and there is no
CPU fallback: the arithmetic runs in libhiprec.so on the GPU or not at all.
"""
import torch

from . import _lib
from ._stats import _new_stats, clear_status, raise_on_status, read_stats
from .data import build_positive_csr
from .flat_engine import index_tensor

MAX_K = 128        # HIPREC_TOPK_MAX_K
MAX_DIM = 512      # HIPREC_TOPK_MAX_DIM

_stats = {}


class SeenCsr(tuple):
    """``(user_ptr, pos_sorted)`` that :func:`normalise_seen` has checked and placed on the device: handed back in as
    ``seen`` it is taken as it is (no checks, no host sync), so a caller that recommends repeatedly normalises once."""


def ranking_factors(model):
    """``(U, I, alpha, item_bias | None)`` of a model with the hook; NotImplementedError (with the model's own reason, or
    that it has no hook) otherwise."""
    hook = getattr(model, "ranking_factors", None)
    if hook is None:
        raise NotImplementedError(f"{type(model).__name__} has no ranking_factors(): full-catalogue ranking needs a score "
                                  "that is a dot product of a user row and an item row")
    return hook()


def normalise_seen(seen, n_users, n_items, device):
    """``seen`` as the kernel takes it: ``None`` or ``(user_ptr[n_users + 1], pos_sorted)`` int64 on ``device``.

    Accepted: ``None``; a ``(user_ptr, pos_sorted)`` pair (what ``data.build_positive_csr`` returns: recognised by
    ``len(user_ptr) == n_users + 1`` and ``user_ptr[-1] == len(pos_sorted)``, and by its first entry being 0); or a
    ``(users, items)`` pair of id columns of equal length, which goes through ``build_positive_csr``."""
    if seen is None:
        return None
    if isinstance(seen, SeenCsr) and seen[0].device == torch.device(device) and seen[0].numel() == n_users + 1:
        return seen
    if not isinstance(seen, (tuple, list)) or len(seen) != 2:
        raise ValueError("seen must be None, a (user_ptr, pos_sorted) pair or a (users, items) pair of id columns")
    a, b = index_tensor(seen[0], device), index_tensor(seen[1], device)
    if a.numel() == n_users + 1 and a.numel() != b.numel():
        is_csr = True
    elif a.numel() == n_users + 1:     # both readings have the right lengths: a CSR's pointer starts at 0 and ends at nnz
        is_csr = int(a[0]) == 0 and int(a[-1]) == b.numel() and bool((a[1:] >= a[:-1]).all())
    else:
        is_csr = False
    if is_csr:
        if int(a[0]) != 0 or int(a[-1]) != b.numel() or bool((a[1:] < a[:-1]).any()):
            raise ValueError("seen: user_ptr must start at 0, never decrease and end at len(pos_sorted)")
        if b.numel() and (int(b.min()) < 0 or int(b.max()) >= n_items):
            raise IndexError("seen: pos_sorted holds an item id outside [0, n_items)")
        return SeenCsr((a, b))
    if a.numel() != b.numel():
        raise ValueError(f"seen: users and items differ in length ({a.numel()}, {b.numel()}), and the first is no "
                         f"user_ptr of {n_users + 1} entries")
    return SeenCsr(build_positive_csr(a, b, int(n_users), int(n_items)))


def topk_factors(U, I, alpha, item_bias, users, k, seen=None, item_splits=0):
    """The kernel call on explicit factors: ``U [n_users, D]`` / ``I [n_items, D]`` fp32 device tensors whose rows are
    contiguous (a column slice of a wider buffer is fine), ``item_bias`` ``[n_items]`` or None.  Returns
    ``(items[n, k] int64, scores[n, k] fp32)`` on the device; raises IndexError for a query id outside the table."""
    k, item_splits = int(k), int(item_splits)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in 1..{MAX_K}, got {k}")
    if U.dim() != 2 or I.dim() != 2 or U.shape[1] != I.shape[1]:
        raise ValueError(f"user / item factors must be [n, D] with one D, got {tuple(U.shape)} and {tuple(I.shape)}")
    dim = int(U.shape[1])
    if not 1 <= dim <= MAX_DIM:
        raise ValueError(f"factor width must be in 1..{MAX_DIM}, got {dim}")
    if item_splits < 0:
        raise ValueError(f"item_splits must be >= 0, got {item_splits}")
    dev = U.device
    if dev.type != "cuda" or I.device != dev:
        raise RuntimeError("hiprec recommendation runs on an MI355X through libhiprec.so; factors are on "
                           f"{U.device} / {I.device} and there is deliberately no CPU fallback")
    if U.dtype != torch.float32 or I.dtype != torch.float32:
        raise TypeError("factors must be fp32")
    if U.stride(1) != 1:
        U = U.contiguous()
    if I.stride(1) != 1:
        I = I.contiguous()
    n_users, n_items = int(U.shape[0]), int(I.shape[0])
    if n_users < 1 or n_items < 1:
        raise ValueError("empty factor table")
    ldu = int(U.stride(0)) if n_users > 1 else dim
    ldi = int(I.stride(0)) if n_items > 1 else dim
    if item_bias is not None:
        item_bias = item_bias.to(dev, torch.float32).reshape(-1).contiguous()
        if item_bias.numel() != n_items:
            raise ValueError("item_bias must hold one value per item")
    csr = normalise_seen(seen, n_users, n_items, dev)
    lib = _lib.load()
    users_t = index_tensor(users, dev)
    n = users_t.numel()
    out_items = torch.empty((n, k), dtype=torch.int64, device=dev)
    out_scores = torch.empty((n, k), dtype=torch.float32, device=dev)
    if n == 0:
        return out_items, out_scores
    key = (dev.type, dev.index)
    if key not in _stats:
        _stats[key] = _new_stats(dev)
    stats = _stats[key]
    ws_bytes = lib.hiprec_topk_workspace_bytes(n, n_items, k, item_splits)
    workspace = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    _lib.check(lib.hiprec_topk_recommend(
        _lib.ptr(U), ldu, n_users, _lib.ptr(I), ldi, n_items, dim, float(alpha), _lib.ptr(item_bias),
        _lib.ptr(users_t), n, _lib.ptr(csr[0]) if csr else None, _lib.ptr(csr[1]) if csr else None, k, item_splits,
        _lib.ptr(workspace), ws_bytes, _lib.ptr(out_items), _lib.ptr(out_scores), _lib.ptr(stats),
        _lib.stream_ptr(dev)))
    st = read_stats(stats)
    if st.status:
        clear_status(stats)
        err = None
        try:
            raise_on_status(st.status)
        except IndexError as exc:
            err = exc
        err.partial = (out_items, out_scores)   # the rows of the in-range users are complete
        raise err
    return out_items, out_scores


def recommend(model, users, k, seen=None, item_splits=0):
    """``(items[n, k] int64, scores[n, k] fp32)`` on the device: for every query user the ``k`` best items of the whole
    catalogue by the model's ranking score, best first (ties to the lower item id), never an item of the user's ``seen``
    row; a user with fewer than ``k`` unseen items gets ``-1`` / ``-inf`` in the tail.

    ``model``: a model with ``ranking_factors()`` (MF, LightGCN, NGCF, UltraGCN) or an engine holding one; a model that
    defines ``topk_items(users, k, seen, item_splits)`` (ItemKNN, UserKNN: csrc/knn.hip) is ranked through that instead.
    ``seen``: None, a ``(user_ptr, pos_sorted)`` pair or a ``(users, items)`` pair of id columns (the training frame);
    what :func:`normalise_seen` returns is taken without being checked again.
    ``item_splits``: into how many item ranges the catalogue is cut to fill the chip (0 = chosen by the library); the
    result does not depend on it."""
    engine = model if hasattr(model, "model") and not hasattr(model, "ranking_factors") else None
    if engine is not None:
        flush = getattr(engine, "flush_lazy", None)
        if flush is not None:
            flush()                    # a lazy optimizer's lagging rows, as predict does
        model = engine.model
    hook = getattr(model, "topk_items", None)     # a model that ranks by its own kernel (the neighbourhood models)
    if hook is not None:
        return hook(users, k, seen, item_splits)
    U, I, alpha, bias = ranking_factors(model)
    return topk_factors(U, I, alpha, bias, users, k, seen, item_splits)
