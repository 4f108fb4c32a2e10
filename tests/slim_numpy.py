"""SLIM (Ning and Karypis 2011) restated in numpy: the oracle of csrc/slim.hip (the reference has no counterpart).

    X = [frame > 0]      G = X^T X      A = G + l2 I
    column w = W[:, j] minimises  1/2 w^T A w - G[:, j]^T w + l1 sum |w_k|   with w_j = 0 and, in positive mode, w >= 0

``coordinate_descent`` is the kernel's schedule: cyclic sweeps over ``k = 0 .. n-1`` in ascending order from ``w = 0``,
``q = A w`` kept up to date, a column frozen after the first sweep whose largest ``|d|`` is ``<= tol``.  All columns
advance together, one ``k`` at a time (coordinate ``k`` of every column that still runs is one row of ``W``), so a sweep
is ``n`` rank-1 updates.  Every operation is one rounded operation of ``dtype`` in the kernel's order:

    positive   g = (q_k - G_kj) + l1            w_new = max(0, w_k - g / A_kk)
    signed     r = G_kj - (q_k - A_kk w_k)      w_new = sign(r) max(0, |r| - l1) / A_kk
    d = w_new - w_k;   if d != 0:  q = q + d * A[:, k]  (a product, then a sum: no fma)  and  w_k = w_new

``W64`` (float64, run until the KKT violation is ``<= 1e-10``) is the truth the GPU is held to; ``W32`` (float32 at the
case's ``tol`` and ``max_sweeps``) is the yardstick, whose distance from the truth is what stopping at ``tol`` costs.

The named defects are the mistakes a kernel for this model can make; tests/test_slim_host.py shows that each lands
outside the bound the GPU test applies.
"""
import functools

import numpy as np

import ease_numpy as en

CHUNK = 64            # HIPREC_SLIM_CHUNK (tests/test_slim_host.py holds it to the header)
BLOCK = 256           # threads of the kernel's workgroup
REL = 1e-5            # the project's relative bound (tests/helpers.py)
KKT64 = 1e-10         # what W64 is run to
EMPTY_USER = en.EMPTY_USER
DEFECTS = ("no_l1", "no_l2_in_denominator", "stale_q", "diagonal_free", "descending_one_sweep", "counts_not_binary",
           "no_clamp")
TOL = 1e-6
MAX_SWEEPS = 100
DEFECT_SWEEPS = 50

# name -> (frame, l1, l2, positive_only, tol, max_sweeps, lds_cap); frame = a fixture of tests/ease_numpy.py (its
# popularity-skewed frames with multiplicities up to 3, one empty user and one empty item) or "pair" (below);
# lds_cap = 0 leaves w and q to the library (LDS here)
FIXTURES = {
    "n1": ("n1", 1.0, 1.0, True, TOL, MAX_SWEEPS, 0),
    "n2": ("pair", 0.5, 1.0, True, TOL, MAX_SWEEPS, 0),
    "n15": ("n15", 1.0, 1.0, True, TOL, MAX_SWEEPS, 0),
    "n17": ("n17", 0.5, 10.0, True, TOL, MAX_SWEEPS, 0),
    "chunk_minus": ("panel_minus", 1.0, 1.0, True, TOL, MAX_SWEEPS, 0),
    "chunk": ("panel", 0.5, 10.0, True, TOL, MAX_SWEEPS, 0),
    "chunk_plus": ("panel_plus", 1.0, 1.0, True, TOL, MAX_SWEEPS, 0),
    "l1_zero": ("two_panels_ragged", 0.0, 5.0, True, TOL, MAX_SWEEPS, 0),
    "signed": ("panel_plus", 1.0, 1.0, False, TOL, MAX_SWEEPS, 0),
    "block_plus": ("ws_path", 1.0, 1.0, True, TOL, MAX_SWEEPS, 0),         # 261 = 256 + 5: more than a block, ragged
    "ws_path": ("ws_path", 0.5, 10.0, True, TOL, MAX_SWEEPS, 256),         # 261 > lds_cap: w and q in the workspace
    "all_zero": ("n17", 1000.0, 1.0, True, TOL, MAX_SWEEPS, 0),            # l1 above every count: W = 0 after one sweep
}
SUPPORT = tuple(name for name, f in FIXTURES.items() if f[1] >= 0.5)       # the fixtures of the support test

# the two-item frame: both items touched and co-occurring (ease_numpy's n2 leaves its second item untouched, which
# makes W all zeros); user 1 is empty, multiplicities up to 3
PAIR = np.array([[3, 1], [0, 0], [1, 0], [2, 2], [0, 1], [1, 1]], dtype=np.int64)


def gram(X, l2, dtype=np.float64):
    """``(A, G)``: ``G = X^T X`` (integer counts: exact in either dtype below 2^24) and ``A = G + l2 I``."""
    X = np.asarray(X)
    counts = X.astype(np.int64).T @ X.astype(np.int64)
    G = counts.astype(dtype)
    A = G.copy()
    A[np.diag_indices_from(A)] += dtype(l2)
    return A, G


def coordinate_descent(A, l1, positive_only, tol, max_sweeps, dtype=np.float64, l2=None, defect=None, screen=False):
    """The schedule above on the symmetric matrix ``A`` in ``dtype`` arithmetic.  Returns a dict: ``W``, ``sweeps``
    (per column), ``converged`` (per column), ``dmax_last`` and ``dmax_prev`` (the largest ``|d|`` of a column's last
    sweep and of the one before: what decided its count).  ``screen=True`` applies the positive mode's screening rule
    (a coordinate with ``G_kj <= l1`` is never visited).  ``l2`` is needed by the defect that forgets it
    (``no_l2_in_denominator``: the update in its residual form divided by ``G_kk``; the gradient form's fixed point does
    not depend on the divisor, this one's does)."""
    assert defect is None or defect in DEFECTS, defect
    A = np.ascontiguousarray(A, dtype=dtype)
    n = A.shape[0]
    l1 = dtype(0.0 if defect == "no_l1" else l1)
    tol = dtype(tol)
    diag = np.diag(A).copy()
    if defect == "no_l2_in_denominator":
        diag = diag - dtype(l2)
    WT = np.zeros((n, n), dtype=dtype)                  # row j = column j of W (the rank-1 update runs over rows)
    QT = np.zeros((n, n), dtype=dtype)                  # QT[j] = A W[:, j]
    running = np.ones(n, dtype=bool)
    sweeps = np.zeros(n, dtype=np.int32)
    converged = np.zeros(n, dtype=bool)
    dmax_last = np.zeros(n, dtype=dtype)
    dmax_prev = np.full(n, np.inf, dtype=dtype)
    order = range(n - 1, -1, -1) if defect == "descending_one_sweep" else range(n)
    if defect == "descending_one_sweep":
        max_sweeps = 1
    zero = dtype(0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(max_sweeps):
            cols = np.nonzero(running)[0]
            if cols.size == 0:
                break
            dmax = np.zeros(cols.size, dtype=dtype)
            for k in order:
                wk, qk, bk, akk = WT[cols, k], QT[cols, k], A[k, cols], diag[k]
                if defect == "no_l2_in_denominator":
                    # the residual form with the bare count underneath: S(G_kj - sum_{l != k} A_kl w_l, l1) / G_kk
                    r = bk - (qk - A[k, k] * wk)
                    m = np.abs(r) - l1
                    w_new = np.where(m > zero, np.copysign(m / akk, r), zero)
                    if positive_only:
                        w_new = np.maximum(w_new, zero)
                elif positive_only:
                    g = (qk - bk) + l1
                    t = wk - g / akk
                    w_new = t if defect == "no_clamp" else np.where(t > zero, t, zero)
                else:
                    r = bk - (qk - akk * wk)
                    m = np.abs(r) - l1
                    v = np.copysign(m / akk, r)
                    w_new = v if defect == "no_clamp" else np.where(m > zero, v, zero)
                w_new = np.nan_to_num(w_new, nan=0.0, posinf=0.0, neginf=0.0).astype(dtype)    # (the defects only)
                d = w_new - wk
                live = d != zero
                if defect != "diagonal_free":
                    live &= cols != k
                if screen and positive_only:
                    live &= bk > l1
                mv = np.nonzero(live)[0]
                if mv.size == 0:
                    continue
                dm, cm = d[mv], cols[mv]
                if defect != "stale_q":
                    QT[cm] = QT[cm] + dm[:, None] * A[k][None, :]
                WT[cm, k] = w_new[mv]
                dmax[mv] = np.maximum(dmax[mv], np.abs(dm))
            sweeps[cols] += 1
            dmax_prev[cols] = dmax_last[cols] if sweeps[cols[0]] > 1 else np.inf
            dmax_last[cols] = dmax
            done = dmax <= tol
            converged[cols[done]] = True
            running[cols[done]] = False
    return dict(W=np.ascontiguousarray(WT.T), sweeps=sweeps, converged=converged, dmax_last=dmax_last, dmax_prev=dmax_prev)


def gradient(A, G, W, l1):
    """float64 ``A W - G + l1``: the smooth part's gradient plus ``l1``, column by column."""
    A, G, W = (np.asarray(a, dtype=np.float64) for a in (A, G, W))
    return A @ W - G + l1


def kkt_violation(A, G, W, l1, positive_only):
    """The largest violation of the optimality conditions, in float64, the diagonal excluded.  Positive mode: ``|g|`` on
    an active entry and ``max(0, -g)`` on a zero one, ``g = A w - G_j + l1``.  Signed mode: ``|A w - G_j + l1 sign(w)|``
    on an active entry and ``max(0, |A w - G_j| - l1)`` on a zero one."""
    W = np.asarray(W, dtype=np.float64)
    s = gradient(A, G, W, 0.0)
    if positive_only:
        g = s + l1
        v = np.where(W != 0.0, np.abs(g), np.maximum(0.0, -g))
    else:
        v = np.where(W != 0.0, np.abs(s + l1 * np.sign(W)), np.maximum(0.0, np.abs(s) - l1))
    v[np.diag_indices_from(v)] = 0.0
    return float(v.max())


def exact_weights(A, G, l1, positive_only):
    """``W64``: the schedule in float64 until the KKT violation is ``<= KKT64``."""
    out = coordinate_descent(A, l1, positive_only, 1e-15, 20000, np.float64)
    W = out["W"]
    assert kkt_violation(A, G, W, l1, positive_only) <= KKT64
    return W


def frame(name):
    """``(R, empty_item)``: the count matrix of a frame and its untouched item (``None`` for the pair)."""
    if name == "pair":
        return PAIR, None
    case = en.make_case(name)
    return case["R"], case["empty_item"]


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The frame, its matrices, ``W64`` and the yardstick ``W32`` with its sweep counts, computed once and shared
    (read-only)."""
    fr, l1, l2, positive, tol, max_sweeps, lds_cap = FIXTURES[name]
    R, e_item = frame(fr)
    u, i = np.nonzero(R)
    reps = R[u, i]
    rng = np.random.default_rng(len(name) + R.shape[1])
    perm = rng.permutation(int(reps.sum()))
    users, items = np.repeat(u, reps)[perm].astype(np.int64), np.repeat(i, reps)[perm].astype(np.int64)
    X = (R > 0).astype(np.float64)
    A64, G64 = gram(X, l2, np.float64)
    A32, G32 = gram(X, l2, np.float32)
    W64 = exact_weights(A64, G64, l1, positive)
    y = coordinate_descent(A32, l1, positive, tol, max_sweeps, np.float32)
    out = dict(name=name, U=R.shape[0], I=R.shape[1], l1=l1, l2=l2, positive=positive, tol=tol, max_sweeps=max_sweeps,
               lds_cap=lds_cap, users=users, items=items, R=R, X=X, A64=A64, G64=G64, A32=A32, W64=W64, W32=y["W"],
               sweeps32=y["sweeps"], converged32=y["converged"], dmax_last32=y["dmax_last"], dmax_prev32=y["dmax_prev"],
               empty_item=e_item)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def defect_weights(case, defect, dtype=np.float64):
    """``W`` of the case computed with one named mistake (at most DEFECT_SWEEPS sweeps: the yardstick's slowest column
    takes 50, and a mistake that keeps a column from settling is no nearer the truth after 100)."""
    X = case["R"] if defect == "counts_not_binary" else case["X"]
    A, _ = gram(X, case["l2"], dtype)
    return coordinate_descent(A, case["l1"], case["positive"], case["tol"], min(case["max_sweeps"], DEFECT_SWEEPS), dtype,
                              l2=case["l2"], defect=defect)["W"]


def scores(X, W):
    """float64 ``[X > 0] @ W``: every user's score row."""
    return (np.asarray(X) > 0).astype(np.float64) @ np.asarray(W, dtype=np.float64)


def forward_error(W, exact):
    """max |W - exact| relative to max |exact| (1 when the truth is all zeros)."""
    exact = np.asarray(exact, dtype=np.float64)
    scale = np.abs(exact).max()
    return float(np.abs(np.asarray(W, dtype=np.float64) - exact).max() / (scale if scale > 0 else 1.0))


def bound(case, ref=None):
    """What ``helpers.assert_as_accurate_as_reference(got, W32, W64)`` allows, relative to ``W64``'s scale."""
    return REL + 2.0 * forward_error(case["W32"] if ref is None else ref, case["W64"])


def kkt_bound(case):
    """The backward bound of the GPU test: 4 x the yardstick's violation plus ``tol * max_k sum_l |A_kl|``.  (A sweep
    that ends with every ``|d| <= tol`` leaves ``q_k`` no further than ``tol sum_l |A_kl|`` from where coordinate ``k``
    saw it, and coordinate ``k`` left its own ``g_k`` at zero or on the feasible side.)"""
    y = kkt_violation(case["A64"], case["G64"], case["W32"], case["l1"], case["positive"])
    return 4.0 * y + case["tol"] * float(np.abs(case["A64"]).sum(axis=1).max())


def decisive(case):
    """``(dec, positive, zero)`` of the support test: ``dec`` is twice what the forward test allows (absolute);
    ``positive`` marks the entries with ``|W64| > dec`` (the signed fixture: the GPU's entry must carry the same sign),
    ``zero`` those with ``W64 = 0`` and ``g64 > dec * A_kk`` (the signed fixture: ``l1 - |A w - G_j| > dec * A_kk``, the
    distance to either threshold).  The diagonal is in neither."""
    W64 = case["W64"]
    scale = np.abs(W64).max()
    dec = 2.0 * bound(case) * (scale if scale > 0 else 1.0)
    g = gradient(case["A64"], case["G64"], W64, case["l1"])
    if not case["positive"]:
        g = case["l1"] - np.abs(g - case["l1"])
    off = ~np.eye(case["I"], dtype=bool)
    pos = off & (np.abs(W64) > dec)
    zero = off & (W64 == 0.0) & (g > dec * np.diag(case["A64"])[:, None])
    return dec, pos, zero
