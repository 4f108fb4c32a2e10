"""EASE (Steck 2019) restated in numpy: the oracle of csrc/ease.hip (the reference has no counterpart).

    X = [frame > 0]          G = X^T X + reg I          P = G^-1
    B[i, j] = -P[i, j] / P[j, j]  (i != j),  B[j, j] = 0          score(u, .) = X_u B

``ease_weights(X, reg, np.float64)`` is the truth the GPU is held to; ``ease_weights(X, reg, np.float32)`` is the
yardstick: the same computation in float32 with numpy's Cholesky (``L = cholesky(G)``, ``W = solve(L, I)``,
``P = W^T W``), whose distance from the truth is what float32 costs on this matrix.

The named defects are the mistakes a kernel for this model can make; tests/test_ease_host.py shows that each lands
outside the bound the GPU test applies.
"""
import functools

import numpy as np

PANEL = 64            # HIPREC_EASE_PANEL (tests/test_ease_host.py holds it to the header)
MFMA = 16             # HIPREC_EASE_MFMA
REL = 1e-5            # the project's relative bound (tests/helpers.py)
EMPTY_USER = 1
DEFECTS = ("no_reg", "row_div", "keep_diag", "sign", "counts_not_binary", "upper_not_mirrored")

# name -> (n_users, n_items, reg, lds_cap, seed); lds_cap = 0 leaves the Gram accumulator to the library (LDS here)
FIXTURES = {
    "n1": (5, 1, 10.0, 0, 1),
    "n2": (6, 2, 10.0, 0, 2),
    "n15": (40, 15, 10.0, 0, 3),
    "n17": (40, 17, 10.0, 0, 4),
    "panel_minus": (130, PANEL - 1, 10.0, 0, 5),
    "panel": (130, PANEL, 10.0, 0, 6),
    "panel_plus": (130, PANEL + 1, 10.0, 0, 7),
    "two_panels_ragged": (300, 2 * PANEL + 21, 10.0, 0, 8),
    "ws_path": (500, 261, 10.0, 256, 9),          # 261 > lds_cap: the accumulator goes through the workspace
    "stiff": (120, 40, 0.004, 0, 10),             # items 5 and 6 are the same column, reg is small
}
STIFF_TWINS = (5, 6)


def empty_item(n_items):
    return min(3, n_items - 1)


@functools.lru_cache(maxsize=None)
def make_case(name):
    """The frame (``users``, ``items``: shuffled, pairs repeated up to three times), its count matrix ``R`` and the
    derived matrices, computed once and shared (read-only)."""
    U, I, reg, lds_cap, seed = FIXTURES[name]
    rng = np.random.default_rng(seed)
    p = np.clip(0.5 / np.sqrt(1.0 + np.arange(I)), 0.03, 0.5)          # popularity-skewed columns
    m = rng.random((U, I)) < p
    e_item = empty_item(I)
    if name == "stiff":
        m[:, STIFF_TWINS[1]] = m[:, STIFF_TWINS[0]]
    m[:, e_item] = False
    m[EMPTY_USER] = False
    for j in np.nonzero(~m.any(axis=0))[0]:                            # exactly one empty item and one empty user
        if j != e_item:
            m[0, j] = True
    for u in np.nonzero(~m.any(axis=1))[0]:
        if u != EMPTY_USER and I > 1:
            m[u, 0] = True
    if name == "stiff":
        m[:, STIFF_TWINS[1]] = m[:, STIFF_TWINS[0]]
    u, i = np.nonzero(m)
    reps = rng.integers(1, 4, len(u))
    u, i = np.repeat(u, reps), np.repeat(i, reps)
    perm = rng.permutation(len(u))
    users, items = u[perm].astype(np.int64), i[perm].astype(np.int64)
    R = np.zeros((U, I), dtype=np.int64)
    np.add.at(R, (users, items), 1)
    X = (R > 0).astype(np.float64)
    B64, P64 = ease_weights(X, reg, np.float64, want_inverse=True)
    B32, P32 = ease_weights(X, reg, np.float32, want_inverse=True)
    G32 = gram(X, reg, np.float32)
    out = dict(name=name, U=U, I=I, reg=reg, lds_cap=lds_cap, users=users, items=items, R=R, X=X, G32=G32, B64=B64,
               P64=P64, B32=B32, P32=P32, empty_item=e_item)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def gram(X, reg, dtype=np.float64):
    """``X^T X + reg I`` (integer counts: exact in either dtype below 2^24)."""
    X = np.asarray(X)
    counts = X.astype(np.int64).T @ X.astype(np.int64)
    G = counts.astype(dtype)
    G[np.diag_indices_from(G)] += dtype(reg)
    return G


def ease_weights(X, reg, dtype=np.float64, defect=None, want_inverse=False):
    """``B`` of the matrix ``X`` (binary, or the count matrix: it is binarised here) in ``dtype`` arithmetic."""
    assert defect is None or defect in DEFECTS, defect
    X = np.asarray(X)
    Xb = X if defect == "counts_not_binary" else (X > 0)
    n = X.shape[1]
    if defect == "no_reg":
        # reg left out wherever the diagonal is not zero already (an untouched item keeps it, or nothing is defined)
        counts = Xb.astype(np.int64).T @ Xb.astype(np.int64)
        G = counts.astype(dtype)
        idx = np.nonzero(np.diag(counts) == 0)[0]
        G[idx, idx] = dtype(reg)
        P = np.linalg.pinv(G.astype(np.float64)).astype(dtype)
    else:
        G = gram(Xb, reg, dtype)
        L = np.linalg.cholesky(G)
        W = np.linalg.solve(L, np.eye(n, dtype=dtype))
        P = W.T @ W
    assert P.dtype == dtype
    d = np.diag(P).copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        B = -P / (d[:, None] if defect == "row_div" else d[None, :])
    if defect == "sign":
        B = -B
    if defect == "upper_not_mirrored":       # the upper triangle copied from B's lower one, not formed from P's
        B = np.tril(B) + np.tril(B, -1).T
    if defect != "keep_diag":
        B[np.diag_indices_from(B)] = 0.0
    return (B, P) if want_inverse else B


def scores(X, B):
    """float64 ``[X > 0] @ B``: every user's score row."""
    return (np.asarray(X) > 0).astype(np.float64) @ np.asarray(B, dtype=np.float64)


def forward_error(B, exact):
    """max |B - exact| relative to max |exact| (1 when the truth is all zeros)."""
    exact = np.asarray(exact, dtype=np.float64)
    scale = np.abs(exact).max()
    return float(np.abs(np.asarray(B, dtype=np.float64) - exact).max() / (scale if scale > 0 else 1.0))


def residual(G, P):
    """The backward error ``max |G P - I|`` evaluated in float64."""
    G, P = np.asarray(G, dtype=np.float64), np.asarray(P, dtype=np.float64)
    return float(np.abs(G @ P - np.eye(G.shape[0])).max())


def bound(case):
    """What ``helpers.assert_as_accurate_as_reference(got, B32, B64)`` allows, relative to ``B64``'s scale."""
    return REL + 2.0 * forward_error(case["B32"], case["B64"])
