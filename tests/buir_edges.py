"""Edge-case inputs for BUIR's kernels (tests/test_buir_edges_gpu.py holds them to the fp64 restatement).  A crossed subset
around the fused kernel's own tile -- TILE_B batch rows per block --: the batch at 1, TB - 1, TB, TB + 1 and 2 TB + 3 (a
third, partial block), every row width at which a wave's four registers per lane, the 16-wide MFMA column blocks or the
16-wide K-slabs of W take another path (1, 3, 4, 5, 16, 17, 64, 100, 256), every L, a batch of one repeated pair, isolated
nodes in the batch, and all-zero target rows (their loss term is exactly 2 and they add no gradient).

The target tables are drawn independently of the online ones, so a swapped or a trained target shows."""
import numpy as np

import buir_numpy as bx

TB = 32          # HIPREC_BUIR_TILE_B; the GPU test asserts it against the library

# name: (D, L, B, extras)
CASES = {
    "d1_l1_b1": (1, 1, 1, {}),
    "d1_l2_two_blocks": (1, 2, 2 * TB + 3, {}),
    "d3_l2_tb_minus_1": (3, 2, TB - 1, {}),
    "d4_l3_tb": (4, 3, TB, {}),
    "d5_l4_tb_plus_1": (5, 4, TB + 1, {}),
    "d16_l2_three_blocks": (16, 2, 2 * TB + 3, {}),
    "d17_l3_tb": (17, 3, TB, {}),
    "d64_l3_isolated": (64, 3, TB + 1, {"isolated": True}),
    "d64_l2_repeated_pair": (64, 2, TB + 1, {"repeat": True}),
    "d100_l1_zero_target": (100, 1, 2 * TB + 3, {"isolated": True, "zero_target": True}),
    "d256_l4_three_blocks": (256, 4, 2 * TB + 3, {}),
    "d256_l1_b1": (256, 1, 1, {}),
}
N_ISO = 3


def norm_adj(eu, ei, U, I):
    N = U + I
    A = np.zeros((N, N), dtype=np.float64)
    A[eu, U + ei] = 1
    A = A + A.T
    deg = A.sum(axis=1)
    d = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1)), 0.0)
    A = (d[:, None] * A * d[None, :]).astype(np.float32)
    rows, cols = np.nonzero(A)
    return rows.astype(np.int64), cols.astype(np.int64), A[rows, cols], N


def build(name):
    """``dict(w, graph, L, batch, U, I, D, B, n_iso)`` of one case; deterministic in its name."""
    D, L, B, extra = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 11)
    n_iso = N_ISO if extra.get("isolated") else 0
    U, I = 21 + n_iso, 27 + n_iso
    lu, li = U - n_iso, I - n_iso                       # the last n_iso users and items have no edge
    pairs = {(u, int(rng.integers(0, li))) for u in range(lu)} | {(int(rng.integers(0, lu)), i) for i in range(li)}
    for u in range(lu):
        for i in rng.choice(li, size=3, replace=False):
            pairs.add((u, int(i)))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    graph = norm_adj(pairs[:, 0], pairs[:, 1], U, I)
    if extra.get("repeat"):
        users, pos = np.full(B, 4, dtype=np.int64), np.full(B, 9, dtype=np.int64)
    else:
        users, pos = rng.integers(0, lu, size=B), rng.integers(0, li, size=B)
        if n_iso and B > 2 * n_iso:                     # every isolated node sits in the batch, paired both ways
            users[:n_iso] = np.arange(lu, U)
            pos[n_iso:2 * n_iso] = np.arange(li, I)
            users[2 * n_iso], pos[2 * n_iso] = U - 1, I - 1
    neg = rng.integers(0, I, size=B)
    s = np.float32(1.0 / np.sqrt(D))
    w = {bx.ONLINE[0]: rng.standard_normal((U, D)).astype(np.float32), bx.ONLINE[1]: rng.standard_normal((I, D)).astype(np.float32),
         bx.TARGET[0]: rng.standard_normal((U, D)).astype(np.float32), bx.TARGET[1]: rng.standard_normal((I, D)).astype(np.float32),
         bx.PREDICTOR[0]: (rng.standard_normal((D, D)) * s).astype(np.float32),
         bx.PREDICTOR[1]: (rng.standard_normal(D) * np.float32(0.1)).astype(np.float32)}
    if extra.get("zero_target"):                        # isolated: the pooled row is the raw row / (L + 1), exactly 0
        w[bx.TARGET[0]][lu:] = 0
        w[bx.TARGET[1]][li:] = 0
    return dict(w=w, graph=graph, L=L, batch=(users.astype(np.int64), pos.astype(np.int64), neg.astype(np.int64)), U=U, I=I,
                D=D, B=B, n_iso=n_iso)
