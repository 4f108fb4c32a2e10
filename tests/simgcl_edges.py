"""Edge-case inputs for SimGCL's kernels (tests/test_simgcl_edges_gpu.py holds them to the fp64 restatement; the CPU tests
in tests/test_simgcl_host.py check the builder itself).  A crossed subset around the kernels' own tiles -- TB query rows
and TN key rows per InfoNCE tile --: the number of unique ids per side at 1, TB - 1, TB, TB + 1 and 2 TN + 3 (the last
key tile partial), every row width at which a wave's four registers per lane or the 16-wide MFMA column blocks take
another path, every L, eps 0 (the views coincide) / 0.1 / 1, isolated nodes, a batch matrix of norm 0, and one case whose
most negative pos - neg is -14, where the 1e-7 inside the log matters (4 elsewhere).

The uniforms are settled by simgcl_numpy.settle_noise -- no noise where 0 < |y| < 1e-4 max|Y_k| -- and a case with more
than 1 % of them zeroed is rejected here, on the CPU."""
import numpy as np

import simgcl_numpy as sx

TB, TN = 32, 64          # HIPREC_SIMGCL_TILE_B / _N; the GPU test asserts them against the library

# name: (D, L, eps, unique users, unique items, extras)
CASES = {
    "d1_l1_one_user": (1, 1, 0.1, 1, TB - 1, {}),
    "d3_l2_eps1": (3, 2, 1.0, TB, TB + 1, {}),
    "d4_l3_eps0": (4, 3, 0.0, TB + 1, TB, {}),
    "d5_l4_one_item": (5, 4, 0.1, TB - 1, 1, {}),
    "d16_l2_tail": (16, 2, 0.1, 2 * TN + 3, 2 * TN + 3, {}),
    "d64_l3_isolated": (64, 3, 0.1, TB + 1, TB - 1, {"isolated": True}),
    "d100_l2_zero_norm": (100, 2, 1.0, TB, TB, {"isolated": True, "zero_neg": True}),
    "d256_l4": (256, 4, 0.1, 2 * TN + 3, TB + 1, {}),
    "d64_l1_deep": (64, 1, 0.1, TB - 1, TB + 1, {"min_x": -14.0}),
    "d16_l4_two_views": (16, 4, 1.0, 1, 2 * TN + 3, {"user_view": "two_views"}),
}


def norm_adj(eu, ei, U, I):
    N = U + I
    A = np.zeros((N, N), dtype=np.float64)
    A[eu, U + ei] = 1
    A = A + A.T
    deg = A.sum(axis=1)
    d = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1)), 0.0)
    A = (d[:, None] * A * d[None, :]).astype(np.float32)
    rows, cols = np.nonzero(A)
    return (rows.astype(np.int64), cols.astype(np.int64), A[rows, cols], N), A


def build(name):
    """``dict(w, graph, hp, batch, noise, zeroed, n_uniq)`` of one case; deterministic in its name."""
    D, L, eps, nu, ni, extra = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 7)
    n_iso = 3 if extra.get("isolated") else 0
    U, I = max(nu, 8) + 5 + n_iso, max(ni, 8) + 6 + n_iso
    lu, li = U - n_iso, I - n_iso                       # the last n_iso users and items have no edge
    pairs = {(u, int(rng.integers(0, li))) for u in range(lu)} | {(int(rng.integers(0, lu)), i) for i in range(li)}
    for u in range(lu):
        for i in rng.choice(li, size=min(li, 3), replace=False):
            pairs.add((u, int(i)))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    graph, A = norm_adj(pairs[:, 0], pairs[:, 1], U, I)
    B = max(nu, ni) + 9
    # exactly nu unique users and ni unique items, each at least once, ids spread over the connected range
    pu, pi = rng.choice(lu, size=nu, replace=False), rng.choice(li, size=ni, replace=False)
    users = np.concatenate([pu, pu[rng.integers(0, nu, size=B - nu)]])[rng.permutation(B)]
    pos = np.concatenate([pi, pi[rng.integers(0, ni, size=B - ni)]])[rng.permutation(B)]
    neg = np.full(B, I - 1, dtype=np.int64) if extra.get("zero_neg") else rng.integers(0, li, size=B)
    w = {sx.KEYS[0]: rng.standard_normal((U, D)).astype(np.float32), sx.KEYS[1]: rng.standard_normal((I, D)).astype(np.float32)}
    # scale the tables so that the most negative pos - neg is min_x (the clean pool is linear in them)
    E0 = np.concatenate([w[sx.KEYS[0]], w[sx.KEYS[1]]]).astype(np.float64)
    P0 = sx.pooled(E0, A.astype(np.float64), L)
    x = (P0[users] * (P0[U + pos] - P0[U + neg])).sum(axis=1)
    scale = np.sqrt(abs(extra.get("min_x", -4.0)) / abs(x.min())) if x.min() < 0 else 1.0
    w = {k: (v * np.float32(scale)).astype(np.float32) for k, v in w.items()}
    E0 = np.concatenate([w[sx.KEYS[0]], w[sx.KEYS[1]]])
    noise, zeroed = [], 0.0
    for v in range(2):
        nz, share = sx.settle_noise(E0, A, L, eps, rng.random((L, U + I, D), dtype=np.float32))
        noise.append(nz)
        zeroed = max(zeroed, share)
    assert zeroed <= sx.ZEROED_CAP, f"{name}: {zeroed:.2%} of the uniforms zeroed"
    hp = dict(L=L, eps=eps, reg=1e-3, lam=0.5, temp=0.2, user_view=extra.get("user_view", "reference"))
    return dict(w=w, graph=graph, hp=hp, batch=(users.astype(np.int64), pos.astype(np.int64), neg.astype(np.int64)),
                noise=np.stack(noise), zeroed=zeroed, n_uniq=(nu, ni), U=U, I=I, D=D, n_iso=n_iso, min_x=float(x.min() * scale ** 2))
