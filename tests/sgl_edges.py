"""Edge cases of the SGL kernels (csrc/sgl.hip), held to the fp64 restatement (tests/sgl_numpy.py); no goldens.  The
shapes come from the kernels' own tile sizes, ``TB = _lib.SGL_TILE_B`` batch rows and ``TN = _lib.SGL_TILE_N`` node rows:
batches of 1, TB - 1, TB and TB + 1 rows; sides of 1, TN - 1, TN, TN + 1 and 2 TN + 3 nodes; widths at which the zero
padding to the MFMA's 4 columns and the tiles' 16, and the columns-per-wave forms (64 | 128 | 256), change: 1, 3, 4, 5,
64, 100, 256; 0, 1 and 3 layers; a batch of one repeated user; positives that sit in the last, partial node tile; the node
dimension of the forward in one block and split over several; both ends of the temperature (0.05, 1.0) and of the
dropout (0, 0.9 -- most nodes isolated).  A crossed subset, not the product.  The cold temperature is crossed with
the narrow widths only: at D = 64 random rows have cosines of ~0.1 against ~1 for a row's own positive, every
exp((s - s_pos) / 0.05) is ~e^-17 against 1, and a row's InfoNCE part, log(sum) - (s_pos - 1) / temp, is the rounding
residue of two equal numbers in ANY fp32 arithmetic (the fp32 restatement misses the fp64 one by 1e-1 of it there): a
bound relative to the part cannot hold it, and the fixtures hold the warm and the default temperature at width.

The sub-graphs are the restatement's own fp32 matrices, handed to the mirror in the reference's dict format, so a case
tests the step and nothing else.  Bounds: every loss part REL of itself, every gradient REL of its scale -- against fp64,
with no allowance for a reference's rounding, since there is none here.
"""
import numpy as np

import sgl_numpy as sx
from helpers import REL, assert_scalar_close, assert_tensor_close, float64_oracle, to64

TB, TN = 32, 64      # asserted against _lib.SGL_TILE_B / SGL_TILE_N by the GPU test

#        name                  B       U            I            D    L  temp  ratio splits mode         extras
CASES = [
    ("b1_side1_d1_l0",         1,      1,           TN - 1,      1,   0, 1.0,  0.0,  1, "both_side", {}),
    ("b31_d3_cold",            TB - 1, TN,          TN + 1,      3,   1, 0.05, 0.9,  0, "both_side", {}),
    ("b32_d4_l3_split2",       TB,     TN + 1,      2 * TN + 3,  4,   3, 0.2,  0.4,  2, "both_side", {}),
    ("b33_d5_cold",            TB + 1, 2 * TN + 3,  TN,          5,   1, 0.05, 0.4,  0, "both_side", {}),
    ("d64_l3",                 TB + 1, TN - 1,      2 * TN + 3,  64,  3, 0.2,  0.4,  0, "both_side", {}),
    ("d100_l1",                TB - 1, TN + 1,      TN,          100, 1, 0.2,  0.4,  0, "both_side", {}),
    ("d256_l3_split3",         TB + 1, 2 * TN + 3,  TN + 1,      256, 3, 0.2,  0.4,  3, "both_side", {}),
    ("one_user",               TB + 1, TN + 1,      TN - 1,      24,  1, 0.2,  0.4,  0, "both_side", {"one_user": True}),
    ("pos_in_last_tile",       TB,     TN + 1,      2 * TN + 3,  24,  1, 0.2,  0.0,  0, "both_side", {"last_tile": True}),
    ("user_side_d64_l0",       TB,     TN,          TN + 1,      64,  0, 0.2,  0.4,  1, "user_side", {}),
    ("item_side_sparse",       TB - 1, TN - 1,      TN,          5,   3, 1.0,  0.9,  2, "item_side", {}),
    ("d64_split_many",         1,      1,           2 * TN + 3,  64,  1, 1.0,  0.0,  3, "both_side", {}),
]
CASE_NAMES = [c[0] for c in CASES]


def make_case(name):
    """dict(w, graph, subs, hp, batch, U, I, D, L, B, splits) of one edge case, seeded by its position in CASES."""
    idx = CASE_NAMES.index(name)
    _, B, U, I, D, L, temp, ratio, splits, mode, extra = CASES[idx]
    rng = np.random.default_rng(300 + idx)
    N = U + I
    pairs = {(u % U, i) for i, u in enumerate(rng.permutation(max(U, I)))  if i < I}   # every item keeps an edge
    for u in range(U):
        for i in rng.choice(I, size=min(3, I), replace=False):
            pairs.add((u, int(i)))
    pairs = np.array(sorted(pairs), dtype=np.int64)[rng.permutation(len(pairs))]
    eu, ei = pairs[:, 0].copy(), pairs[:, 1].copy()
    deg = np.bincount(np.concatenate([eu, U + ei]), minlength=N).astype(np.float64)
    rows, cols = np.concatenate([eu, U + ei]), np.concatenate([U + ei, eu])
    graph = (rows, cols, (1.0 / np.sqrt(deg[rows] * deg[cols])).astype(np.float32), N)
    keeps = [[(rng.random(eu.size) >= ratio).astype(np.uint8) if ratio > 0 else None for _ in range(max(L, 1))]
             for _ in range(2)]
    subs = [[sx.sub_matrix(eu, ei, U, I, k) for k in keeps[v]] for v in range(2)]
    w = {"user_embedding": rng.standard_normal((U, D)).astype(np.float32),
         "item_embedding": rng.standard_normal((I, D)).astype(np.float32)}
    pick = rng.integers(0, eu.size, B)
    users, pos = eu[pick].copy(), ei[pick].copy()
    if extra.get("one_user"):
        users[:] = U // 2
    if extra.get("last_tile"):          # ids beyond the last full tile of their side
        users[:] = (U // TN) * TN + rng.integers(0, U - (U // TN) * TN, B)
        pos[:] = (I // TN) * TN + rng.integers(0, I - (I // TN) * TN, B)
    neg = rng.integers(0, I, B)
    hp = dict(L=L, regs=1e-3, ssl_reg=0.1, ssl_temp=temp, ssl_mode=mode, ssl_ratio=ratio, pretrain=0, aug_type=2)
    # the batch's largest |pos - neg| score is 4, whatever the width and depth: no softplus saturates
    x = sx.sgl_predict(w, graph, hp, users, pos) - sx.sgl_predict(w, graph, hp, users, neg)
    f = np.float32(np.sqrt(4.0 / max(float(np.abs(x).max()), 1e-30)))
    w = {k: v * f for k, v in w.items()}
    return dict(name=name, w=w, graph=graph, subs=subs, hp=hp, batch=(users, pos, neg), U=U, I=I, D=D, L=L, B=B,
                splits=splits)


def reference_format(case):
    """The case's sub-graphs as the reference's per-layer dict (aug_type 2 keys)."""
    N = case["U"] + case["I"]
    d = {}
    for v in range(2):
        for l in range(max(case["L"], 1)):
            r, c = np.nonzero(case["subs"][v][l])
            nm = "sub%d%d" % (v + 1, l + 1)
            d["adj_indices_" + nm] = np.vstack([r, c])
            d["adj_values_" + nm] = case["subs"][v][l][r, c]
            d["adj_shape_" + nm] = (N, N)
    return d


def check_step(case, loss, parts, grads, what=""):
    """Loss parts and gradients against the fp64 restatement."""
    with float64_oracle(sx):
        subs = [[np.asarray(a, dtype=np.float64) for a in view] for view in case["subs"]]
        p64, l64, g64 = sx.sgl_grads(to64(case["w"]), case["graph"], subs, case["hp"], case["batch"])
    assert_scalar_close(loss, l64, REL, f"{what} loss")
    for got, ref, name in zip(parts, p64, ("bpr", "emb", "ssl")):
        assert_scalar_close(got, ref, REL, f"{what} {name}")
    for k in sx.KEYS:
        got = np.asarray(grads[k]).reshape(g64[k].shape)
        print(f"  {what} grad {k}: err {np.abs(got - g64[k]).max():.3e} of scale {np.abs(g64[k]).max():.3e}")
        assert_tensor_close(got, g64[k], REL, f"{what} grad {k}")
