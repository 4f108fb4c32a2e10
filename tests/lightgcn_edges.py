"""Fixtures of the LightGCN edge tests, shared by tests/test_lightgcn_edges_host.py (which shows on the CPU that the
inputs can see a defect of each kind the kernels could have, and that the fp32 oracle is a fair yardstick on them) and
tests/test_lightgcn_edges_gpu.py (which runs csrc/lightgcn.hip and csrc/spmm_sliced.hip on those very inputs).  No
tests here.

A LightGCN step takes its form from the embedding width D and the node count N: ``sliced_width`` (column slices of 4
or 2 floats in LDS, or the edge-parallel gather), rank-one factored edge values or a values stream, and the loss
kernel's columns per lane (NPL 1 / 2 / 4 at D <= 64 / 128 / 256).  ``forms`` restates those limits and ``FORM_TABLE``
holds what they give per case, written out by hand.  The width cases reach every (slice width, NPL) pair that exists,
the depth cases L = 0 .. 5 (the code of ``propagate_sliced`` that runs only at L < 2, the ping-pong parity beyond 3),
the hub cases the rows the sliced SpMM does not write directly, the threshold cases the last node count of each slice
width (row cap exactly ``kSlicedMinRowCap``) and the first of the next form, the seam cases the second trip of the
grid-stride loops (triple 8192), the batch cases one triple, one user, ``pos == neg`` and both saturated branches of
the softplus.

The yardstick is ``oracle.lightgcn_numpy`` in fp32 and (``float64_oracle``) fp64.  Host-drawn keep masks are the draw
the engine itself makes, ``(torch.rand(nnz) + keep_pro).int().bool()`` under ``torch.manual_seed(case.seed)``."""
import collections
import functools

import numpy as np

from helpers import REL, float64_oracle, to64
from ngcf_edges import HUB, WINDOW_SLOTS, hub_graph
from oracle import lightgcn_numpy as olg

# the limits of csrc/common.hpp (kWave, kMaxBlocks * kWavesPerBlock), csrc/lightgcn.hip (launch_lightgcn_loss) and
# csrc/spmm_sliced.hip (kSlicedLds, kSlicedMinRowCap, kSlicedMaxRowCap, the 16-bit node ids)
WAVE = 64
NPL_STEPS = (64, 128, 256)                       # D <= 64: 1 column per lane, <= 128: 2, <= 256: 4
MAX_DIM = NPL_STEPS[-1]
GRID_WAVES = 2048 * 4                            # kMaxBlocks * kWavesPerBlock: triples of one trip of the loss kernel
SLICED_LDS, SLICED_MIN_ROW_CAP, SLICED_MAX_ROW_CAP = 160 * 1024 - 64, 128, 512
MAX_SLICED_NODES = 65536
KEYS = olg.KEYS

Case = collections.namedtuple("Case", "key U I D L adj w batch mask keep_pro decay spmm dropout_rng seed pairs")
Ref = collections.namedtuple("Ref", "loss64 g64 loss32 g32 table64")

DECAY, KEEP = 1e-5, 0.6
ORDERS, ORDER_SHARE = 8, 1.0 / 3.0               # tests/test_ngcf_edges_host.py's

DEFECTS = ("last_col", "cols64", "cols128", "mean_over_l", "last_layer_fwd", "last_layer_bwd", "l2_row",
           "col_factor", "triple_8192", "dup_overwrite", "softplus_inf", "empty_stale", "spill_lost", "edge_kept_bwd")


def sliced_width(n_rows, dim):
    """``sliced_width`` of csrc/spmm_sliced.hip on a device with 160 KB of LDS."""
    if n_rows <= 0 or n_rows >= MAX_SLICED_NODES or dim <= 0:
        return 0
    for w in (4, 2):
        if dim % w == 0 and (n_rows + 1 + SLICED_MIN_ROW_CAP) * w * 4 <= SLICED_LDS:
            return w
    return 0


def sliced_row_cap(n_rows, dim):
    """``sliced_row_cap`` of csrc/spmm_sliced.hip."""
    w = sliced_width(n_rows, dim)
    return 0 if w == 0 else min(SLICED_LDS // (w * 4) - n_rows - 1, SLICED_MAX_ROW_CAP)


def npl(dim):
    return next(k for k, top in zip((1, 2, 4), NPL_STEPS) if dim <= top)


# the last node count each slice width holds (row cap exactly SLICED_MIN_ROW_CAP there), from the constants
LAST_W4 = SLICED_LDS // (4 * 4) - 1 - SLICED_MIN_ROW_CAP
LAST_W2 = SLICED_LDS // (2 * 4) - 1 - SLICED_MIN_ROW_CAP

# ---- the cases ------------------------------------------------------------------------------------------------------
WIDTHS = (1, 6, 7, 63, 64, 65, 70, 100, 128, 129, 130, 200, 256)   # 70, 130: slice width 2 at NPL 2 and 4
WIDTH_CASES = {f"w{d}": d for d in WIDTHS}
DEPTH_CASES = {f"l{l}": l for l in (0, 1, 2, 4, 5)}
HUB_CASES = {"hub_empty16": 16, "hub_empty6": 6}
THRESHOLD_CASES = {f"n{n}": n for n in (LAST_W4, LAST_W4 + 1, LAST_W2, LAST_W2 + 1)}
BIG_CASE = f"n{MAX_SLICED_NODES}"
BATCH_CASES = ("one_triple", "one_user", "pos_eq_neg", "saturated", "decay0")
DEVICE_CASES = {"dev6": 6, "dev100": 100}
STAGED_CASES = {"staged_l1": 1, "staged_l3": 3}
ALL_CASES = (list(WIDTH_CASES) + list(DEPTH_CASES) + list(HUB_CASES) + list(THRESHOLD_CASES) + [BIG_CASE, "general",
             "seam", "seam_predict"] + list(BATCH_CASES) + ["keep1"] + list(DEVICE_CASES) + list(STAGED_CASES))
TRAIN_CASES = [k for k in ALL_CASES if k != "seam_predict"]

# what ``forms`` must give: (slice width under ``auto``, factored, NPL) -- written out by hand;
# tests/test_lightgcn_edges_host.py holds ``forms`` to it and tests/test_lightgcn_edges_gpu.py prints it
T_, F_ = True, False
FORM_TABLE = {
    "w1": (0, F_, 1), "w6": (2, T_, 1), "w7": (0, F_, 1), "w63": (0, F_, 1), "w64": (4, T_, 1), "w65": (0, F_, 2),
    "w70": (2, T_, 2), "w100": (4, T_, 2), "w128": (4, T_, 2), "w129": (0, F_, 4), "w130": (2, T_, 4),
    "w200": (4, T_, 4), "w256": (4, T_, 4),
    "l0": (4, T_, 1), "l1": (4, T_, 1), "l2": (4, T_, 1), "l4": (4, T_, 1), "l5": (4, T_, 1),
    "hub_empty16": (4, T_, 1), "hub_empty6": (2, T_, 1),
    "n10107": (4, T_, 1), "n10108": (2, T_, 1), "n20343": (2, T_, 1), "n20344": (0, F_, 1), "n65536": (0, F_, 1),
    "general": (4, F_, 1), "seam": (4, T_, 1), "seam_predict": (4, T_, 1),
    "one_triple": (4, T_, 1), "one_user": (4, T_, 1), "pos_eq_neg": (4, T_, 1), "saturated": (4, T_, 1),
    "decay0": (4, T_, 1), "keep1": (4, T_, 1), "dev6": (2, T_, 1), "dev100": (4, T_, 2),
    "staged_l1": (4, T_, 2), "staged_l3": (4, T_, 2),
}

SAT_HIGH, SAT_LOW, OVERFLOW = 20.0, -20.0, 89.0  # the kernel's branch points; expf overflows fp32 beyond 88.7


def factors(adj):
    """``factor_edge_values`` of a CSR: (row_scale, col_scale) or None."""
    from beta_recsys_amd.lightgcn import factor_edge_values

    return factor_edge_values(adj.indptr, adj.indices, adj.data)


def forms(c):
    w = sliced_width(c.U + c.I, c.D)
    factored = w > 0 and factors(c.adj) is not None and factors(c.adj.T.tocsr()) is not None
    return w, factored, npl(c.D)


def settings(key):
    """``(spmm settings, dropout_rng settings)`` a case runs under: ``auto`` and ``gather``, and the values stream where
    ``auto`` slices, with the host draw, unless the case says otherwise."""
    if key in DEPTH_CASES or key in ("general", "seam", "seam_predict"):
        spmm = ("auto", "gather")
    elif key in THRESHOLD_CASES or key == BIG_CASE or key in STAGED_CASES:
        spmm = ("auto",)
    elif key in DEVICE_CASES:
        spmm = ("auto", "sliced_values")
    else:
        spmm = ("auto", "gather") + (("sliced_values",) if FORM_TABLE[key][0] else ())
    if key in DEVICE_CASES or key in STAGED_CASES:
        return spmm, ("device",)
    return spmm, ("torch_cpu", "device") if key == "keep1" else ("torch_cpu",)


def spmm_modes(key):
    return list(settings(key)[0])


def host_mask(nnz, keep_pro, seed):
    """The keep mask ``LightGCN.draw_keep_mask`` draws on the host under ``torch.manual_seed(seed)``."""
    import torch

    gen = torch.Generator().manual_seed(seed)
    return (torch.rand(nnz, generator=gen) + keep_pro).int().bool().numpy()


def draw_weights(rng, U, I, D, gain=1.0):
    return {"user_embedding.weight": (gain * rng.standard_normal((U, D))).astype(np.float32),
            "item_embedding.weight": (gain * rng.standard_normal((I, D))).astype(np.float32)}


def random_batch(rng, U, I, B):
    return tuple(np.asarray(x, dtype=np.int64) for x in (rng.integers(0, U, B), rng.integers(0, I, B),
                                                         rng.integers(0, I, B)))


def make_case(key, D, L, seed, U=37, I=29, n_edges=250, B=24, adj=None, batch=None, gain=1.0, keep_pro=KEEP,
              decay=DECAY, pairs=None):
    rng = np.random.default_rng(seed)
    if adj is None:
        adj = olg.build_norm_adj(U, I, rng.integers(0, U, n_edges), rng.integers(0, I, n_edges))
    w = draw_weights(rng, U, I, D, gain)
    if batch is None:
        batch = random_batch(rng, U, I, B)
    batch = tuple(np.asarray(x, dtype=np.int64) for x in batch)
    spmm, dropout_rng = settings(key)
    return Case(key, U, I, D, L, adj, w, batch, host_mask(adj.nnz, keep_pro, seed), keep_pro, decay, spmm, dropout_rng,
                seed, pairs)


def hub_fixture(key):
    """D^-1 A without the identity (tests/ngcf_edges.py ``hub_graph``): item HUB is linked to every user that has an
    edge (a row of 1300 edges in both graphs), four users and three items have no edge; one edgeless node of each kind
    and the hub are in the batch."""
    seed = 301 + HUB_CASES[key]
    rng = np.random.default_rng(seed)
    U, I, adj, empty_u, empty_i = hub_graph(rng)
    users, pos, neg = random_batch(rng, U, I, 24)
    live_u, live_i = np.setdiff1d(np.arange(U), empty_u), np.setdiff1d(np.arange(I), empty_i)
    users, pos, neg = live_u[users % live_u.size], live_i[pos % live_i.size], live_i[neg % live_i.size]
    users[0], pos[1], neg[2], pos[3] = empty_u[0], empty_i[0], empty_i[0], HUB
    return make_case(key, HUB_CASES[key], 2, seed, U=U, I=I, adj=adj, batch=(users, pos, neg))


def empty_rows(c):
    return np.nonzero(np.diff(c.adj.indptr) == 0)[0]


def general_graph(rng, U, I, n_edges):
    """``build_norm_adj`` with every edge value multiplied by an independent U(0.5, 1.5) factor: not rank-one."""
    adj = olg.build_norm_adj(U, I, rng.integers(0, U, n_edges), rng.integers(0, I, n_edges))
    adj.data = (adj.data * rng.uniform(0.5, 1.5, adj.nnz)).astype(np.float32)
    return adj


def seam_batch(rng, U, I, B):
    """B triples of which the last uses a user, a positive and a negative item that occur nowhere else."""
    users, pos, neg = (rng.integers(0, n - 2, B) for n in (U, I, I))
    users[-1], pos[-1], neg[-1] = U - 1, I - 1, I - 2
    return users, pos, neg


def saturated_stats(c):
    """x = neg score - pos score of every triple of the fp64 evaluation (training graph)."""
    dropped = olg.apply_edge_dropout(c.adj, c.mask, c.keep_pro)
    with float64_oracle(olg):
        ua, ia = olg.propagate(to64(c.w), dropped.astype(np.float64), c.L)
    users, pos, neg = c.batch
    return (ua[users] * ia[neg]).sum(1) - (ua[users] * ia[pos]).sum(1)


def saturated_fixture():
    """D = 64, weights x 3, B = 48: the triples are the first 48 of a random draw, except that the last three are the
    (user, pos, neg) combinations of largest x, of smallest x, and of smallest |x| among 4000 random ones -- so the
    large-x branch of the softplus is taken beyond the point where expf overflows fp32 when that is reachable."""
    seed = 77
    c = make_case("saturated", 64, 3, seed, B=48, gain=3.0)
    rng = np.random.default_rng(seed + 1)
    pool = c._replace(batch=random_batch(rng, c.U, c.I, 4000))
    x = saturated_stats(pool)
    picks = [int(np.argmax(x)), int(np.argmin(x)), int(np.argmin(np.abs(x)))]
    batch = tuple(np.concatenate([b[:45], p[picks]]) for b, p in zip(c.batch, pool.batch))
    return c._replace(batch=batch)


@functools.lru_cache(maxsize=None)
def fixture(key):
    """The Case of ``key``; computed once, never written to."""
    if key in WIDTH_CASES:
        return make_case(key, WIDTH_CASES[key], 3, 1000 + WIDTH_CASES[key])
    if key in DEPTH_CASES:
        return make_case(key, 16, DEPTH_CASES[key], 2000 + DEPTH_CASES[key])
    if key in HUB_CASES:
        return hub_fixture(key)
    if key in THRESHOLD_CASES or key == BIG_CASE:
        n = MAX_SLICED_NODES if key == BIG_CASE else THRESHOLD_CASES[key]
        U = n * 3 // 5
        return make_case(key, 4, 1 if key == BIG_CASE else 2, 3000 + n % 1000, U=U, I=n - U, n_edges=60000, B=64)
    if key == "general":
        rng = np.random.default_rng(41)
        return make_case(key, 16, 2, 41, adj=general_graph(rng, 37, 29, 250))
    if key in ("seam", "seam_predict"):
        U, I, B = 1000, 900, GRID_WAVES + 1
        rng = np.random.default_rng(51)
        pairs = None
        if key == "seam_predict":
            pairs = (rng.integers(0, U, B), rng.integers(0, I, B))
        return make_case(key, 16, 2, 51, U=U, I=I, n_edges=6000, batch=seam_batch(np.random.default_rng(52), U, I, B),
                         pairs=pairs)
    if key == "one_triple":
        return make_case(key, 16, 2, 61, batch=([5], [2], [11]))
    if key == "one_user":
        rng = np.random.default_rng(62)
        return make_case(key, 64, 2, 62, batch=(np.full(64, 7), rng.integers(0, 29, 64), rng.integers(0, 29, 64)))
    if key == "pos_eq_neg":
        c = make_case(key, 16, 2, 63)
        neg = c.batch[2].copy()
        neg[::2] = c.batch[1][::2]
        neg[1::2] = np.where(neg[1::2] == c.batch[1][1::2], (neg[1::2] + 1) % c.I, neg[1::2])
        return c._replace(batch=(c.batch[0], c.batch[1], neg))
    if key == "saturated":
        return saturated_fixture()
    if key == "decay0":
        return make_case(key, 16, 2, 64, decay=0.0)
    if key == "keep1":
        return make_case(key, 16, 2, 65, keep_pro=1.0)
    if key in DEVICE_CASES:      # (the mask is a stand-in for the host conditions: the GPU test reads the draw back)
        return make_case(key, DEVICE_CASES[key], 2, 4000 + DEVICE_CASES[key])
    if key in STAGED_CASES:
        return make_case(key, 100, STAGED_CASES[key], 5000 + STAGED_CASES[key], U=300, I=200, n_edges=4000, B=256)
    raise KeyError(key)


# ---- the yardstick --------------------------------------------------------------------------------------------------
def dropped_graph(c, mask="case"):
    mask = c.mask if isinstance(mask, str) else mask
    return olg.apply_edge_dropout(c.adj, mask, c.keep_pro)


def table64(w, adj, L):
    """The eval-mode propagated table [N, D] in fp64."""
    with float64_oracle(olg):
        ua, ia = olg.propagate(to64(w), adj.astype(np.float64), L)
    return np.concatenate([ua, ia], axis=0)


def reference_of(c, mask="case", w=None):
    """``Ref`` of a case from ``oracle.lightgcn_numpy``, with the keep mask (and weights) given instead of its own."""
    w = c.w if w is None else w
    dropped = dropped_graph(c, mask)
    with np.errstate(over="ignore"):      # (saturated: exp(-x) of the sigmoid overflows fp32 to inf, 1 / inf = 0)
        loss32, g32 = olg.lightgcn_grads(w, dropped, c.L, *c.batch, c.decay)
    with float64_oracle(olg):
        loss64, g64 = olg.lightgcn_grads(to64(w), dropped.astype(np.float64), c.L, *c.batch, c.decay)
    return Ref(loss64, g64, loss32, g32, table64(w, c.adj, c.L))


@functools.lru_cache(maxsize=None)
def reference(key):
    """``Ref`` of ``fixture(key)``: fp64 and fp32 loss and gradients of the training step under the case's mask, and
    the fp64 eval-mode table; computed once, never written to."""
    return reference_of(fixture(key))


def tolerances(ref):
    """Per tensor what ``assert_grads_as_accurate`` allows."""
    return {k: REL * float(np.abs(ref.g64[k]).max()) + 2.0 * float(np.abs(ref.g32[k] - ref.g64[k]).max())
            for k in ref.g64}


# ---- the restatement, with a defect ---------------------------------------------------------------------------------
def applies(c, defect):
    """Whether ``defect`` names something the case's shape has (and the case is one this module holds to seeing it)."""
    width, factored, _ = FORM_TABLE[c.key]
    x_max = float(saturated_stats(c).max()) if c.key == "saturated" else 0.0
    return {
        "last_col": c.key in WIDTH_CASES,
        "cols64": c.D > NPL_STEPS[0],
        "cols128": c.D > NPL_STEPS[1],
        "mean_over_l": c.L >= 1,
        "last_layer_fwd": c.L >= 1,
        "last_layer_bwd": c.L >= 1,
        "l2_row": c.decay > 0 and c.D >= 64,     # (the L2 term is decay * D of the loss: below REL at narrow widths)
        "col_factor": factored and c.L >= 1,
        "triple_8192": len(c.batch[0]) > GRID_WAVES,
        "dup_overwrite": c.key in ("one_user", "seam"),
        "softplus_inf": x_max > OVERFLOW,
        "empty_stale": c.key in HUB_CASES,
        "spill_lost": c.key in HUB_CASES,
        "edge_kept_bwd": c.keep_pro < 1.0 and c.L >= 1,
    }[defect]


def restate(c, dt=np.float64, defect=None, mask="case", train=True):
    """A local copy of ``oracle.lightgcn_numpy``'s step on a Case: ``(loss, grads, table)``, the table being the
    propagated layer mean [N, D] of the graph used (``train`` False: the whole graph, the eval-mode forward alone).
    Without a defect it is that module's computation, operation for operation; with one, the intermediate arrays are
    altered the way a kernel with that defect would leave them."""
    assert defect is None or defect in DEFECTS
    T = dt
    U, N, L, D = c.U, c.U + c.I, c.L, c.D
    mask = c.mask if isinstance(mask, str) else mask
    keep = np.asarray(mask, dtype=bool).copy() if train else np.ones(c.adj.nnz, bool)
    if defect == "spill_lost":            # the hub row keeps the slots of its first window only
        keep[c.adj.indptr[U + HUB] + WINDOW_SLOTS:c.adj.indptr[U + HUB + 1]] = False
    if train:
        adj = olg.apply_edge_dropout(c.adj, keep, c.keep_pro).astype(T)
    else:
        adj = c.adj.astype(T) if keep.all() else olg.apply_edge_dropout(c.adj, keep, 1.0).astype(T)
    w = {k: v.astype(T) for k, v in c.w.items()}
    empty = empty_rows(c)

    def forward_pass(e):
        y = (adj @ e).astype(T)
        if defect == "empty_stale":       # a row without edges keeps what the buffer held: here the row's own source
            y[empty] = e[empty]
        return y

    e = np.concatenate([w["user_embedding.weight"], w["item_embedding.weight"]], axis=0).astype(T)
    acc = e.copy()
    for _ in range(L - 1 if defect == "last_layer_fwd" else L):
        e = forward_pass(e)
        acc += e
    inv = T(L if defect == "mean_over_l" else L + 1)
    out = (acc / inv).astype(T)
    if not train:
        return None, None, out
    users, pos, neg = c.batch
    B = T(len(users))
    cols = np.ones(D, dtype=T)            # the columns the loss kernel sees
    if defect == "last_col":
        cols[D - 1:] = 0
    elif defect == "cols64":
        cols[NPL_STEPS[0]:] = 0
    elif defect == "cols128":
        cols[NPL_STEPS[1]:] = 0
    live = np.ones(len(users), dtype=T)   # the triples it sees
    if defect == "triple_8192":
        live[GRID_WAVES:] = 0
    gated = defect in ("last_col", "cols64", "cols128", "triple_8192")
    ua, ia = out[:U], out[U:]
    ue, pe, ne = ua[users], ia[pos], ia[neg]
    if gated:
        ue, pe, ne = ue * cols, pe * cols, ne * cols
    pos_s = (ue * pe).sum(axis=1, dtype=T)
    neg_s = (ue * ne).sum(axis=1, dtype=T)
    x = (neg_s - pos_s).astype(T)
    if defect == "softplus_inf":          # log1pf(expf(x)) in fp32 without the x > 20 branch
        with np.errstate(over="ignore"):
            sp_x = np.log1p(np.exp(x.astype(np.float32))).astype(T)
    else:
        sp_x = np.where(x > 20, x, np.log1p(np.exp(np.minimum(x, T(20)), dtype=T), dtype=T)).astype(T)
    u0, p0, n0 = w["user_embedding.weight"][users], w["item_embedding.weight"][pos], w["item_embedding.weight"][neg]
    if defect == "l2_row":
        n0 = np.zeros_like(n0)
    if gated:
        sp_x = sp_x * live
        u0, p0, n0 = (r * cols * live[:, None] for r in (u0, p0, n0))
    mf = T(sp_x.mean(dtype=T))
    reg = T(0.5) * ((u0 ** 2).sum(dtype=T) + (p0 ** 2).sum(dtype=T) + (n0 ** 2).sum(dtype=T)) / B
    reg = T(reg * T(c.decay))
    with np.errstate(over="ignore"):
        dx = (T(1) / (T(1) + np.exp(-x, dtype=T)) / B).astype(T)
    if gated:
        dx = dx * live
    d_out = np.zeros((N, D), dtype=T)

    def scatter(dst, rows, vals):
        if defect == "dup_overwrite":     # of the triples that share a row, the last one's term alone arrives
            once = np.zeros_like(dst)
            once[rows] = vals
            dst += once
        else:
            np.add.at(dst, rows, vals)

    scatter(d_out, users, dx[:, None] * (ne - pe))
    scatter(d_out, pos + U, -dx[:, None] * ue)
    scatter(d_out, neg + U, dx[:, None] * ue)
    if gated:
        d_out = d_out * cols
    d_out /= inv
    if defect == "edge_kept_bwd":         # the transposed passes do not look at the keep bytes
        at = olg.apply_edge_dropout(c.adj, np.ones(c.adj.nnz, bool), c.keep_pro).astype(T).T.tocsr()
    else:
        at = adj.T.tocsr()
    g_e, cur = d_out.copy(), d_out
    for l in range(L - 1 if defect == "last_layer_bwd" else L):
        if defect == "col_factor" and l == 0:     # the first transposed pass takes its source without the column factor
            cs = factors(c.adj.T.tocsr())[1].astype(T)
            cur = cur / cs[:, None]
        cur = (at @ cur).astype(T)
        g_e += cur
    cc = T(c.decay) / B
    np.add.at(g_e, users, cc * u0)
    np.add.at(g_e, pos + U, cc * p0)
    np.add.at(g_e, neg + U, cc * n0)
    grads = {"user_embedding.weight": g_e[:U], "item_embedding.weight": g_e[U:]}
    return float(mf + reg), grads, out


def defect_margin(key, defect):
    """The largest move of an asserted quantity under ``defect`` in units of what the GPU test allows it: the loss
    (REL), every gradient (``tolerances``), the eval-mode table (REL of its scale); with the fp64 restatement alone.
    Returns ``(margin, the quantity that moved most)``; a quantity that stops being finite counts as infinitely far."""
    c, ref = fixture(key), reference(key)
    loss, g, _ = restate(c, defect=defect)
    _, _, table = restate(c, defect=defect, train=False)
    tol = tolerances(ref)
    moves = {"loss": abs(loss - ref.loss64) / (REL * abs(ref.loss64)),
             "table": float(np.abs(table - ref.table64).max()) / (REL * float(np.abs(ref.table64).max()))}
    for k in ref.g64:
        moves[k] = float(np.abs(g[k] - ref.g64[k]).max()) / tol[k]
    moves = {k: (v if np.isfinite(v) else np.inf) for k, v in moves.items()}
    worst = max(moves, key=moves.get)
    return moves[worst], worst


def other_order_ratio(key, seed):
    """The fp32 oracle on the same problem with users and items renumbered at random (the same function in exact
    arithmetic; in fp32 every sum over nodes, edges and triples runs in another order), held to the bound the kernel
    is held to: the largest distance of one of its gradients from the exact one in units of ``tolerances``."""
    c, ref = fixture(key), reference(key)
    rng = np.random.default_rng(seed)
    pu, pi = rng.permutation(c.U), rng.permutation(c.I)            # new user j is old user pu[j]
    perm = np.concatenate([pu, c.U + pi])
    dropped = dropped_graph(c)[perm][:, perm].tocsr()
    dropped.sort_indices()
    w = {"user_embedding.weight": c.w["user_embedding.weight"][pu],
         "item_embedding.weight": c.w["item_embedding.weight"][pi]}
    iu, ii = np.argsort(pu), np.argsort(pi)
    order = rng.permutation(len(c.batch[0]))
    batch = (iu[c.batch[0]][order], ii[c.batch[1]][order], ii[c.batch[2]][order])
    _, g = olg.lightgcn_grads(w, dropped, c.L, *batch, c.decay)
    back = {}
    for k, p in (("user_embedding.weight", pu), ("item_embedding.weight", pi)):
        back[k] = np.empty_like(g[k])
        back[k][p] = g[k]
    tol = tolerances(ref)
    ratio = {k: float(np.abs(back[k] - ref.g64[k]).max()) / tol[k] for k in ref.g64}
    worst = max(ratio, key=ratio.get)
    return ratio[worst], worst
