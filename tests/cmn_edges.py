"""Fixtures of the CMN edge tests, shared by tests/test_cmn_edges_host.py (which shows on the CPU that the inputs can see
one row lost at a round's seam, and that the fp32 restatement is a fair yardstick on them) and
tests/test_cmn_edges_gpu.py (which runs the kernel on those very inputs).  No tests here.

Almost every index of ``cmn_sample_kernel`` depends on three numbers derived from the width D (``derived``): G lanes per
row, whether a lane reads a ``float4`` (VEC), and Dp lanes per row in the scatter.  ``WIDTH_CASES`` holds one width per
(G, VEC) pair the goldens and tests/test_cmn_gpu.py leave out, each with lists at the seams of ITS round of 4 R rows;
the other cases reach the block-stride loop, a softmax with real dynamic range, a neighbour listed more than once and a
saturated BPR term.

The weights are ``synthetic``'s (tests/test_cmn_gpu.py draws its own from the same recipe) with ``user_memory`` scaled so
that the hop-0 logits spread over about +-3 instead of +-0.3: every rescale factor exp(m - m_new) of the online softmax
is then far from 1 while every probability of a list still counts in some gradient."""
import collections
import functools

import numpy as np

import cmn_numpy as cn
from helpers import REL, float64_oracle, to64
from test_oracle_golden_cmn import exact_grads, term_floors

KEYS = cn.KEYS
HOP_B = "mem_layer.hop_mapping.1.bias"
LAM, CLIP = 0.001, 5.0
WAVE, WAVES_PER_BLOCK, MAX_BLOCKS = 64, 4, 1024      # kWave, kWavesPerBlock, kCmnMaxBlocks

# D -> (G, R = rows per wave, VEC, Dp, rows per atomic instruction), written out by hand; test_cmn_edges_host.py holds
# ``derived`` (the restatement of cmn_lanes_per_row and of the scatter's layout) to it
DERIVED = {4: (1, 64, True, 4, 16), 8: (2, 32, True, 8, 8), 10: (4, 16, False, 16, 4), 12: (4, 16, True, 16, 4),
           30: (8, 8, False, 32, 2), 50: (16, 4, False, 64, 1), 65: (32, 2, False, 64, 1), 68: (32, 2, True, 64, 1),
           130: (64, 1, False, 64, 1), 132: (64, 1, True, 64, 1)}
WIDTH_CASES = sorted(DERIVED)
COVERED_ELSEWHERE = (7, 16, 20, 64, 100, 256)         # the widths of the goldens and of tests/test_cmn_gpu.py
STRIDE_CASE = "stride"
SHARP_CASES = [(D, shape) for D in (16, 50) for shape in ("ascending", "descending", "late_peak")]
DUPLICATE_CASE = "duplicate"
SATURATED_CASE = "saturated"

LOGIT_STD = 1.5            # hop-0 logits of the width cases: about +-3 at two standard deviations
SPARE_USERS = 8            # the last users of a width case are in no list and are no sample's user
HUB = 0                    # the user in most lists

# The sharp cases: hop-0 logits along the one long list from -SHARP_TOP to +SHARP_TOP for the positive item (a spread of
# 79 with |logit| <= 40), 0.9 of that for the negative item on the same list (71.1), 0.95 for the third item; the late
# peak stands SHARP_TOP above a floor of -SHARP_FLOOR (69.5, 62.6 on the negative side).  The fp32 restatement holds
# REL of the fp64 one at these values (test_fp32_restatement_is_a_fair_yardstick: 1.1e-6 of a tensor's scale at worst),
# so the spread was not narrowed.
SHARP_TOP, SHARP_FLOOR = 39.5, 30.0
SHARP_NEG, SHARP_THIRD = 0.9, 0.95
# |M[u] + E[0]| of the sharp cases' query is set to sqrt(40), so that the query and the list's rows t_j z0 / |z0|^2 are
# equally long.  A shorter query makes the rows longer, and the flat rows of the late-peak case share the component
# -SHARP_FLOOR z0 / |z0|^2: in dz = sum_j da_j M[n_j] it multiplies sum_j da_j, which is 0 in exact arithmetic and a
# rounding residual in fp32 -- a different one for each legal way of writing the softmax's backward.  At |z0| = 3 the
# restatement with delta = do . o (as the kernel computes it) in place of sum_j p_j dp_j is 3.3x the gradient bound away
# from the exact hop-mapping gradient at D = 16, at sqrt(40) 0.23x (test_both_softmax_backward_forms_meet_the_bound).
SHARP_Z0_NORM = 40.0 ** 0.5
# The saturated case: out.weight scaled until |s+ - s-| = SATURATED_X in fp64 (>= 30 as asked; at 32 the x <= -30
# sample still has a gradient of norm 0.86, by 40 it has sunk below the L2 term's).  The fp32 restatement holds REL at
# every |x| of SATURATED_SCAN (worst 4.9e-6 of a tensor's scale, at 36), so the threshold was not lowered.  The seed is
# the one of 0 .. 63 whose two unscaled scores have opposite signs and differ most: x = s+ - s- then loses nothing to
# cancellation once out.weight is scaled up (by 154, to |out.weight| <= 86).
SATURATED_X = 32.0
SATURATED_SCAN = (30.5, 32.0, 36.0, 40.0, 50.0, 60.0, 80.0)
SATURATED_SEED = 37
SATURATED_CLIP = 1e9       # the clip is off

Case = collections.namedtuple("Case", "key D w rowptr col triples batch lam clip")


def derived(D):
    """(G, R, VEC, Dp, rows_per_instr) as csrc/cmn.hip derives them from the width."""
    g = 1
    while 4 * g < D:                                   # cmn_lanes_per_row
        g <<= 1
    dp = WAVE if D >= WAVE else 1 << (D - 1).bit_length()
    return g, WAVE // g, D % 4 == 0, dp, WAVE // dp


def width_lengths(D):
    """The list lengths of a width case: below a wave's share (L < R: whole waves get no row), one past it, the seams of
    a round of 4 R rows, two rounds and one row, and two ordinary lengths in between."""
    R = derived(D)[1]
    seams = {1, R + 1, 4 * R - 1, 4 * R, 4 * R + 1, 8 * R + 1} | ({R - 1} if R > 1 else set())
    return sorted(seams | {5 * R + 1, 7 * R})


def draw_weights(rng, U, I, D, scale):
    shapes = {"user_memory.weight": (U, D), "item_memory.weight": (I, D), "user_output.weight": (U, D),
              "mem_layer.hop_mapping.1.weight": (D, D), "mem_layer.hop_mapping.1.bias": (D,),
              "dense.weight": (D, 2 * D), "dense.bias": (D,), "out.weight": (1, D)}
    return {k: (rng.standard_normal(shapes[k]) * scale).astype(np.float32) for k in KEYS}


def csr_of(lists):
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return rowptr, np.concatenate(lists).astype(np.int64)


def synthetic(U, D, lengths, B, seed, scale=0.3):
    """Random lists without repeats, every tensor N(0, scale^2), sample b's positive item b mod I and its user one of
    that item's list: ``(w, rowptr, col, (users, pos, neg))``."""
    rng = np.random.default_rng(seed)
    I = len(lengths)
    lists = [rng.permutation(U)[:n] for n in lengths]
    rowptr, col = csr_of(lists)
    w = draw_weights(rng, U, I, D, scale)
    pos = np.arange(B) % I
    neg = (pos + 1 + rng.integers(0, I - 1, B)) % I
    users = np.array([lists[p][rng.integers(0, len(lists[p]))] for p in pos])
    return w, rowptr, col, (users, pos, neg)


def memory_scale(D, item_scale, logit_std=LOGIT_STD):
    """The std s of user_memory at which a hop-0 logit (M[u] + E[i]) . M[n] has std ``logit_std``:
    s^2 (s^2 + item_scale^2) D = logit_std^2."""
    e2 = item_scale ** 2
    return float(np.sqrt((-e2 + np.sqrt(e2 * e2 + 4 * logit_std ** 2 / D)) / 2))


def pre_activations(w, batch, lam=LAM):
    """{"pre1", "preh"}: both queries' pre-activations of the fp64 evaluation, [2 B, D] each."""
    with float64_oracle(cn):
        _, _, caches = cn.cmn_grads(to64(w), batch, lam, with_cache=True)
    return {layer: np.concatenate([c[layer] for c in caches]) for layer in ("pre1", "preh")}


def settle_biases(w, batch):
    """No pre-activation of the exact evaluation within 1e-4 of its layer's scale from zero (the rule of
    test_fixtures_hold_what_the_kernel_can_get_wrong: a unit whose sign fp32 rounding decides tests nothing): a unit
    that has one gets its bias moved by the smallest multiple of 4e-4 of the scale that clears all 2 B queries.  A bias
    shifts its own unit's pre-activation only, so the hop mapping is settled first and the dense layer after it."""
    for layer, key in (("pre1", HOP_B), ("preh", "dense.bias")):
        pre = pre_activations(w, batch)[layer]
        step = 4e-4 * float(np.abs(pre).max())
        for r in np.nonzero(np.abs(pre).min(axis=0) < step)[0]:
            shift = next(s for k in range(1, 1000) for s in (k * step, -k * step)
                         if np.abs(pre[:, r] + s).min() >= step)
            w[key][r] += np.float32(shift)
    return w


def width_fixture(D):
    R = derived(D)[1]
    lengths = width_lengths(D)
    I, U = len(lengths), 8 * R + 40
    rng = np.random.default_rng(7000 + D)
    listed = U - SPARE_USERS
    lists = [rng.permutation(listed)[:n] for n in lengths]
    for lst in lists:                                  # the hub in every list of three rows or more, away from the seams
        if len(lst) >= 3 and HUB not in lst:
            lst[len(lst) // 2] = HUB
    rowptr, col = csr_of(lists)
    w = draw_weights(rng, U, I, D, 0.3)
    w["user_memory.weight"] *= np.float32(memory_scale(D, 0.3) / 0.3)
    # every length once as a positive and once as a negative list; one more sample on the two longest seam lists
    pos = np.concatenate([np.arange(I), [lengths.index(4 * R + 1)]])
    neg = np.concatenate([(np.arange(I) + 1) % I, [lengths.index(8 * R + 1)]])
    users = rng.integers(1, listed, len(pos))
    users[0] = lists[pos[0]][0]                        # u in N(i+): the one-row list is its own user's
    triples = (users.astype(np.int64), pos.astype(np.int64), neg.astype(np.int64))
    batch = cn.padded_batch(rowptr, col, *triples)
    return Case(D, D, settle_biases(w, batch), rowptr, col, triples, batch, LAM, CLIP)


def stride_fixture():
    """1030 samples at D = 8: the grid is capped at 1024 blocks, so blocks 0 .. 5 run a second sample on the same LDS.
    Weights of std 0.5: at 0.3 the 2060 terms of out.weight's gradient cancel so far that the restatement's own
    sequential fp32 sum over the batch is 1e-5 .. 4e-5 of the tensor's scale from the exact value, and no yardstick."""
    D, B = 8, MAX_BLOCKS + 6
    w, rowptr, col, triples = synthetic(40, D, [1, 2, 3, 4, 5, 3], B, seed=42, scale=0.5)
    triples = tuple(np.asarray(t, dtype=np.int64) for t in triples)
    return Case(STRIDE_CASE, D, w, rowptr, col, triples, cn.padded_batch(rowptr, col, *triples), LAM, CLIP)


def sharp_targets(D, shape):
    """The hop-0 logits asked of the positive query along the long list of 4 R x 3 + 1 rows."""
    L = 12 * derived(D)[1] + 1
    if shape == "ascending":                           # every round raises the running maximum
        return np.linspace(-SHARP_TOP, SHARP_TOP, L)
    if shape == "descending":                          # the first row dominates
        return np.linspace(SHARP_TOP, -SHARP_TOP, L)
    t = np.full(L, -SHARP_FLOOR)                       # flat, one peak in the last full round
    t[L - 3] = SHARP_TOP
    return t


def sharp_fixture(D, shape):
    """One long list shared by items 0 and 1 (sample 0's positive and negative list are the same list) and, rotated by
    R + 1 rows, item 2's.  With z0 = M[u] + E[0] (grown to SHARP_Z0_NORM), row j of the list is
    M[n_j] = t_j z0 / |z0|^2 + r_j, so the logits are the targets t.  E[1] and E[2] put the other items' queries at
    0.9 z0 + v and 0.95 z0 - v, v normal to z0 and as long: their logits are 0.9 t and 0.95 t, yet the queries differ
    enough for s+ - s- not to vanish.  Every r_j is normal to z0 and to v."""
    R = derived(D)[1]
    t = sharp_targets(D, shape)
    L = len(t)
    U, user = L + 8, L
    rng = np.random.default_rng(9000 + D + len(shape))
    order = rng.permutation(L)
    lists = [order, order.copy(), np.roll(order, R + 1)]
    rowptr, col = csr_of(lists)
    w = draw_weights(rng, U, 3, D, 0.3)
    M, E = w["user_memory.weight"], w["item_memory.weight"]
    z0 = M[user].astype(np.float64) + E[0].astype(np.float64)
    grow = SHARP_Z0_NORM / float(np.linalg.norm(z0))
    M[user], E[0] = (M[user] * grow).astype(np.float32), (E[0] * grow).astype(np.float32)
    z0 = M[user].astype(np.float64) + E[0].astype(np.float64)
    zz = float(z0 @ z0)
    v = rng.standard_normal(D)
    v -= (v @ z0) * z0 / zz
    v *= np.sqrt(zz / float(v @ v))
    noise = M[order].astype(np.float64)
    noise -= np.outer(noise @ z0, z0) / zz + np.outer(noise @ v, v) / zz
    M[order] = (np.outer(t, z0) / zz + noise).astype(np.float32)
    E[1] = (SHARP_NEG * z0 + v - M[user]).astype(np.float32)
    E[2] = (SHARP_THIRD * z0 - v - M[user]).astype(np.float32)
    triples = (np.array([user, user]), np.array([0, 2]), np.array([1, 0]))
    return Case((D, shape), D, w, rowptr, col, triples, cn.padded_batch(rowptr, col, *triples), LAM, CLIP)


def duplicate_fixture():
    """Padded form only.  Sample 0's positive list holds one neighbour at slots 2, 7 and 11 (its last) among nine
    distinct others; sample 1's negative list is one user five times."""
    D, U = 20, 60
    rng = np.random.default_rng(2020)
    lists = [rng.permutation(U - 2)[:n] for n in (12, 7, 5, 9)]
    rowptr, col = csr_of(lists)
    w = draw_weights(rng, U, 4, D, 0.3)
    w["user_memory.weight"] *= np.float32(memory_scale(D, 0.3) / 0.3)
    triples = (np.array([lists[0][1], 5, 17]), np.array([0, 1, 2]), np.array([1, 2, 3]))
    u, p, n, pn, pl, nn_, nl = cn.padded_batch(rowptr, col, *triples)
    pn[0, [2, 7, 11]] = U - 1
    nn_[1, :5] = U - 2
    return Case(DUPLICATE_CASE, D, w, rowptr, col, None, (u, p, n, pn, pl, nn_, nl), LAM, CLIP)


def saturated_fixture(x=None):
    """Two samples, the second the first with positive and negative swapped; out.weight scaled to |x| = SATURATED_X."""
    D, U = 8, 30
    x_target = SATURATED_X if x is None else x
    w, rowptr, col, _ = synthetic(U, D, [6, 9], 2, seed=SATURATED_SEED)
    triples = (np.array([3, 3]), np.array([0, 1]), np.array([1, 0]))
    batch = cn.padded_batch(rowptr, col, *triples)
    x = score_differences(w, batch)
    w["out.weight"] = (w["out.weight"].astype(np.float64) * (x_target / abs(x[0]))).astype(np.float32)
    return Case(SATURATED_CASE, D, w, rowptr, col, triples, batch, LAM, SATURATED_CLIP)


def scores64(w, batch):
    """(s+, s-) of the fp64 evaluation."""
    with float64_oracle(cn):
        sp, _ = cn.cmn_query(to64(w), batch[0], batch[1], batch[3], batch[4])
        sn, _ = cn.cmn_query(to64(w), batch[0], batch[2], batch[5], batch[6])
    return sp, sn


def score_differences(w, batch):
    sp, sn = scores64(w, batch)
    return sp - sn


def hop_logits(w, batch, side, hop):
    """The fp64 logits z_hop . M[n_j] of every sample's list on ``side`` (0 positive, 1 negative): [B, L], NaN in the
    padding."""
    nbr, lens = (batch[3], batch[4]) if side == 0 else (batch[5], batch[6])
    with float64_oracle(cn):
        _, c = cn.cmn_query(to64(w), batch[0], batch[1 + side], nbr, lens)
    a = np.einsum("bd,bld->bl", c["z0"] if hop == 0 else c["z1"], c["Mn"])
    return np.where(c["mask"], a, np.nan)


@functools.lru_cache(maxsize=None)
def fixture(key):
    """The Case of a width (an int of WIDTH_CASES), of a ``(D, shape)`` of SHARP_CASES or of one of the named cases;
    computed once, never written to."""
    if isinstance(key, tuple):
        return sharp_fixture(*key)
    if isinstance(key, str):
        return {STRIDE_CASE: stride_fixture, DUPLICATE_CASE: duplicate_fixture, SATURATED_CASE: saturated_fixture}[key]()
    return width_fixture(key)


def _hop_backward_from_output(z, p, do, c):
    """``cn._hop_backward`` with the softmax's backward written as the kernel writes it: da_j = p_j (dp_j - do . o),
    o = sum_j p_j C[n_j], instead of p_j (dp_j - sum_k p_k dp_k).  The same function in exact arithmetic."""
    F = cn.F32
    dp = np.einsum("bd,bld->bl", do, c["Cn"]).astype(F)
    o = np.einsum("bl,bld->bd", p, c["Cn"]).astype(F)
    da = (p * (dp - (do * o).sum(axis=1, keepdims=True, dtype=F))).astype(F)
    return da[:, :, None] * z[:, None, :], p[:, :, None] * do[:, None, :], np.einsum("bl,bld->bd", da, c["Mn"]).astype(F)


def restated32(c, delta_from_output=False):
    """``(loss32, total32, g32 clipped)`` of the fp32 restatement on a Case; ``delta_from_output``: with the softmax's
    backward in the kernel's form (``_hop_backward_from_output``)."""
    saved = cn._hop_backward
    cn._hop_backward = _hop_backward_from_output if delta_from_output else saved
    try:
        loss32, g32 = cn.cmn_grads(c.w, c.batch, c.lam)
    finally:
        cn._hop_backward = saved
    total32, g32 = cn.clip_grads(g32, c.clip)
    return loss32, total32, g32


@functools.lru_cache(maxsize=None)
def reference(key):
    """``(loss64, g64 clipped, total64, g32, floors)`` of ``fixture(key)``."""
    c = fixture(key)
    loss64, g64, total64 = exact_grads(c.w, c.batch, c.lam, c.clip)
    return loss64, g64, total64, restated32(c)[2], term_floors(c.w, c.batch, c.lam, c.clip)


def tolerances(g32, g64, floors):
    """Per tensor what ``helpers.assert_grads_as_accurate`` allows with ``floors``."""
    return {k: REL * max(float(np.abs(g64[k]).max()), floors[k]) + 2.0 * float(np.abs(g32[k] - g64[k]).max())
            for k in g64}


def drop_margin(D, length, row):
    """Drop neighbour ``row`` of the width case's list of ``length`` rows: the largest move of a tensor of the fp64
    gradient, in units of that tensor's tolerance."""
    c = fixture(D)
    _, g64, _, g32, floors = reference(D)
    tol = tolerances(g32, g64, floors)
    item = width_lengths(D).index(length)
    lists = [c.col[c.rowptr[i]:c.rowptr[i + 1]] for i in range(len(c.rowptr) - 1)]
    lists[item] = np.delete(lists[item], row)
    rowptr, col = csr_of(lists)
    _, moved, _ = exact_grads(c.w, cn.padded_batch(rowptr, col, *c.triples), c.lam, c.clip)
    return max(float(np.abs(moved[k] - g64[k]).max()) / tol[k] for k in KEYS)
