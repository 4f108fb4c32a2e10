"""Fixtures of the PairwiseGMF edge tests, shared by tests/test_pgmf_edges_host.py (which shows on the CPU that the inputs
can see one lost triple, one lost block of grad v and one lost column, and that the fp32 restatement is a fair yardstick
on them) and tests/test_pgmf_edges_gpu.py (which runs csrc/pgmf.hip on those very inputs).  No tests here.

``pgmf_bpr_grad_kernel`` lays a row out as columns ``lane + 64 k``, k < 4, guarded by ``c < D``, runs one triple per wave
and trip on a grid capped at 1024 blocks of 4 waves, and leaves one [D] partial of grad v per block;
``pgmf_finish_kernel`` folds those partials in ``n_slices = 1024 // D`` slices with a 4-way unrolled loop and a remainder
loop.  ``WIDTH_CASES`` holds the widths with one live column in an upper slot, one short of a full slot and below 8, each
with batch sizes that put the block count at the seams of ITS unrolling; the other cases reach the second trip of the
grid-stride loop, both ``continue``s of it, a saturated BPR term and rows every triple collides on.

The weights are N(0, 1) rows with v ~ N(0, 1 / D): the pre-activations v . (u * i) are O(1), so that about a quarter of
the triples have both ReLUs closed, about half have one closed, and sigmoid(s+ - s-) is far from 0, 1/2 and 1."""
import collections
import functools

import numpy as np

from helpers import REL, float64_oracle, to64
from oracle import pgmf_numpy as pn

KEYS = pn.KEYS
UM, IM, V = KEYS
LAM = 1e-3
CLIP = 0.01                # active on every case but the all-closed one (test_clip_is_active)
NO_CLIP = 1e9
WAVE, WAVES_PER_BLOCK, MAX_BLOCKS, MAX_NPL, FINISH_THREADS = 64, 4, 1024, 4, 1024   # kWave .. kFinishThreads
TRIP = MAX_BLOCKS * WAVES_PER_BLOCK                    # triples per trip of the grid-stride loop

WIDTH_CASES = (1, 3, 63, 65, 129, 193, 255)
COVERED_ELSEWHERE = (8, 16, 20, 64, 100, 128, 256)     # the widths of the goldens and of tests/test_pgmf_gpu.py
# live columns per slot k, written out by hand; test_pgmf_edges_host.py holds ``live_columns`` to it
LIVE = {1: [1, 0, 0, 0], 3: [3, 0, 0, 0], 63: [63, 0, 0, 0], 65: [64, 1, 0, 0], 129: [64, 64, 1, 0],
        193: [64, 64, 64, 1], 255: [64, 64, 64, 63]}
SMALL_BLOCKS = 70          # where n_slices is large (D = 1, 3) only block counts below this are kept ...
TINY_BATCHES = (1, 2, 3, 5)                            # ... plus these: one block with idle waves, and two blocks

USERS, ITEMS, SPARE = 40, 30, 4                        # the last SPARE rows of either table are in no triple
GATE_MARGIN = 1e-3         # no pre-activation of the exact evaluation closer to zero (they are O(1)): a gate whose sign
#                            fp32 rounding decides tests nothing

STRIDE_CASE, CLOSED_CASE, SATURATED_CASE = "stride", "closed", "saturated"
SAME_ITEM_CASE, ONE_USER_CASE, HOT_CASE = "pos_is_neg", "one_user", "hot"
NAMED_CASES = (STRIDE_CASE, CLOSED_CASE, SATURATED_CASE, SAME_ITEM_CASE, ONE_USER_CASE, HOT_CASE)
STRIDE_D, STRIDE_B, STRIDE_TABLES = 65, TRIP + 6, (1500, 1200)
# wave w of the grid runs triples w and TRIP + w: (kind of the first, kind of the second)
STRIDE_PAIRS = (("open", "open"), ("closed", "open"), ("open", "closed"), ("pos_only", "neg_only"),
                ("closed", "closed"), ("same_item", "open"))
# The saturated case: v scaled until the largest |s+ - s-| of the batch is SATURATED_X in fp64 (every triple is in the
# batch with its positive and negative item swapped as well, so x comes with both signs).  At x = -32 the loss term is
# 27.6 and its derivative sigmoid'(x) / (sigmoid(x) + 1e-12) = 0.0125; at +32 sigmoid rounds to 1 in fp32.  The fp32
# restatement holds REL at every |x| of SATURATED_SCAN (test_saturation_threshold_the_restatement_holds), so the
# magnitude was not lowered.
SATURATED_X = 32.0
SATURATED_SCAN = (30.5, 32.0, 36.0, 40.0, 50.0, 60.0, 80.0)
SATURATED_D = 65

Case = collections.namedtuple("Case", "key D w batch lam clip")
Ref = collections.namedtuple("Ref", "loss64 g64 total64 coef64 loss32 g32 total32 g32_clipped")


def live_columns(D):
    return [sum(lane + WAVE * k < D for lane in range(WAVE)) for k in range(MAX_NPL)]


def n_blocks(B):
    """pgmf_grid."""
    return max(1, min(MAX_BLOCKS, -(-B // WAVES_PER_BLOCK)))


def finish_split(D, blocks):
    """``(n_slices, main, rest)``: how often ``pgmf_finish_kernel``'s slices together run the body of the 4-way
    unrolled loop and of the remainder loop over ``blocks`` partials."""
    n_slices = FINISH_THREADS // D
    main = rest = 0
    for sl in range(n_slices):
        b = sl
        while b + 3 * n_slices < blocks:
            main, b = main + 1, b + 4 * n_slices
        while b < blocks:
            rest, b = rest + 1, b + n_slices
    return n_slices, main, rest


def width_batch_sizes(D):
    """Batch sizes whose block count ceil(B / 4) sits at 1 and at the seams of the finish kernel's unrolling for this
    width's n_slices."""
    ns = FINISH_THREADS // D
    blocks = {min(b, MAX_BLOCKS) for b in (1, ns - 1, ns, ns + 1, 4 * ns - 1, 4 * ns, 4 * ns + 1) if b >= 1}
    if ns > SMALL_BLOCKS:
        return sorted({WAVES_PER_BLOCK * b for b in blocks if b < SMALL_BLOCKS} | set(TINY_BATCHES))
    return sorted(WAVES_PER_BLOCK * b for b in blocks)


WIDTH_KEYS = [(D, B) for D in WIDTH_CASES for B in width_batch_sizes(D)]


def draw_weights(rng, U, I, D):
    return {UM: rng.standard_normal((U, D)).astype(np.float32), IM: rng.standard_normal((I, D)).astype(np.float32),
            V: (rng.standard_normal((1, D)) / np.sqrt(D)).astype(np.float32)}


def pre_activations(w, batch):
    """(v . (u * i+), v . (u * i-)) of the fp64 evaluation, before the ReLU."""
    with float64_oracle(pn):
        w64 = to64(w)
        return pn.pgmf_scores(w64, batch[0], batch[1])[1], pn.pgmf_scores(w64, batch[0], batch[2])[1]


def kinds(w, batch):
    """Per triple: "open" (both ReLUs), "pos_only", "neg_only", "closed" (both; the kernel's second ``continue``)."""
    pp, pq = pre_activations(w, batch)
    return np.where(pp > 0, np.where(pq > 0, "open", "pos_only"), np.where(pq > 0, "neg_only", "closed"))


def candidate_triples(rng, w, n, U, I):
    """n random triples with pos != neg and no pre-activation within GATE_MARGIN of zero."""
    out = [np.zeros(0, dtype=np.int64)] * 3
    while len(out[0]) < n:
        u, p = rng.integers(0, U, 2 * n + 16), rng.integers(0, I, 2 * n + 16)
        q = (p + 1 + rng.integers(0, I - 1, len(p))) % I
        pp, pq = pre_activations(w, (u, p, q))
        keep = (np.abs(pp) >= GATE_MARGIN) & (np.abs(pq) >= GATE_MARGIN)
        out = [np.concatenate([a, b[keep]]) for a, b in zip(out, (u, p, q))]
    return tuple(a[:n].astype(np.int64) for a in out)


@functools.lru_cache(maxsize=None)
def width_weights(D):
    return draw_weights(np.random.default_rng(7100 + D), USERS, ITEMS, D)


def width_fixture(D, B):
    """B random triples on the width's tables; where the first three triples of a block of four (or all before the
    batch's last) have both ReLUs closed, the next candidate with an open one takes the fourth place: every block then
    writes a partial of grad v that is not all zeros."""
    w = width_weights(D)
    rng = np.random.default_rng([7100 + D, B])
    pool = candidate_triples(rng, w, 3 * B + 16, USERS - SPARE, ITEMS - SPARE)
    closed = kinds(w, pool) == "closed"
    take, i = [], 0
    for t in range(B):
        first = t - t % WAVES_PER_BLOCK
        if (t % WAVES_PER_BLOCK == WAVES_PER_BLOCK - 1 or t == B - 1) and all(closed[j] for j in take[first:]):
            while closed[i]:
                i += 1
        take.append(i)
        i += 1
    return Case((D, B), D, w, tuple(a[take] for a in pool), LAM, CLIP)


def stride_fixture():
    """TRIP + 6 triples: waves 0 .. 5 of the grid run a second triple with gv and the loss of the first in their
    registers.  A random batch, permuted so that (triple w, triple TRIP + w) have the kinds of STRIDE_PAIRS."""
    D, B = STRIDE_D, STRIDE_B
    U, I = STRIDE_TABLES
    rng = np.random.default_rng(4102)
    w = draw_weights(rng, U, I, D)
    u, p, q = candidate_triples(rng, w, B, U - SPARE, I - SPARE)
    kind = kinds(w, (u, p, q))
    free = list(range(2 * len(STRIDE_PAIRS), TRIP)) + list(range(TRIP + len(STRIDE_PAIRS), B))
    order = np.arange(B)
    for wv, pair in enumerate(STRIDE_PAIRS):
        for slot, want in zip((wv, TRIP + wv), pair):
            want = "open" if want == "same_item" else want
            src = next(j for j in free if kind[order[j]] == want)
            free.remove(src)
            order[slot], order[src] = order[src], order[slot]
    u, p, q = u[order], p[order], q[order]
    wv = [pair[0] for pair in STRIDE_PAIRS].index("same_item")
    q[wv] = p[wv]
    return Case(STRIDE_CASE, D, w, (u, p, q), LAM, CLIP)


def closed_fixture():
    """37 triples, both ReLUs closed on every one: the kernel's second ``continue`` on every trip of every wave."""
    D, B = 65, 37
    rng = np.random.default_rng(3700)
    w = draw_weights(rng, USERS, ITEMS, D)
    pool = candidate_triples(rng, w, 16 * B, USERS - SPARE, ITEMS - SPARE)
    sel = np.nonzero(kinds(w, pool) == "closed")[0][:B]
    return Case(CLOSED_CASE, D, w, tuple(a[sel] for a in pool), LAM, CLIP)


def saturated_fixture(x=None):
    """12 triples and the same 12 with positive and negative swapped; v scaled so that max |s+ - s-| is SATURATED_X."""
    D, B = SATURATED_D, 12
    rng = np.random.default_rng(3200)
    w = draw_weights(rng, USERS, ITEMS, D)
    u, p, q = candidate_triples(rng, w, B, USERS - SPARE, ITEMS - SPARE)
    batch = (np.concatenate([u, u]), np.concatenate([p, q]), np.concatenate([q, p]))
    grow = (SATURATED_X if x is None else x) / float(np.abs(score_differences(w, batch)).max())
    w[V] = (w[V].astype(np.float64) * grow).astype(np.float32)
    return Case(SATURATED_CASE, D, w, batch, LAM, NO_CLIP)


def score_differences(w, batch):
    pp, pq = pre_activations(w, batch)
    return np.maximum(pp, 0.0) - np.maximum(pq, 0.0)


def collision_fixture(key):
    """D = 65.  ``pos_is_neg``: every second triple has its positive item as its negative one (x = 0; the two item
    atomics land on one row with opposite signs); ``one_user``: one user row takes all 37 triples; ``hot``: one open
    (u, p, n) 64 times, so that three rows take 64 atomics per column each."""
    D = 65
    rng = np.random.default_rng(6500 + NAMED_CASES.index(key))
    w = draw_weights(rng, USERS, ITEMS, D)
    u, p, q = candidate_triples(rng, w, 37, USERS - SPARE, ITEMS - SPARE)
    if key == SAME_ITEM_CASE:
        q[::2] = p[::2]
    elif key == ONE_USER_CASE:
        pool = candidate_triples(rng, w, 4000, USERS - SPARE, ITEMS - SPARE)
        mine = np.nonzero(pool[0] == u[0])[0][:37]
        u, p, q = pool[0][mine], pool[1][mine], pool[2][mine]
    else:
        first = int(np.nonzero(kinds(w, (u, p, q)) == "open")[0][0])
        u, p, q = (np.full(64, a[first]) for a in (u, p, q))
    return Case(key, D, w, (u, p, q), LAM, CLIP)


@functools.lru_cache(maxsize=None)
def fixture(key):
    """The Case of a ``(D, B)`` of WIDTH_KEYS or of one of NAMED_CASES; computed once, never written to."""
    if isinstance(key, tuple):
        return width_fixture(*key)
    if key in (SAME_ITEM_CASE, ONE_USER_CASE, HOT_CASE):
        return collision_fixture(key)
    return {STRIDE_CASE: stride_fixture, CLOSED_CASE: closed_fixture, SATURATED_CASE: saturated_fixture}[key]()


def exact(c, batch=None, lam=None):
    """(loss, unclipped gradients, norm, clip coefficient) of the restatement evaluated in fp64."""
    with float64_oracle(pn):
        loss, g = pn.pgmf_grads(to64(c.w), *(c.batch if batch is None else batch), c.lam if lam is None else lam)
    total = float(np.sqrt(sum((v ** 2).sum() for v in g.values())))
    return loss, g, total, min(1.0, c.clip / (total + 1e-6))


def reference_of(c):
    loss64, g64, total64, coef64 = exact(c)
    loss32, g32 = pn.pgmf_grads(c.w, *c.batch, c.lam)
    clipped = {k: v.copy() for k, v in g32.items()}
    total32 = pn.clip_grad_norm(clipped, c.clip)
    return Ref(loss64, g64, total64, coef64, loss32, g32, total32, clipped)


@functools.lru_cache(maxsize=None)
def reference(key):
    """The fp64 evaluation and the fp32 restatement of ``fixture(key)``, before and after the clip."""
    return reference_of(fixture(key))


def tolerances(g32, g64):
    """Per tensor what ``helpers.assert_grads_as_accurate`` allows."""
    return {k: REL * float(np.abs(g64[k]).max()) + 2.0 * float(np.abs(g32[k] - g64[k]).max()) for k in g64}


def terms(c, idx):
    """What the triples ``idx`` add to the fp64 loss and (unclipped) gradient of the whole batch."""
    idx = np.atleast_1d(idx)
    loss, g, _, _ = exact(c, tuple(a[idx] for a in c.batch), lam=0.0)
    share = len(idx) / len(c.batch[0])
    return loss * share, {k: v * share for k, v in g.items()}


def removal_margins(key, idx):
    """The batch without the triples ``idx``: ``(largest move of a gradient tensor, move of grad v, move of the loss)``,
    each in units of the tolerance the GPU test applies to it."""
    r = reference(key)
    tol = tolerances(r.g32, r.g64)
    loss, g = terms(fixture(key), idx)
    moved = {k: float(np.abs(g[k]).max()) / tol[k] if tol[k] > 0 else 0.0 for k in KEYS}
    return max(moved.values()), moved[V], abs(loss) / (REL * abs(r.loss64) + 1e-12)


def column_margin(key, t, col):
    """Triple ``t`` with column ``col`` of its three row updates and of its share of grad v lost: per tensor the move
    in units of its tolerance."""
    r = reference(key)
    tol = tolerances(r.g32, r.g64)
    _, g = terms(fixture(key), t)
    return {k: float(np.abs(g[k][:, col]).max()) / tol[k] for k in KEYS}
