"""Fixtures of the Triple2vec edge tests, shared by tests/test_t2v_edges_host.py (which shows on the CPU that the inputs
can see one lost unit and one lost column, and that the fp32 restatement is a fair yardstick on them) and
tests/test_t2v_edges_gpu.py (which runs csrc/triple2vec.hip on those very inputs).  No tests here.

``t2v_grad_kernel`` runs one wave per unit -- unit 0 of a triple carries its three positive terms, unit 1 + j its negative
j -- on a grid capped at 2048 blocks of 4 waves, lays a row out as columns ``lane + 64 k``, k < 4, guarded by ``c < D``,
and scatters every share with float atomics.  ``WIDTH_CASES`` holds the widths with one live column in an upper slot,
one short of a full slot and below 8, each with unit counts that leave waves of a block idle, with ``n_neg == 0`` and
with shared and independent item tables; the other cases reach the second trip of the grid-stride loop with a triple
astride the boundary, saturated logits, and every address collision the atomics must absorb.

The rows are N(0, s^2) with s^4 = 1 / (2 D), so that a positive logit e_u . (e_1 + e_2) has unit variance, and the
biases N(0, 0.3^2).  ``batch_size`` of the config is larger than every batch: the loss is divided by 3 x the configured
size (triple2vec.py:92), whatever the batch's length."""
import collections
import functools

import numpy as np

from helpers import REL, float64_oracle, to64
from oracle import triple2vec_numpy as tn
from test_oracle_golden_t2v import bias_floor

KEYS = tn.KEYS
UE, E1, E2, UB, IB = KEYS
ROW_KEYS = (UE, E1, E2)
WAVE, WAVES_PER_BLOCK, MAX_BLOCKS, MAX_NPL = 64, 4, 2048, 4      # kWave, kWavesPerBlock, kT2vMaxBlocks, kT2vMaxNpl
TRIP = MAX_BLOCKS * WAVES_PER_BLOCK                    # units per trip of the grid-stride loop

WIDTH_CASES = (1, 3, 63, 65, 129, 193, 255)
COVERED_ELSEWHERE = (8, 16, 64, 100, 128, 256)         # the widths of the goldens and of tests/test_t2v_gpu.py
LIVE = {1: [1, 0, 0, 0], 3: [3, 0, 0, 0], 63: [63, 0, 0, 0], 65: [64, 1, 0, 0], 129: [64, 64, 1, 0],
        193: [64, 64, 64, 1], 255: [64, 64, 64, 63]}
# (shared item tables, B, n_neg) of every width: 1, 3, 4 and 5 units (one and two blocks with idle waves), 5 units
# without negatives, and 28 units with either kind of tables.  n_neg == 0 needs independent tables: ``use_bias = n_neg``
# is what aliases item_emb2 (triple2vec.py:19, 38-39).
WIDTH_SHAPES = ((False, 1, 0), (True, 1, 2), (False, 2, 1), (True, 1, 4), (False, 5, 0), (True, 7, 3), (False, 7, 3))
WIDTH_KEYS = [(D,) + s for D in WIDTH_CASES for s in WIDTH_SHAPES]
BATCH_SIZE = 16            # the config's; the width cases' batches have 1 .. 7 triples
USERS, ITEMS, SPARE = 24, 20, 4                        # the last SPARE rows of every table are in no batch

STRIDE_CASE, SATURATED_CASE = "stride", "saturated"
COLLISION_CASES = (("collisions", True), ("collisions", False), ("hot", True), ("hot", False))
NAMED_CASES = (STRIDE_CASE, SATURATED_CASE) + COLLISION_CASES
STRIDE_D, STRIDE_B, STRIDE_NEG, STRIDE_TABLES, STRIDE_BATCH_SIZE = 65, 2732, 2, (1500, 1200), 4096
# The saturated case: every row scaled by one factor until positive and negative logits both reach SATURATED_X with
# both signs in fp64 (the smallest of the four extremes is SATURATED_X).  logsigmoid is linear or ~0 there and its
# derivative 1 or ~1e-14; the fp32 restatement holds REL at every magnitude of SATURATED_SCAN
# (test_saturation_threshold_the_restatement_holds), so the magnitude was not lowered.
SATURATED_X = 32.0
SATURATED_SCAN = (30.5, 32.0, 40.0, 60.0, 80.0)

Case = collections.namedtuple("Case", "key D w batch batch_size shared")
Ref = collections.namedtuple("Ref", "loss64 g64 loss32 g32")


def live_columns(D):
    return [sum(lane + WAVE * k < D for lane in range(WAVE)) for k in range(MAX_NPL)]


def n_units(c):
    B, n_neg = c.batch[3].shape
    return B * (1 + n_neg)


def unit_of(q, n_neg):
    """(triple, j) of unit q as the kernel splits it: j = -1 the positive group, j >= 0 negative j."""
    return q // (1 + n_neg), q % (1 + n_neg) - 1


def draw_weights(rng, U, I, D, shared):
    s = (1.0 / (2 * D)) ** 0.25
    w = {k: (rng.standard_normal((n, D)) * s).astype(np.float32) for k, n in ((UE, U), (E1, I), (E2, I))}
    w[UB] = rng.normal(0, 0.3, (U, 1)).astype(np.float32)
    w[IB] = rng.normal(0, 0.3, (I, 1)).astype(np.float32)
    if shared:                                         # what the state_dict shows once item_emb2 IS item_emb1
        w[E2] = w[E1].copy()
    return w


def draw_batch(rng, B, n_neg, U, I):
    ids = lambda hi, shape: rng.integers(0, hi, shape).astype(np.int64)  # noqa: E731
    return (ids(U, B), ids(I, B), ids(I, B), ids(U, (B, n_neg)), ids(I, (B, n_neg)), ids(I, (B, n_neg)))


@functools.lru_cache(maxsize=None)
def width_weights(D, shared):
    return draw_weights(np.random.default_rng([7200 + D, shared]), USERS, ITEMS, D, shared)


def width_fixture(D, shared, B, n_neg):
    rng = np.random.default_rng([7200 + D, shared, B, n_neg])
    pu, p1, p2, nu, n1, n2 = draw_batch(rng, B, n_neg, USERS - SPARE, ITEMS - SPARE)
    p2 = np.where(p2 == p1, (p2 + 1) % (ITEMS - SPARE), p2)        # collisions belong to the collision cases: a row
    nu = np.where(nu == pu[:, None], (nu + 1) % (USERS - SPARE), nu)    # against itself is a logit of sqrt(D / 2)
    for _ in range(2):
        n2 = np.where((n2 == p1[:, None]) | (n2 == p2[:, None]), (n2 + 1) % (ITEMS - SPARE), n2)
    return Case((D, shared, B, n_neg), D, width_weights(D, shared), (pu, p1, p2, nu, n1, n2), BATCH_SIZE, shared)


def stride_fixture():
    """2732 triples with 2 negatives: 8196 units on a grid of 2048 blocks, 8192 to a trip.  Triple 2730 has its
    positive group and negative 0 in the first trip and negative 1 in the second; triple 2731 lies in the second."""
    U, I = STRIDE_TABLES
    rng = np.random.default_rng(8196)
    w = draw_weights(rng, U, I, STRIDE_D, True)
    return Case(STRIDE_CASE, STRIDE_D, w, draw_batch(rng, STRIDE_B, STRIDE_NEG, U - SPARE, I - SPARE),
                STRIDE_BATCH_SIZE, True)


def logits(c):
    """(positive [B, 3], negative [B, n_neg, 3]) logits of the fp64 evaluation."""
    w = to64(c.w)
    pu, p1, p2, nu, n1, n2 = c.batch
    U, A = w[UE], w[E1]
    Bt = A if c.shared else w[E2]
    bu, bi = w[UB][:, 0], w[IB][:, 0]
    eu, e1, e2 = U[pu], A[p1], Bt[p2]
    pos = np.stack([(eu * (e1 + e2)).sum(1) + bu[pu], (e1 * (eu + e2)).sum(1) + bi[p1],
                    (e2 * (eu + e1)).sum(1) + bi[p2]], axis=1)
    neg = np.stack([np.einsum("bnd,bd->bn", U[nu], eu) + bu[nu], np.einsum("bnd,bd->bn", A[n2], e1) + bi[n1],
                    np.einsum("bnd,bd->bn", Bt[n2], e2) + bi[n2]], axis=2)
    return pos, neg


def saturated_fixture(x=None):
    """D = 65, 6 triples with 3 negatives, independent tables: every row scaled until the smallest of the four extremes
    (largest and smallest positive logit, largest and smallest negative logit) is SATURATED_X."""
    rng = np.random.default_rng(3265)
    w = draw_weights(rng, USERS, ITEMS, 65, False)
    batch = draw_batch(rng, 6, 3, USERS - SPARE, ITEMS - SPARE)
    target = SATURATED_X if x is None else x
    for _ in range(8):                               # the biases do not scale: a few rounds settle the factor
        pos, neg = logits(Case(None, 65, w, batch, BATCH_SIZE, False))
        reach = min(pos.max(), -pos.min(), neg.max(), -neg.min())
        assert reach > 0
        for k in ROW_KEYS:
            w[k] = (w[k].astype(np.float64) * (target / reach) ** 0.5).astype(np.float32)
    return Case(SATURATED_CASE, 65, w, batch, BATCH_SIZE, False)


def collision_fixture(kind, shared):
    """D = 65, 3 negatives.  ``collisions``: triple 0 has i1 == i2 (with shared tables ONE row written through item_emb1
    and item_emb2), triple 1 u' == u, triple 2 a negative i2' that is its i1, triple 3 one that is its i2, triple 4 the
    same negative twice, triple 5 all of these at once; triples 6 and 7 are ordinary.  ``hot``: 64 identical triples
    whose negatives all name one user row and one item row."""
    rng = np.random.default_rng([6500, shared])
    w = draw_weights(rng, USERS, ITEMS, 65, shared)
    if kind == "hot":
        one = draw_batch(rng, 1, 1, USERS - SPARE, ITEMS - SPARE)
        batch = tuple(np.repeat(a[:1], 64, axis=0) if a.ndim == 1 else np.tile(a[:1], (64, 3)) for a in one)
        return Case((kind, shared), 65, w, batch, 128, shared)
    pu, p1, p2, nu, n1, n2 = draw_batch(rng, 8, 3, USERS - SPARE, ITEMS - SPARE)
    p2 = np.where(p2 == p1, (p2 + 1) % (ITEMS - SPARE), p2)
    p2[[0, 5]] = p1[[0, 5]]
    nu[[1, 5], 0] = pu[[1, 5]]
    n2[[2, 5], 0] = p1[[2, 5]]
    n2[[3, 5], 1] = p2[[3, 5]]
    for a in (nu, n1, n2):
        a[[4, 5], 2] = a[[4, 5], 0]
    return Case((kind, shared), 65, w, (pu, p1, p2, nu, n1, n2), BATCH_SIZE, shared)


@functools.lru_cache(maxsize=None)
def fixture(key):
    """The Case of a ``(D, shared, B, n_neg)`` of WIDTH_KEYS or of one of NAMED_CASES; computed once, never written
    to."""
    if key == STRIDE_CASE:
        return stride_fixture()
    if key == SATURATED_CASE:
        return saturated_fixture()
    if len(key) == 2:
        return collision_fixture(*key)
    return width_fixture(*key)


def exact(c, batch=None):
    """(loss, gradients) of the restatement evaluated in fp64."""
    with float64_oracle(tn):
        return tn.t2v_grads(to64(c.w), c.batch if batch is None else batch, c.batch_size, c.shared, acc=np.float64)


def reference_of(c):
    loss64, g64 = exact(c)
    loss32, g32 = tn.t2v_grads(c.w, c.batch, c.batch_size, c.shared)
    return Ref(loss64, g64, loss32, g32)


@functools.lru_cache(maxsize=None)
def reference(key):
    """The fp64 evaluation and the fp32 restatement of ``fixture(key)``."""
    return reference_of(fixture(key))


def floor_fn(c):
    """``floor_fn`` of ``assert_grads_as_accurate``: a bias gradient sums terms of size <= 1 / (3 batch_size)."""
    return lambda k: bias_floor(k, 1.0 / (3 * c.batch_size))


def tolerances(c, g32, g64):
    """Per tensor what ``helpers.assert_grads_as_accurate`` allows with ``floor_fn(c)``."""
    floor = floor_fn(c)
    return {k: REL * max(float(np.abs(g64[k]).max()), floor(k)) + 2.0 * float(np.abs(g32[k] - g64[k]).max())
            for k in g64}


def predict64(c, users, items):
    with float64_oracle(tn):
        return tn.t2v_predict(to64(c.w), users, items, c.shared)


def unit_terms(c, t, j):
    """What unit (t, j) adds to the fp64 loss and gradient of the batch: the three positive terms of triple t (j = -1)
    or the three terms of its negative j."""
    alone = tuple(a[t:t + 1] for a in c.batch[:3])
    none = tuple(a[t:t + 1, :0] for a in c.batch[3:])
    loss0, g0 = exact(c, alone + none)
    if j < 0:
        return loss0, g0
    loss1, g1 = exact(c, alone + tuple(a[t:t + 1, j:j + 1] for a in c.batch[3:]))
    return loss1 - loss0, {k: g1[k] - g0[k] for k in KEYS}


def unit_margins(key, t, j):
    """The batch without unit (t, j): ``(largest move of a gradient tensor, move of the loss, per row tensor the move
    its last live column alone makes)``, each in units of the tolerance the GPU test applies."""
    c, r = fixture(key), reference(key)
    tol = tolerances(c, r.g32, r.g64)
    loss, g = unit_terms(c, t, j)
    rows = [k for k in ROW_KEYS if not (c.shared and k == E2)]
    return (max(float(np.abs(g[k]).max()) / tol[k] for k in KEYS if g[k].any() or tol[k] > 0),
            abs(loss) / (REL * abs(r.loss64) + 1e-12),
            {k: float(np.abs(g[k][:, c.D - 1]).max()) / tol[k] for k in rows})
