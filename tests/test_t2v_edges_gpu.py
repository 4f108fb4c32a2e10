"""GPU parity tests of Triple2vec (csrc/triple2vec.hip) where the goldens and tests/test_t2v_gpu.py do not reach: widths
with one live column in an upper slot, one short of a full slot and below 8, unit counts that leave waves of a block
idle, ``n_neg == 0``, a triple astride the trip boundary of the grid-stride loop, saturated logits, every address
collision the atomics must absorb, and ``predict`` at those widths and past one trip.  The inputs are
tests/t2v_edges.py's, which tests/test_t2v_edges_host.py shows to see one lost unit or column; the yardstick is the fp64
restatement under ``assert_scalar_close``, ``assert_grads_as_accurate`` with ``bias_floor`` and ``assert_tensor_close``."""
import numpy as np
import pytest

import t2v_edges as te
from helpers import assert_grads_as_accurate, assert_scalar_close, assert_sgd_exact, assert_tensor_close
from oracle import triple2vec_numpy as tn
from test_t2v_gpu import get_weights, load_weights, make_engine

pytestmark = pytest.mark.gpu
KEYS = te.KEYS
WORST = {"ratio": 0.0, "where": ""}


def sgd_lr(c):
    """Every share of the gradient carries 1 / (3 batch_size): with lr = batch_size a step moves a weight by ~0.1."""
    return float(c.batch_size)


def engine_of(c, optimizer="sgd", lr=None):
    """``n_neg`` of the config decides the aliasing alone (``use_bias = n_neg``); the batches bring their own count."""
    U, I = c.w[te.UE].shape[0], c.w[te.E1].shape[0]
    eng = make_engine(U, I, c.D, c.batch_size, 3 if c.shared else 0, optimizer, sgd_lr(c) if lr is None else lr)
    eng.model._alias()
    assert eng.model.shared_items == c.shared
    load_weights(eng, c.w)
    return eng


def written_rows(c):
    """Per tensor the rows some term of the batch adds to."""
    pu, p1, p2, nu, n1, n2 = (a.ravel() for a in c.batch)
    users, items = np.concatenate([pu, nu]), np.concatenate([p1, p2, n1, n2])
    if c.shared:
        return {te.UE: users, te.E1: np.concatenate([p1, p2, n2]), te.E2: np.zeros(0, dtype=np.int64), te.UB: users,
                te.IB: items}
    return {te.UE: users, te.E1: np.concatenate([p1, n2]), te.E2: np.concatenate([p2, n2]), te.UB: users, te.IB: items}


def check_backward(eng, key, what):
    """Loss and every gradient of one ``backward_only`` against ``te.reference(key)``; rows no term names are exactly
    0.0 -- with shared tables the whole slot of item_emb2 -- and the gradient buffer is left cleared.  Returns the
    gradients as numpy arrays."""
    c, r = te.fixture(key), te.reference(key)
    loss, grads = eng.backward_only(c.batch)
    grads = {k: grads[k].cpu().numpy().reshape(r.g64[k].shape) for k in KEYS}
    tol = te.tolerances(c, r.g32, r.g64)
    print(f"{what}: loss {loss!r} vs exact {r.loss64!r}")
    for k in KEYS:
        err = float(np.abs(grads[k] - r.g64[k]).max())
        ratio = err / tol[k] if tol[k] > 0 else 0.0
        if ratio > WORST["ratio"]:
            WORST.update(ratio=ratio, where=f"{what} {k}")
        print(f"  grad {k}: err vs exact {err:.3e}, fp32 restatement's {np.abs(r.g32[k] - r.g64[k]).max():.3e}, "
              f"bound {tol[k]:.3e}, err / bound {ratio:.3f}")
    print(f"  worst err / bound so far: {WORST['ratio']:.3f} ({WORST['where']})")
    assert_scalar_close(loss, r.loss64, what=f"{what}: loss")
    assert_grads_as_accurate(grads, r.g32, r.g64, what=f"{what}: grad", floor_fn=te.floor_fn(c))
    assert float(eng._g_flat.abs().max()) == 0.0, "the gradient buffer is left cleared"
    for k, rows in written_rows(c).items():
        idle = np.setdiff1d(np.arange(c.w[k].shape[0]), rows)
        assert len(idle) >= te.SPARE, "the fixture has no untouched row"
        assert float(np.abs(grads[k][idle]).max()) == 0.0, f"{what}: rows of {k} no term names"
    return grads


def check_sgd_step(eng, key, what):
    """One ``train_single_batch`` from the fixture's weights against the fp32 restatement's step."""
    c, r = te.fixture(key), te.reference(key)
    load_weights(eng, c.w)
    loss = eng.train_single_batch(c.batch)
    assert_scalar_close(loss, r.loss64, what=f"{what}: loss of the step")
    w_ref = {k: v.copy() for k, v in c.w.items()}
    tn.t2v_train_step(w_ref, tn.new_opt_state(w_ref, "sgd"), c.batch, c.batch_size, "sgd", sgd_lr(c), c.shared)
    assert float(np.abs(w_ref[te.UE] - c.w[te.UE]).max()) > 1e-3, "the step moves nothing"
    got = get_weights(eng)
    assert_sgd_exact(got, w_ref, c.w, f"{what}: SGD step")
    if c.shared:
        assert np.array_equal(got[te.E2], got[te.E1])
    assert float(eng._g_flat.abs().max()) == 0.0
    load_weights(eng, c.w)


@pytest.mark.parametrize("D", te.WIDTH_CASES)
def test_every_width_and_unit_count(hip_device, D):
    """D = 1 and 3: one slot, 63 and 61 idle lanes of it; 63: one short of a slot; 65, 129, 193: one live column in slot
    1, 2, 3; 255: one short of four slots.  1, 3, 4 and 5 units (idle waves in the only or in the second block), 5
    units with ``n_neg == 0`` (null negative arrays, one unit per triple) and 28 units, on shared and on independent
    item tables."""
    engines = {}
    for key in te.WIDTH_KEYS:
        if key[0] != D:
            continue
        c = te.fixture(key)
        if c.shared not in engines:
            engines[c.shared] = engine_of(c)
        eng = engines[c.shared]
        check_backward(eng, key, f"{key}")
        check_sgd_step(eng, key, f"{key}")


def test_triple_astride_the_trip_boundary(hip_device):
    """8196 units on the grid of 2048 blocks: triple 2730 has its last negative in the second trip, triple 2731 all
    three units; a second run is held to the same bound and the two agree within it (float atomics: no bit equality is
    asked)."""
    key = te.STRIDE_CASE
    c, r = te.fixture(key), te.reference(key)
    assert te.n_units(c) > te.TRIP
    eng = engine_of(c)
    first = check_backward(eng, key, "stride")
    again = check_backward(eng, key, "stride again")
    tol = te.tolerances(c, r.g32, r.g64)
    for k in KEYS:
        apart = float(np.abs(first[k] - again[k]).max())
        assert apart <= tol[k], f"stride: two runs differ in {k} by {apart:.3e} > {tol[k]:.3e}"
    check_sgd_step(eng, key, "stride")


def test_saturated_logits(hip_device):
    """Positive and negative logits beyond +-30 with both signs: logsigmoid where it is linear and where it is 1e-14,
    and its derivative.  Then one Adam step: the weights stay finite and move; and one SGD step."""
    key = te.SATURATED_CASE
    c = te.fixture(key)
    eng = engine_of(c, "adam", 1e-3)
    grads = check_backward(eng, key, "saturated")
    assert all(np.isfinite(v).all() for v in grads.values())
    eng.load_optimizer_state(0)
    loss = eng.train_single_batch(c.batch)
    assert_scalar_close(loss, te.reference(key).loss64, what="saturated: loss of the step")
    w1 = get_weights(eng)
    assert all(np.isfinite(v).all() for v in w1.values())
    assert any(not np.array_equal(w1[k], c.w[k]) for k in KEYS), "the step moved nothing"
    check_sgd_step(engine_of(c), key, "saturated")


@pytest.mark.parametrize("kind,shared", te.COLLISION_CASES)
def test_colliding_addresses(hip_device, kind, shared):
    """``collisions``: i1 == i2 (with shared tables one row written through item_emb1 and item_emb2), u' == u, a
    negative i2' equal to i1 or to i2, one negative twice in a triple, and all of them in one triple; ``hot``: 64
    identical triples whose negatives name one row.  The atomics add every share."""
    key = (kind, shared)
    eng = engine_of(te.fixture(key))
    check_backward(eng, key, f"{kind} shared {shared}")
    check_sgd_step(eng, key, f"{kind} shared {shared}")


def check_predict(eng, c, n, seed, what):
    rng = np.random.default_rng(seed)
    users = rng.integers(0, c.w[te.UE].shape[0], n)
    items = rng.integers(0, c.w[te.E1].shape[0], n)
    scores = eng.model.predict(users, items)
    assert tuple(scores.shape) == (n,)
    assert_tensor_close(scores.cpu().numpy(), te.predict64(c, users, items), what=what)


@pytest.mark.parametrize("D", te.WIDTH_CASES)
def test_predict_at_every_width(hip_device, D):
    """``t2v_predict_kernel`` against the fp64 predict, shared and independent: 37 pairs at every width, and
    8192 + 3 pairs at D = 65, three of them in the second trip of its grid-stride loop."""
    for shared in (True, False):
        c = te.fixture((D, shared, 7, 3))
        eng = engine_of(c)
        check_predict(eng, c, 37, D, f"predict D {D} shared {shared}")
        if D == 65:
            check_predict(eng, c, te.TRIP + 3, D + 1, f"predict D {D} shared {shared}, two trips")


@pytest.mark.parametrize("shared", [True, False])
def test_clean_state_after_an_error(hip_device, shared):
    """A batch with a positive id out of range, then one with a negative id out of range: IndexError each time, the
    weights as they were, and the next ``backward_only`` meets its bound -- nothing left in the gradient buffer or in
    the scratch partials."""
    key = (65, shared, 7, 3)
    c = te.fixture(key)
    eng = engine_of(c)
    check_backward(eng, key, "before the errors")
    for n, (slot, where, bad) in enumerate(((1, 3, te.ITEMS), (0, 6, -1), (3, (2, 1), te.USERS), (5, (6, 2), te.ITEMS),
                                            (4, (0, 0), -2))):
        batch = [a.copy() for a in c.batch]
        batch[slot][where] = bad
        with pytest.raises(IndexError):
            eng.backward_only(tuple(batch))
        check_backward(eng, key, f"after error {n}")
    assert all(np.array_equal(v, c.w[k]) for k, v in get_weights(eng).items()), "the weights moved"
    check_sgd_step(eng, key, "after the errors")
