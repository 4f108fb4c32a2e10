"""GPU parity tests of PairwiseGMF (csrc/pgmf.hip) where the goldens and tests/test_pgmf_gpu.py do not reach: widths with
one live column in an upper slot, one short of a full slot and below 8, block counts at the seams of the finish kernel's
unrolled fold, the second trip of the grid-stride loop with every pair of triple kinds on one wave, both ReLUs closed on
every triple, a saturated BPR term, and rows every triple collides on.  The inputs are tests/pgmf_edges.py's, which
tests/test_pgmf_edges_host.py shows to see one lost triple, block or column; the yardstick is the fp64 restatement under
``assert_scalar_close`` and ``assert_grads_as_accurate``, with the clip off and on."""
import numpy as np
import pytest

import pgmf_edges as pe
from helpers import assert_grads_as_accurate, assert_scalar_close, assert_sgd_exact
from oracle import pgmf_numpy as pn
from test_pgmf_gpu import get_weights, load_weights, make_engine, np_grads

pytestmark = pytest.mark.gpu
KEYS = pe.KEYS
SGD_LR = 100.0             # the clipped gradient has norm 0.01: the step then moves a weight by up to ~0.1
WORST = {"ratio": 0.0, "where": ""}


def engine_of(c, optimizer="sgd", lr=SGD_LR):
    U, I = c.w[pe.UM].shape[0], c.w[pe.IM].shape[0]
    eng = make_engine(U, I, c.D, len(c.batch[0]), optimizer, lr, c.lam, c.clip)
    load_weights(eng, c.w)
    return eng


def check_backward(eng, key, what, clip):
    """Loss, pre-clip norm and every gradient of one ``backward_only`` against ``pe.reference(key)``: with the clip on,
    the clipped gradient against the fp64 gradient times the fp64 coefficient.  Rows no triple names are exactly 0.0
    and the gradient buffer is left cleared.  Returns the gradients as numpy arrays."""
    c, r = pe.fixture(key), pe.reference(key)
    loss, grads, total = eng.backward_only(c.batch, clip=clip)
    grads = {k: v.reshape(r.g64[k].shape) for k, v in np_grads(grads).items()}
    exact = {k: v * r.coef64 for k, v in r.g64.items()} if clip else r.g64
    ref32 = r.g32_clipped if clip else r.g32
    tol = pe.tolerances(ref32, exact)
    print(f"{what} clip {clip}: loss {loss!r} vs exact {r.loss64!r}, norm {total!r} vs {r.total64!r}")
    for k in KEYS:
        err = float(np.abs(grads[k] - exact[k]).max())
        ratio = err / tol[k] if tol[k] > 0 else 0.0
        if ratio > WORST["ratio"]:
            WORST.update(ratio=ratio, where=f"{what} clip {clip} {k}")
        print(f"  grad {k}: err vs exact {err:.3e}, fp32 restatement's {np.abs(ref32[k] - exact[k]).max():.3e}, "
              f"bound {tol[k]:.3e}, err / bound {ratio:.3f}")
    print(f"  worst err / bound so far: {WORST['ratio']:.3f} ({WORST['where']})")
    assert_scalar_close(loss, r.loss64, what=f"{what}: loss")
    if clip:
        assert_scalar_close(total, r.total64, what=f"{what}: total norm")
    else:
        assert total is None
    assert_grads_as_accurate(grads, ref32, exact, what=f"{what}: grad")
    assert float(eng._g_flat.abs().max()) == 0.0, "the gradient buffer is left cleared"
    u, p, q = c.batch
    no_user = np.setdiff1d(np.arange(c.w[pe.UM].shape[0]), u)
    no_item = np.setdiff1d(np.arange(c.w[pe.IM].shape[0]), np.concatenate([p, q]))
    assert len(no_user) >= pe.SPARE and len(no_item) >= pe.SPARE, "the fixture has no untouched row"
    assert float(np.abs(grads[pe.UM][no_user]).max()) == 0.0, f"{what}: user rows no triple names"
    assert float(np.abs(grads[pe.IM][no_item]).max()) == 0.0, f"{what}: item rows no triple names"
    return grads


def check_sgd_step(eng, key, what):
    """One ``train_single_batch`` (clip included) from the fixture's weights against the fp32 restatement's step."""
    c, r = pe.fixture(key), pe.reference(key)
    load_weights(eng, c.w)
    loss = eng.train_single_batch(c.batch)
    assert_scalar_close(loss, r.loss64, what=f"{what}: loss of the step")
    w_ref = {k: v.copy() for k, v in c.w.items()}
    pn.pgmf_train_step(w_ref, pn.new_opt_state(w_ref, "sgd"), c.batch, "sgd", SGD_LR, c.lam, c.clip)
    assert float(np.abs(w_ref[pe.V] - c.w[pe.V]).max()) > 1e-4, "the step moves nothing"
    assert_sgd_exact(get_weights(eng), w_ref, c.w, f"{what}: SGD step")
    assert float(eng._g_flat.abs().max()) == 0.0
    load_weights(eng, c.w)


def check_case(eng, key, what):
    for clip in (False, True):
        grads = check_backward(eng, key, what, clip)
    check_sgd_step(eng, key, what)
    return grads


@pytest.mark.parametrize("D", pe.WIDTH_CASES)
def test_every_width_at_the_finish_kernels_seams(hip_device, D):
    """D = 1 and 3: one slot, 63 and 61 idle lanes of it; 63: one short of a slot; 65, 129, 193: one live column in slot
    1, 2, 3; 255: one short of four slots.  Block counts 1, n_slices - 1 .. + 1 and 4 n_slices - 1 .. + 1 of the width's
    own n_slices (D = 1, 3: B = 1 .. 5, one block with idle waves and two blocks): the unrolled fold of grad v alone,
    with a remainder, and the remainder alone."""
    eng = None
    for B in pe.width_batch_sizes(D):
        c = pe.fixture((D, B))
        eng = eng or engine_of(c)
        check_case(eng, (D, B), f"D {D} B {B}")


def test_second_trip_of_the_grid_stride_loop(hip_device):
    """4096 + 6 triples on the grid of 1024 blocks: waves 0 .. 5 run a second triple behind (open, both closed,
    one-sided, pos == neg) first ones, with grad v and the loss of the first in their registers; a second run is held to
    the same bound and the two agree within it (float atomics: no bit equality is asked)."""
    key = pe.STRIDE_CASE
    c, r = pe.fixture(key), pe.reference(key)
    assert len(c.batch[0]) > pe.TRIP
    eng = engine_of(c)
    first = check_backward(eng, key, "stride", False)
    again = check_backward(eng, key, "stride again", False)
    tol = pe.tolerances(r.g32, r.g64)
    for k in KEYS:
        apart = float(np.abs(first[k] - again[k]).max())
        assert apart <= tol[k], f"stride: two runs differ in {k} by {apart:.3e} > {tol[k]:.3e}"
    check_backward(eng, key, "stride", True)
    check_sgd_step(eng, key, "stride")


def test_both_relus_closed_on_every_triple(hip_device):
    """The second ``continue`` on every trip: the loss is -log(0.5 + 1e-12) + lambda |v|, both tables' gradients are
    exactly 0.0 and grad v is the lambda term alone (every block writes a zero partial)."""
    key = pe.CLOSED_CASE
    c = pe.fixture(key)
    eng = engine_of(c)
    for clip in (False, True):
        grads = check_backward(eng, key, "closed", clip)
        assert not grads[pe.UM].any() and not grads[pe.IM].any()
        assert grads[pe.V].any()
    loss = eng.train_single_batch(c.batch)
    assert_scalar_close(loss, pe.reference(key).loss64, what="closed: loss of the step")
    w1 = get_weights(eng)
    assert np.array_equal(w1[pe.UM], c.w[pe.UM]) and np.array_equal(w1[pe.IM], c.w[pe.IM])
    w_ref = {k: v.copy() for k, v in c.w.items()}
    pn.pgmf_train_step(w_ref, pn.new_opt_state(w_ref, "sgd"), c.batch, "sgd", SGD_LR, c.lam, c.clip)
    assert_sgd_exact(w1, w_ref, c.w, "closed: SGD step")


def test_saturated_bpr_term(hip_device):
    """x = s+ - s- from -32 to +32: -log(sigmoid(x) + 1e-12) and its hand-written derivative where sigmoid(x) is 1e-14
    and where it rounds to 1; the clip off.  Then one Adam step: the weights stay finite and move; and one SGD step."""
    key = pe.SATURATED_CASE
    c = pe.fixture(key)
    eng = engine_of(c, "adam", 1e-3)
    for clip in (False, True):                         # the clip of 1e9 leaves the gradient as it is
        grads = check_backward(eng, key, "saturated", clip)
        assert all(np.isfinite(v).all() for v in grads.values())
    eng.load_optimizer_state(0)
    loss = eng.train_single_batch(c.batch)
    assert_scalar_close(loss, pe.reference(key).loss64, what="saturated: loss of the step")
    w1 = get_weights(eng)
    assert all(np.isfinite(v).all() for v in w1.values())
    assert any(not np.array_equal(w1[k], c.w[k]) for k in KEYS), "the step moved nothing"
    check_sgd_step(engine_of(c), key, "saturated")


@pytest.mark.parametrize("key", [pe.SAME_ITEM_CASE, pe.ONE_USER_CASE, pe.HOT_CASE])
def test_colliding_rows(hip_device, key):
    """pos == neg on every second triple (both item atomics on one row, x = 0), one user in all 37 triples, one
    (u, p, n) 64 times: the atomics add every share."""
    eng = engine_of(pe.fixture(key))
    check_case(eng, key, key)


def test_clean_state_after_an_error(hip_device):
    """A batch with an out-of-range user, then one with an out-of-range positive and one with a negative item, through
    ``backward_only`` (clip off and on): IndexError each time, the weights as they were, and the next ``backward_only``
    meets its bound -- nothing left in the gradient buffer, in the workspace of grad v or in the scratch partials."""
    key = (65, 64)
    c = pe.fixture(key)
    eng = engine_of(c)
    check_backward(eng, key, "before the errors", True)
    u, p, q = (a.copy() for a in c.batch)
    bad_user, bad_item, bad_neg = u.copy(), p.copy(), q.copy()
    bad_user[5], bad_item[17], bad_neg[63] = pe.USERS, pe.ITEMS, -1
    for n, (batch, clip) in enumerate((((bad_user, p, q), False), ((u, bad_item, q), True), ((u, p, bad_neg), True))):
        with pytest.raises(IndexError):
            eng.backward_only(batch, clip=clip)
        check_backward(eng, key, f"after error {n}", clip)
    assert all(np.array_equal(v, c.w[k]) for k, v in get_weights(eng).items()), "the weights moved"
    check_sgd_step(eng, key, "after the errors")
