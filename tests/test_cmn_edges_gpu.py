"""GPU parity tests of CMN (csrc/cmn.hip) where the goldens and tests/test_cmn_gpu.py do not reach: every (lanes per
row, float4 or strided columns) pair of ``cmn_sample_kernel`` with lists at the seams of that width's round, the
block-stride loop (a batch above kCmnMaxBlocks), a softmax whose logits spread over 60 .. 80, a neighbour listed more than
once, a saturated BPR term, and the width limits.  The inputs are tests/cmn_edges.py's, which
tests/test_cmn_edges_host.py shows to see one row lost at a seam; the yardsticks are those of tests/test_cmn_gpu.py: the
fp64 restatement, ``assert_scalar_close``, ``assert_grads_as_accurate`` with ``term_floors`` and ``assert_tensor_close``."""
import numpy as np
import pytest
import torch

import cmn_edges as ce
import cmn_numpy as cn
from helpers import assert_as_accurate_as_reference, assert_grads_as_accurate, assert_scalar_close, assert_sgd_exact
from helpers import assert_tensor_close
from test_cmn_gpu import get_weights, make_engine, np_grads

pytestmark = pytest.mark.gpu
KEYS = ce.KEYS


def engine_of(c, optimizer="sgd", lr=0.01):
    return make_engine(c.w, c.rowptr, c.col, optimizer, lr, 0.9, c.lam, c.clip, len(c.batch[0]))


def check_backward(eng, key, batch, what, clip=True):
    """Loss, pre-clip norm and every gradient of one ``backward_only`` against ``ce.reference(key)``; ``user_output`` is
    not written to and the gradient buffer is left cleared.  Returns the gradients as numpy arrays."""
    c = ce.fixture(key)
    loss64, g64, total64, g32, floors = ce.reference(key)
    loss, grads, total = eng.backward_only(batch) if clip else eng.backward_only(batch, clip=False)
    grads = np_grads(grads)
    print(f"{what}: loss {loss!r} vs exact {loss64!r}, norm {total!r} vs {total64!r}")
    for k in KEYS:
        print(f"  grad {k}: err vs exact {np.abs(grads[k].reshape(g64[k].shape) - g64[k]).max():.3e}, fp32 restatement's "
              f"{np.abs(g32[k] - g64[k]).max():.3e}, scale {max(np.abs(g64[k]).max(), floors[k]):.3e}")
    assert_scalar_close(loss, loss64, what=f"{what}: loss")
    if clip:
        assert_scalar_close(total, total64, what=f"{what}: total norm")
    else:
        assert total is None
    assert_grads_as_accurate(grads, g32, g64, what=f"{what}: grad", floor_fn=floors.get)
    assert float(eng._g_flat.abs().max()) == 0.0, "the gradient buffer is left cleared"
    assert np.array_equal(get_weights(eng)["user_output.weight"], c.w["user_output.weight"])
    return grads


def check_forward(eng, key, what):
    """``model(*batch)`` and ``model(*batch, evaluation=True)`` against the fp64 scores."""
    c = ce.fixture(key)
    sp, sn = ce.scores64(c.w, c.batch)
    pos, neg = eng.model(*c.batch)
    assert pos.dtype == torch.float32 and tuple(pos.shape) == tuple(neg.shape) == (len(c.batch[0]),)
    assert_tensor_close(pos.cpu().numpy(), sp, what=f"{what}: forward pos")
    assert_tensor_close(neg.cpu().numpy(), sn, what=f"{what}: forward neg")
    only = eng.model(*c.batch, evaluation=True)
    assert_tensor_close(only.cpu().numpy(), sp, what=f"{what}: forward(evaluation=True)")


def check_untouched_rows(c, grads, what):
    """A user in no list of the batch gets no row gradient in ``user_output``, and none in ``user_memory`` unless it
    is a sample's user: exactly 0.0, the kernel never adds there."""
    u, p, n, pn, pl, nn_, nl = c.batch
    U = c.w["user_memory.weight"].shape[0]
    listed = np.zeros(U, dtype=bool)
    for nbr, lens in ((pn, pl), (nn_, nl)):
        for b in range(len(u)):
            listed[nbr[b, :lens[b]]] = True
    is_user = np.zeros(U, dtype=bool)
    is_user[u] = True
    assert (~listed & ~is_user).sum() >= 1, "the fixture has no untouched user"
    assert float(np.abs(grads["user_memory.weight"][~listed & ~is_user]).max()) == 0.0, f"{what}: user_memory"
    assert float(np.abs(grads["user_output.weight"][~listed]).max()) == 0.0, f"{what}: user_output"


@pytest.mark.parametrize("D", ce.WIDTH_CASES)
def test_every_row_width_at_its_round_seams(hip_device, D):
    """Part 1.  D = 4: one lane per row, 64 rows per wave, 16 rows per atomic instruction; 8 and 12: the narrow float4
    widths; 10, 30, 50: strided columns at 4, 8 and 16 lanes per row; 65 and 130: strided columns with one and two live
    columns in the scatter's upper slots; 68 and 132: float4 widths whose upper lanes of a group hold no column.  Lists
    of 1, R - 1, R + 1, 4 R - 1, 4 R, 4 R + 1, 8 R + 1 rows (R = rows per wave at that width) and two in between, each
    as a positive and as a negative list, in the padded and in the CSR form."""
    c = ce.fixture(D)
    assert ce.derived(D) == ce.DERIVED[D]
    eng = engine_of(c)
    for form, batch in (("padded", c.batch), ("csr", c.triples)):
        grads = check_backward(eng, D, batch, f"D {D} {form}")
        check_untouched_rows(c, grads, f"D {D} {form}")
    check_forward(eng, D, f"D {D}")


def test_block_stride_loop(hip_device):
    """Part 2.  1030 samples on a grid capped at 1024 blocks: blocks 0 .. 5 run a second sample on the same shared
    memory, in the training path (both forms) and in the forward-only path; one SGD step lands on the restatement's; a
    second ``backward_only`` is held to the same bounds (float atomics: no bit equality is asked)."""
    key = ce.STRIDE_CASE
    c = ce.fixture(key)
    assert len(c.batch[0]) > ce.MAX_BLOCKS
    lr = 0.1
    eng = engine_of(c, "sgd", lr)
    runs = {}
    for form, batch in (("padded", c.batch), ("csr", c.triples), ("csr again", c.triples)):
        runs[form] = check_backward(eng, key, batch, f"stride {form}")
        check_untouched_rows(c, runs[form], f"stride {form}")
    _, g64, _, g32, floors = ce.reference(key)
    tol = ce.tolerances(g32, g64, floors)
    for k in KEYS:
        apart = float(np.abs(runs["csr again"][k] - runs["csr"][k]).max())
        assert apart <= tol[k], f"stride: two runs differ in {k} by {apart:.3e} > {tol[k]:.3e}"
    check_forward(eng, key, "stride")
    loss64 = ce.reference(key)[0]
    loss = eng.train_single_batch(c.batch)
    assert_scalar_close(loss, loss64, what="stride: loss of the step")
    w_ref = {k: v.copy() for k, v in c.w.items()}
    cn.cmn_train_step(w_ref, cn.new_opt_state(w_ref, "sgd"), c.batch, c.lam, c.clip, "sgd", lr)
    assert float(np.abs(w_ref["item_memory.weight"] - c.w["item_memory.weight"]).max()) > 1e-4, "the step moves nothing"
    assert_sgd_exact(get_weights(eng), w_ref, c.w, "stride: SGD step")
    assert float(eng._g_flat.abs().max()) == 0.0


@pytest.mark.parametrize("D,shape", ce.SHARP_CASES)
def test_softmax_with_real_dynamic_range(hip_device, D, shape):
    """Part 3.  Hop-0 logits over a spread of 60 .. 80 along a list of twelve wave-shares and one row: ascending (every
    round raises the running maximum, every merge rescales), descending (the first row dominates every later one), flat
    with one late peak (the maximum arrives in the last full round); sample 0's two queries run on the same list."""
    key = (D, shape)
    c = ce.fixture(key)
    eng = engine_of(c)
    for form, batch in (("padded", c.batch), ("csr", c.triples)):
        check_backward(eng, key, batch, f"D {D} {shape} {form}")
    check_forward(eng, key, f"D {D} {shape}")


def test_neighbour_listed_more_than_once(hip_device):
    """Part 4.  Padded form: one neighbour at three slots of a list (one of them the last) and a list that is one user
    five times; the repeated neighbours' rows are held like every other row (the atomics add each slot's share)."""
    key = ce.DUPLICATE_CASE
    c = ce.fixture(key)
    eng = engine_of(c)
    grads = check_backward(eng, key, c.batch, "duplicates")
    _, g64, _, g32, _ = ce.reference(key)
    u, p, n, pn, pl, nn_, nl = c.batch
    for rep in (int(pn[0, pl[0] - 1]), int(nn_[1, 0])):
        for k in ("user_memory.weight", "user_output.weight"):
            # (a list that is ONE row k times has da = 0: only user_output's row is non-zero there)
            assert float(np.abs(g64[k][rep]).max()) > 0.0 or (k == "user_memory.weight" and rep == int(nn_[1, 0]))
            assert_as_accurate_as_reference(grads[k][rep], g32[k][rep], g64[k][rep], what=f"duplicates: {k} row {rep}",
                                            scale_floor=float(np.abs(g64[k]).max()))
    check_forward(eng, key, "duplicates")


def test_saturated_bpr_term(hip_device):
    """Part 5.  x = s+ - s- at -32 and +32: -log(sigmoid(x) + 1e-12) and its hand-written derivative where sigmoid(x)
    is 1e-14 and where it rounds to 1; the clip off.  Then one Adam step: the weights stay finite."""
    key = ce.SATURATED_CASE
    c = ce.fixture(key)
    eng = engine_of(c, "adam", 1e-3)
    grads = check_backward(eng, key, c.batch, "saturated", clip=False)
    assert all(np.isfinite(v).all() for v in grads.values())
    check_forward(eng, key, "saturated")
    eng.load_optimizer_state(0)
    loss = eng.train_single_batch(c.batch)
    assert_scalar_close(loss, ce.reference(key)[0], what="saturated: loss of the step")
    w1 = get_weights(eng)
    assert all(np.isfinite(v).all() for v in w1.values())
    assert any(not np.array_equal(w1[k], c.w[k]) for k in KEYS), "the step moved nothing"


@pytest.mark.parametrize("D", [3, 257])
def test_width_limits_are_refused(hip_device, D):
    """Part 6.  ``emb_dim`` below 4 or above 256 is refused by the library before anything is launched: the weights and
    the gradient buffer are as they were; an engine built afterwards at D = 4 works."""
    from beta_recsys_amd._lib import HiprecError

    w, rowptr, col, triples = ce.synthetic(12, D, [1, 3, 5], 2, seed=D)
    batch = cn.padded_batch(rowptr, col, *triples)
    eng = make_engine(w, rowptr, col, "sgd", 0.01, 0.9, ce.LAM, ce.CLIP, 2)
    before = eng.model.flat.clone()
    for call in (lambda: eng.backward_only(batch), lambda: eng.backward_only(triples),
                 lambda: eng.train_single_batch(batch), lambda: eng.model(*batch),
                 lambda: eng.model(*batch, evaluation=True)):
        with pytest.raises((ValueError, HiprecError)):
            call()
    torch.cuda.synchronize()
    assert torch.equal(eng.model.flat, before), "the weights moved"
    assert float(eng._g_flat.abs().max()) == 0.0, "a gradient was written"
    c = ce.fixture(4)
    check_backward(engine_of(c), 4, c.batch, f"D 4 after D {D}")
