"""GPU parity tests of LightGCN (csrc/lightgcn.hip, csrc/spmm_sliced.hip, lightgcn.py) where the goldens and
tests/test_lightgcn_gpu.py do not reach: the loss kernel at 2 and 4 columns per lane and at widths that are no multiple
of 64, in the row-major and the sliced layout; slice width 2 in a training step, with host and device dropout; depths
0, 1, 4 and 5 (the code of ``propagate_sliced`` that runs only at L < 2, the ping-pong parity beyond 3); a hub row and
rows without edges under the flush variants only LightGCN uses (``final_out`` into the row-major gradient,
``zero_out`` of buffer 0); the last node count of each slice width (row cap exactly 128) and the first of the next
form; a graph no rank-one factoring explains under ``auto``; the second trip of the loss and predict kernels' grid-stride
loops; both saturated branches of the softplus, one triple, one user throughout, ``pos == neg``, ``decay = 0``,
``keep_pro = 1``; and the optimizer launch that stages the next step at D = 100, L = 1 and 3.

The inputs are tests/lightgcn_edges.py's, which tests/test_lightgcn_edges_host.py shows to see a defect of each kind;
the yardsticks are those of tests/test_lightgcn_gpu.py: the fp64 oracle, ``assert_scalar_close``,
``assert_grads_as_accurate`` and ``assert_tensor_close`` with their defaults.  Every asserted step runs on an engine
that has first run another step (other weights, another batch): a buffer the step does not rewrite shows.
``pytest -s`` prints, per case, the form taken and each gradient's error against fp64 next to the fp32 oracle's own."""
import numpy as np
import pytest
import torch

import lightgcn_edges as le
from helpers import assert_as_accurate_as_reference, assert_grads_as_accurate, assert_scalar_close, assert_tensor_close
from oracle import lightgcn_numpy as olg
from test_lightgcn_gpu import get_weights, load_weights, make_engine

pytestmark = pytest.mark.gpu
LR = 0.05
ALL_PAIRS_LIMIT = 1 << 16      # predict runs on all (user, item) pairs up to here, else on GRID_WAVES + 1 random ones


def case_modes(keys):
    return [(k, m, r) for k in keys for m in le.spmm_modes(k) for r in le.settings(k)[1]]


def tensors(batch):
    return tuple(torch.from_numpy(np.asarray(x)) for x in batch)


def engine_of(c, spmm, rng, optimizer="sgd", lr=LR, **extra):
    eng = make_engine(c.U, c.I, c.D, c.L, optimizer, lr, len(c.batch[0]), c.adj, c.keep_pro, c.decay, spmm=spmm,
                      dropout_rng=rng, dropout_seed=c.seed, **extra)
    eng.model.train()
    return eng


def check_forms(eng, c, spmm, rng="torch_cpu"):
    """The graph the engine built against the form table: slice width, factored or not, the library's row cap."""
    from beta_recsys_amd import _lib

    lib, N = _lib.load(), c.U + c.I
    width, factored, n_per_lane = le.FORM_TABLE[c.key]
    assert (int(lib.hiprec_sliced_width(N, c.D)), int(lib.hiprec_sliced_row_cap(N, c.D))) == \
        (width, le.sliced_row_cap(N, c.D)) == (le.sliced_width(N, c.D), le.sliced_row_cap(N, c.D))
    gr = eng.model.graph()
    got = gr.get("slice_w", 0)
    has_scale = bool(got) and "col_scale" in gr["sliced"][1]
    print(f"{c.key} [{spmm}, {rng}]: N {N}, D {c.D}, L {c.L}, B {len(c.batch[0])}: slice width {got}, "
          f"{'factored' if has_scale else 'values' if got else 'gather'}, row cap {gr.get('row_cap', 0)}, NPL {n_per_lane}")
    assert got == (0 if spmm == "gather" else width)
    assert n_per_lane == le.npl(c.D)
    if got:
        for tag in ("sliced", "sliced_t"):
            assert ("col_scale" in gr[tag][1]) == (factored and spmm == "auto"), tag
        assert gr["row_cap"] == le.sliced_row_cap(N, c.D)


def pollute(eng, c):
    """One ``backward_only`` with other weights and another batch: what it leaves in the workspaces is not the
    asserted step's."""
    rng = np.random.default_rng(c.seed + 7)
    load_weights(eng, le.draw_weights(rng, c.U, c.I, c.D, gain=2.0))
    torch.manual_seed(c.seed + 7)
    eng.backward_only(tensors(le.random_batch(rng, c.U, c.I, 31)))
    load_weights(eng, c.w)


def step_reference(eng, c, host):
    """The ``Ref`` of the step the engine has just run: the fixture's own where the mask was drawn on the host under
    the case's seed (asserted), else the oracle fed with the mask read back -- on which the fp32 oracle must be as fair
    a yardstick as tests/test_lightgcn_edges_host.py shows it to be on the fixtures."""
    kept = eng.model.last_keep_mask().cpu().numpy().astype(bool)
    if host:
        assert np.array_equal(kept, c.mask), "the engine's draw is not the fixture's mask"
        return le.reference(c.key)
    if c.keep_pro == 1.0:
        assert kept.all()
    else:
        assert abs(kept.mean() - c.keep_pro) < 0.1, kept.mean()
    ref = le.reference_of(c, kept)
    assert_scalar_close(ref.loss32, ref.loss64, what="the fp32 oracle's loss under the device's mask")
    for k in ref.g64:
        assert_tensor_close(ref.g32[k], ref.g64[k], what=f"the fp32 oracle's {k} under the device's mask")
    return ref


def check_backward(eng, c, what, host):
    """Loss and both gradients of one ``backward_only`` against fp64; returns ``(gradients, Ref)``."""
    if host:
        torch.manual_seed(c.seed)
    loss, grads = eng.backward_only(tensors(c.batch))
    ref = step_reference(eng, c, host)
    got = {k: v.cpu().numpy() for k, v in grads.items()}
    print(f"{what}: loss {loss!r} vs exact {ref.loss64!r}")
    for k in ref.g64:
        print(f"  grad {k}: err vs exact {np.abs(got[k] - ref.g64[k]).max():.3e}, fp32 oracle's "
              f"{np.abs(ref.g32[k] - ref.g64[k]).max():.3e}, scale {np.abs(ref.g64[k]).max():.3e}")
    assert np.isfinite(loss) and all(np.isfinite(v).all() for v in got.values())
    assert_scalar_close(loss, ref.loss64, what=f"{what}: loss")
    assert_grads_as_accurate(got, ref.g32, ref.g64, f"{what}: grad")
    return got, ref


def predict_pairs(c):
    if c.pairs is not None:
        return c.pairs
    if c.U * c.I <= ALL_PAIRS_LIMIT:
        return np.divmod(np.arange(c.U * c.I), c.I)
    rng = np.random.default_rng(c.seed + 9)
    return rng.integers(0, c.U, le.GRID_WAVES + 1), rng.integers(0, c.I, le.GRID_WAVES + 1)


def check_forward(eng, c, ref, what):
    """Eval-mode ``forward`` tables and ``predict`` (sigmoid outputs: scale floor 1) against fp64."""
    eng.model.eval()
    ua, ia = eng.model.forward()
    assert ua.shape == (c.U, c.D) and ia.shape == (c.I, c.D)
    assert_tensor_close(torch.cat([ua, ia]).cpu().numpy(), ref.table64, what=f"{what}: eval-mode forward")
    users, items = predict_pairs(c)
    scores = eng.model.predict(users, items).cpu().numpy()
    want = 1.0 / (1.0 + np.exp(-(ref.table64[users] * ref.table64[c.U + items]).sum(1)))
    assert_tensor_close(scores, want, what=f"{what}: predict on {len(users)} pairs", scale_floor=1.0)
    eng.model.train()


def check_step(eng, c, what, host):
    """One whole ``train_single_batch`` from the case's weights: the loss, weights that moved, a cleared gradient."""
    load_weights(eng, c.w)
    if host:
        torch.manual_seed(c.seed)
    loss = eng.train_single_batch(tensors(c.batch))
    ref = step_reference(eng, c, host)
    assert_scalar_close(loss, ref.loss64, what=f"{what}: loss of the step")
    got = get_weights(eng)
    assert any(not np.array_equal(got[k], c.w[k]) for k in c.w), "the step moved nothing"
    assert float(eng._g_flat.abs().max()) == 0, "the gradient buffer is left cleared"


def run_case(key, spmm, rng):
    c = le.fixture(key)
    host = rng == "torch_cpu"
    what = f"{key} [{spmm}, {rng}]"
    eng = engine_of(c, spmm, rng)
    check_forms(eng, c, spmm, rng)
    pollute(eng, c)
    got, ref = check_backward(eng, c, what, host)
    check_forward(eng, c, ref, what)
    check_backward(eng, c, what + " again", host)
    check_step(eng, c, what, host)
    return eng, got, ref


@pytest.mark.parametrize("key,spmm,rng", case_modes(le.WIDTH_CASES))
def test_widths(hip_device, key, spmm, rng):
    """L = 3 at D = 1, 6, 7, 63, 64, 65, 70, 100, 128, 129, 130, 200, 256: the loss kernel at 1, 2 and 4 columns per
    lane with a partial last lane group, row-major (gather) and sliced at widths 4 and 2, factored and with values."""
    run_case(key, spmm, rng)


@pytest.mark.parametrize("key,spmm,rng", case_modes(le.DEPTH_CASES))
def test_depths(hip_device, key, spmm, rng):
    """D = 16 at L = 0 (no pass at all: the gradient is the loss kernel's l = 0 term), 1 (mode 2 and ``final_out`` in
    one pass, buffer 0 cleared by a fill), 2, 4 and 5 (``zero_out`` with the last pass even and odd).  At L = 0 the rows
    of ids the batch does not name are exactly zero."""
    eng, got, ref = run_case(key, spmm, rng)
    c = le.fixture(key)
    if c.L == 0:
        for k in olg.KEYS:
            absent = ~ref.g64[k].any(axis=1)
            assert absent.any() and not got[k][absent].any(), f"{key} [{spmm}]: {k}: a row the batch does not name moved"


@pytest.mark.parametrize("key,spmm,rng", case_modes(le.HUB_CASES))
def test_hub_and_edgeless_rows(hip_device, key, spmm, rng):
    """D^-1 A without the identity, a hub row of 1300 edges, seven rows without edges (two in the batch), at slice
    widths 4 and 2: spill and empty rows through ``final_out`` and ``zero_out``, after a step that left other values
    everywhere."""
    c = le.fixture(key)
    eng, _, _ = run_case(key, spmm, rng)
    if spmm != "gather":
        gr = eng.model.graph()
        for tag in ("sliced", "sliced_t"):
            spill, none = gr[tag][1]["spill_row"].cpu().numpy(), gr[tag][1]["empty_row"].cpu().numpy()
            print(f"{key} [{spmm}] {tag}: lane_slots {gr[tag][0].lane_slots}, spill rows {spill.tolist()}, "
                  f"empty rows {none.tolist()}")
            assert c.U + le.HUB in spill and np.array_equal(none, le.empty_rows(c))


@pytest.mark.parametrize("key,spmm,rng", case_modes(list(le.THRESHOLD_CASES) + [le.BIG_CASE]))
def test_thresholds(hip_device, key, spmm, rng):
    """D = 4 at N = 10107 (width 4, row cap 128), 10108 (width 2), 20343 (width 2, row cap 128), 20344 and 65536 (the
    gather): the slice and its spill rows fill the LDS to the last byte."""
    run_case(key, spmm, rng)


@pytest.mark.parametrize("key,spmm,rng", case_modes(["general", "one_triple", "one_user", "pos_eq_neg", "decay0",
                                                    "keep1"] + list(le.DEVICE_CASES)))
def test_graph_and_batch_edges(hip_device, key, spmm, rng):
    """``auto`` on values that are not rank-one (the values stream, no ``col_scale``); a batch of one triple; one user
    throughout (every atomic of the user side on one row); ``pos == neg`` on half the rows; ``decay = 0``;
    ``keep_pro = 1`` with both draws; the device draw at slice widths 2 and 4 (the mask read back for the oracle)."""
    run_case(key, spmm, rng)


@pytest.mark.parametrize("spmm", le.spmm_modes("seam"))
def test_seam_of_the_loss_kernel(hip_device, spmm):
    """B = 8193: triple 8192 is the second trip of wave 0.  Its user and both its items occur nowhere else in the
    batch; their gradient rows are held to fp64 at those rows' own scale, and are not zero."""
    c = le.fixture("seam")
    _, got, ref = run_case("seam", spmm, "torch_cpu")
    users, pos, neg = c.batch
    for k, row in (("user_embedding.weight", users[-1]), ("item_embedding.weight", pos[-1]),
                   ("item_embedding.weight", neg[-1])):
        print(f"seam [{spmm}]: {k}[{row}]: err {np.abs(got[k][row] - ref.g64[k][row]).max():.3e}, fp32 oracle's "
              f"{np.abs(ref.g32[k][row] - ref.g64[k][row]).max():.3e}, scale {np.abs(ref.g64[k][row]).max():.3e}")
        assert got[k][row].any(), "the second trip did not run"
        assert_as_accurate_as_reference(got[k][row], ref.g32[k][row], ref.g64[k][row], what=f"seam [{spmm}]: {k}[{row}]")


@pytest.mark.parametrize("spmm", le.spmm_modes("seam_predict"))
def test_seam_of_the_predict_kernel(hip_device, spmm):
    """8193 (user, item) pairs: pair 8192 is the second trip of wave 0."""
    c = le.fixture("seam_predict")
    eng = engine_of(c, spmm, "torch_cpu")
    check_forms(eng, c, spmm)
    pollute(eng, c)
    check_forward(eng, c, le.reference("seam_predict"), f"seam_predict [{spmm}]")


@pytest.mark.parametrize("spmm", le.spmm_modes("saturated"))
def test_saturated_softplus(hip_device, spmm):
    """Weights x 3 at D = 64: x beyond +-20 (and beyond +-89, where expf overflows) and near 0 in one batch.  The loss
    is finite; the rows of the x < -20 triples are held to fp64 at their own scale and hold no NaN (those triples' own
    terms are tiny -- sigmoid(x) underflows -- so what the rows hold comes from their other triples, their neighbours
    and the L2 term)."""
    c = le.fixture("saturated")
    _, got, ref = run_case("saturated", spmm, "torch_cpu")
    x = le.saturated_stats(c)
    low = x < le.SAT_LOW
    assert low.sum() >= 5 and (x > le.SAT_HIGH).sum() >= 5
    users, pos, neg = (b[low] for b in c.batch)
    for k, rows in (("user_embedding.weight", np.unique(users)),
                    ("item_embedding.weight", np.unique(np.concatenate([pos, neg])))):
        print(f"saturated [{spmm}]: {k} rows of x < -20: err {np.abs(got[k][rows] - ref.g64[k][rows]).max():.3e}, "
              f"fp32 oracle's {np.abs(ref.g32[k][rows] - ref.g64[k][rows]).max():.3e}, scale "
              f"{np.abs(ref.g64[k][rows]).max():.3e} (tensor {np.abs(ref.g64[k]).max():.3e})")
        assert not np.isnan(got[k][rows]).any()
        assert_as_accurate_as_reference(got[k][rows], ref.g32[k][rows], ref.g64[k][rows],
                                        what=f"saturated [{spmm}]: {k} rows of x < -20")


@pytest.mark.parametrize("key", list(le.STAGED_CASES))
def test_staged_next_step(hip_device, key):
    """``hiprec_lightgcn_opt_stage`` at D = 100 (no multiple of 64), L = 1 and 3: three consecutive adam steps, each
    held to the oracle fed with the mask read back; steps 2 and 3 consume what the optimizer launch staged (counted:
    only step 1 prepares itself); the losses agree to 1e-6 with a run at ``stage_next_step=False``."""
    from beta_recsys_amd import _lib

    c = le.fixture(key)
    rng = np.random.default_rng(c.seed + 3)
    batches = [c.batch] + [le.random_batch(rng, c.U, c.I, len(c.batch[0])) for _ in range(2)]
    runs = {}
    for staged in (True, False):
        eng = engine_of(c, "auto", "device", "adam", LR, stage_next_step=staged)
        check_forms(eng, c, "auto", "device")
        assert eng.model.can_stage_next_step() == staged
        load_weights(eng, c.w)
        w = {k: v.copy() for k, v in c.w.items()}
        st = olg.new_opt_state(w, "adam")
        lib, calls = _lib.load(), []
        plain = lib.hiprec_lightgcn_step_values
        lib.hiprec_lightgcn_step_values = lambda *a: (calls.append(eng.model._step), plain(*a))[1]
        losses = []
        try:
            for s, batch in enumerate(batches):
                loss = eng.train_single_batch(tensors(batch))
                keep = eng.model.last_keep_mask().cpu().numpy().astype(bool)
                want, g_ref = olg.lightgcn_grads(w, olg.apply_edge_dropout(c.adj, keep, c.keep_pro), c.L, *batch, c.decay)
                olg.opt_step(w, g_ref, st, "adam", LR)
                print(f"{key} staged={staged}: step {s}: loss {loss!r} vs oracle {want!r}")
                assert_scalar_close(loss, want, what=f"{key}: loss of step {s} (staged={staged})")
                losses.append(loss)
        finally:
            lib.hiprec_lightgcn_step_values = plain
        assert calls == ([1] if staged else [1, 2, 3]), calls
        assert float(eng._g_flat.abs().max()) == 0
        runs[staged] = losses
    for a_, b_ in zip(runs[True], runs[False]):
        assert abs(a_ - b_) <= 1e-6 * abs(b_)


def test_errors(hip_device):
    """D = 257 is refused (no loss kernel holds more than 256 columns); an id out of range in ``predict`` raises
    IndexError and the next call is clean."""
    from beta_recsys_amd._lib import HiprecError

    c = le.fixture("l2")
    wide = make_engine(c.U, c.I, le.MAX_DIM + 1, c.L, "sgd", LR, len(c.batch[0]), c.adj, c.keep_pro, c.decay)
    wide.model.train()
    with pytest.raises(HiprecError, match="257"):
        wide.backward_only(tensors(c.batch))
    torch.cuda.synchronize()
    eng = engine_of(c, "auto", "torch_cpu")
    load_weights(eng, c.w)
    ref = le.reference("l2")
    for users, items in (([0, c.U], [0, 1]), ([0, 1], [0, c.I]), ([-1], [0])):
        with pytest.raises(IndexError):
            eng.model.predict(np.asarray(users), np.asarray(items))
    check_forward(eng, c, ref, "after the refused calls")
