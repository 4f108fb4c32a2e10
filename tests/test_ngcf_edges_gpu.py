"""GPU parity tests of NGCF (csrc/ngcf.hip, csrc/spmm_sliced.hip) where the goldens and tests/test_ngcf_gpu.py do not
reach: every pair of (fused or three-launch forward hop, fused or per-hop backward), idle column tiles and k-loop tails
of the fused hop kernels, four to six hops, widths up to the limit of 256, slice widths 4, 2 and none, the edges of the
16-row hop tile, the sliced SpMM's spill and empty rows, both branches of the normalize backward's clamp, device-drawn
keep bytes held to their numbers, the width and depth limits, and the older launch forms at fused-eligible shapes.  The
inputs are tests/ngcf_edges.py's, which tests/test_ngcf_edges_host.py shows to see a defect of each kind; the yardsticks
are those of tests/test_ngcf_gpu.py: the fp64 oracle, ``assert_scalar_close``, ``assert_as_accurate_as_reference`` with
the ``terms`` floors, ``assert_tensor_close``, ``ngcf_band`` and ``assert_step_close``."""
import numpy as np
import pytest
import torch

import ngcf_edges as ne
from helpers import assert_as_accurate_as_reference, assert_scalar_close, assert_step_close, assert_tensor_close
from oracle import ngcf_numpy as onp
from test_ngcf_gpu import get_weights, kept_masks, load_weights, make_engine
from test_oracle_golden_ngcf import ngcf_band, ngcf_grad_rel

pytestmark = pytest.mark.gpu
LR = {"sgd": 0.05, "adam": 1e-3}
EMB = ("user_embedding.weight", "item_embedding.weight")


def modes(key):
    return ["auto", "gather"] + (["sliced_values"] if ne.FORM_TABLE[key][2] else [])


def case_modes(keys):
    return [(k, m) for k in keys for m in modes(k)]


def feed_masks(eng, masks):
    """The engine's training forwards use the fixture's keep masks: what ``draw_keep_masks`` hands to the plan is
    overwritten with them (the draw itself, the step counter and the buffers stay the engine's)."""
    if masks is None:
        return
    model, draw = eng.model, eng.model.draw_keep_masks

    def fed():
        out = draw()
        if out is not None:
            for buf, m in zip(out, masks):
                if m is not None:
                    buf.copy_(torch.from_numpy(m.astype(np.uint8)))
        return out

    model.draw_keep_masks = fed


def engine_of(c, optimizer="sgd", spmm="auto", **extra):
    eng = make_engine(c.U, c.I, c.dims[0], c.dims[1:], c.drop, optimizer, LR[optimizer], c.batch_size, c.adj, c.decay,
                      spmm=spmm, **extra)
    load_weights(eng, c.w)
    eng.model.train()
    feed_masks(eng, c.masks)
    return eng


def check_forms(eng, key, spmm):
    """What the engine shows of the form table: the slice width of the graphs it built."""
    fwd, bwd, w = ne.FORM_TABLE[key]
    assert ne.forms(ne.fixture(key)) == (fwd, bwd, w)
    got = eng.model.graph().get("slice_w", 0)
    print(f"{key} [{spmm}]: dims {ne.fixture(key).dims}, forward {'/'.join(fwd)}, backward {bwd}, slice width {w} "
          f"(engine: {got})")
    assert got == (0 if spmm == "gather" else w)
    if got:
        assert ("row_scale" in eng.model.graph()["sliced"][1]) == (spmm == "auto"), "factored under auto only"


def check_backward(eng, c, ref, what):
    """Loss and every gradient of one ``backward_only`` against ``ref``; exact zeros where the restatement has whole
    zero rows; the keep bytes are the fixture's; the gradient buffer is left cleared."""
    loss, grads = eng.backward_only(c.batch)
    got = {k: v.cpu().numpy() for k, v in grads.items()}
    for mine, want in zip(kept_masks(eng, c.drop), c.masks or [None] * len(c.drop)):
        assert (mine is None) == (want is None) and (want is None or np.array_equal(mine, want))
    print(f"{what}: loss {loss!r} vs exact {ref.loss64!r}")
    for k in ref.g64:
        print(f"  grad {k}: err vs exact {np.abs(got[k] - ref.g64[k]).max():.3e}, fp32 oracle's "
              f"{np.abs(ref.g32[k] - ref.g64[k]).max():.3e}, scale "
              f"{max(np.abs(ref.g64[k]).max(), ref.terms.get(k, 0.0)):.3e}")
    assert_scalar_close(loss, ref.loss64, what=f"{what}: loss")
    for k in ref.g64:
        assert_as_accurate_as_reference(got[k], ref.g32[k], ref.g64[k], what=f"{what}: grad {k}",
                                        scale_floor=ref.terms.get(k, 0.0))
    for k in EMB:
        zero = ~ref.g64[k].any(axis=1)
        assert not got[k][zero].any(), f"{what}: {k}: a row the batch cannot reach has a gradient"
    assert float(eng._g_flat.abs().max()) == 0.0, "the gradient buffer is left cleared"
    return got


def check_forward(eng, c, ref, what):
    """Eval-mode ``forward`` and ``predict`` against the fp64 table; with masks, the training forward too, with exact
    zeros where the table has them (dropped units, a row dropped whole)."""
    U = c.U
    eng.model.eval()
    ua, ia = eng.model(None)
    assert_tensor_close(torch.cat([ua, ia]).cpu().numpy(), ref.all64, what=f"{what}: forward")
    users, items = c.batch[0], c.batch[1]
    scores = eng.model.predict(users, items)
    assert_tensor_close(scores.cpu().numpy(), (ref.all64[users] * ref.all64[U + items]).sum(1), what=f"{what}: predict")
    eng.model.train()
    if c.masks is not None:
        ua, ia = eng.model(None)
        got = torch.cat([ua, ia]).cpu().numpy()
        assert_tensor_close(got, ref.all64_train, what=f"{what}: training forward")
        assert not got[ref.all64_train == 0].any(), f"{what}: a dropped unit is not exactly zero"


def check_step(c, ref, spmm, optimizer, what):
    """One ``train_single_batch`` from the fixture's weights against the oracle's step on the fp32 gradients."""
    lr = LR[optimizer]
    eng = engine_of(c, optimizer, spmm)
    eng.load_optimizer_state(0)
    loss, reg = eng.train_single_batch(c.batch)
    assert reg == 0.0
    assert_scalar_close(loss, ref.loss64, what=f"{what}: loss of the step")
    st = onp.new_opt_state(c.w, optimizer)
    band = ngcf_band(c.w, st, ref.g32, optimizer, lr, rel=ngcf_grad_rel(ref.g32, ref.g64))
    w_ref = {k: v.copy() for k, v in c.w.items()}
    onp.opt_step(w_ref, ref.g32, st, optimizer, lr)
    got = get_weights(eng)
    assert any(not np.array_equal(got[k], c.w[k]) for k in c.w), "the step moved nothing"
    for k in c.w:
        assert_step_close(c.w[k], got[k], w_ref[k], band[k], what=f"{what}: {optimizer} weights {k}")
    assert float(eng._g_flat.abs().max()) == 0.0


def run_case(key, spmm):
    """``backward_only`` twice on one engine (the sliced path relies on the backward leaving ``d_all`` zero), the
    forwards, then one step per optimizer."""
    c, ref = ne.fixture(key), ne.reference(key)
    eng = engine_of(c, "sgd", spmm)
    check_forms(eng, key, spmm)
    check_backward(eng, c, ref, f"{key} [{spmm}]")
    check_forward(eng, c, ref, f"{key} [{spmm}]")
    check_backward(eng, c, ref, f"{key} [{spmm}] again")
    for optimizer in ("sgd", "adam"):
        check_step(c, ref, spmm, optimizer, f"{key} [{spmm}]")
    return eng


@pytest.mark.parametrize("key,spmm", case_modes(ne.WIDTH_CASES))
def test_width_chains(hip_device, key, spmm):
    """[32,16,8] and [48,48,20]: a fused backward next to an unfused forward hop, idle column tiles (di = 48) and a
    k-loop tail (dout = 20); [128,64,16]: the largest fused forward; [64]*5: a group of exactly 16 problems; [16]*6 and
    [16]*7: five and six hops, the per-hop backward behind fused forwards; [100,200,256]: columns lane + 64 k up to the
    limit; [10,6,12] at odd N: slice width 2 and bi_mul's scalar tail; [7,5,3]: odd widths, no sliced form;
    [16,18,16]: hop inputs of slice widths 4 and 2, so ``auto`` falls back to the gather."""
    run_case(key, spmm)


@pytest.mark.parametrize("key,spmm", case_modes(ne.TILE_CASES))
def test_tile_geometry(hip_device, key, spmm):
    """N = 9 (below one 16-row tile), 17 (one row in the second tile), 64 (whole tiles), 65; the user / item seam
    inside a tile."""
    run_case(key, spmm)


@pytest.mark.parametrize("key,spmm", case_modes(ne.BATCH_CASES + (ne.DROPPED_ROW_CASE,)))
def test_dropout_and_batch(hip_device, key, spmm):
    """mess_dropout [0.5, 0.3] on [32,16,8] with one user and two items throughout (pos == neg in one triple) and with
    one triple at a configured batch size of 8; and a batch row dropped whole (norm exactly 0)."""
    run_case(key, spmm)
    if key == ne.DROPPED_ROW_CASE:
        c, ref = ne.fixture(key), ne.reference(key)
        assert not ref.all64_train[c.batch[0][0], c.dims[0] + c.dims[1]:].any()


@pytest.mark.parametrize("key,spmm", case_modes(ne.GRAPH_CASES))
def test_sliced_spill_and_empty_rows(hip_device, key, spmm):
    """D^-1 A without the identity and a hub row of 1300 edges: the sliced SpMM's ``final_out`` path (set in the
    forward, added to in the backward) on rows that are several runs and on rows without edges, at slice widths 4 and
    2, factored and with values; edgeless nodes the batch does not touch keep exactly zero gradient rows."""
    c = ne.fixture(key)
    eng = run_case(key, spmm)
    empty = ne.empty_rows(c)
    if spmm != "gather":
        gr = eng.model.graph()
        for tag in ("sliced", "sliced_t"):
            spill, none = gr[tag][1]["spill_row"].cpu().numpy(), gr[tag][1]["empty_row"].cpu().numpy()
            print(f"{key} [{spmm}] {tag}: lane_slots {gr[tag][0].lane_slots}, spill rows {spill.tolist()}, "
                  f"empty rows {none.tolist()}")
            assert c.U + ne.HUB in spill and np.array_equal(none, empty)
    g64 = ne.reference(key).g64
    untouched = np.setdiff1d(empty, np.concatenate([c.batch[0], c.U + c.batch[1], c.U + c.batch[2]]))
    assert len(untouched) >= 3
    assert not np.concatenate([g64[k] for k in EMB])[untouched].any()     # (check_backward held the engine to these)


@pytest.mark.parametrize("spmm", modes(ne.CLAMP_CASE))
def test_normalize_clamp(hip_device, spmm):
    """Row norms of the last hop on both sides of eps = 1e-12: the ``nrm >= eps`` selection of the normalize backward.
    Gradients only (the last hop's are of order 1e10: a step means nothing)."""
    key = ne.CLAMP_CASE
    c, ref = ne.fixture(key), ne.reference(key)
    eng = engine_of(c, "sgd", spmm)
    check_forms(eng, key, spmm)
    check_backward(eng, c, ref, f"clamp [{spmm}]")
    nrm = eng.model._ws["nrm"][-1].cpu().numpy()
    print(f"clamp [{spmm}]: {(nrm < ne.EPS).sum()} rows below eps, {(nrm >= ne.EPS).sum()} above")
    assert (nrm < ne.EPS).sum() >= len(nrm) / 4 and (nrm >= ne.EPS).sum() >= len(nrm) / 4
    check_forward(eng, c, ref, f"clamp [{spmm}]")
    check_backward(eng, c, ref, f"clamp [{spmm}] again")


@pytest.mark.parametrize("spmm", ["auto", "gather"])
def test_device_drawn_keep_bytes(hip_device, spmm):
    """dropout_rng = "device" on [32,16,8] (keep bytes drawn in the fused hop kernel at hop 0, in ngcf_act_kernel at
    hop 1): the bytes read back and fed to the oracle give the engine's loss and gradients within the usual bounds,
    ``predict`` in train mode is the oracle's forward under the bytes of ITS draw, and two engines with one
    ``dropout_seed`` draw equal bytes at equal step."""
    drop = [0.5, 0.3]
    c = ne.fixture(ne.DEVICE_DROPOUT_CASE)._replace(drop=drop)
    eng = engine_of(c, "sgd", spmm, dropout_rng="device", dropout_seed=11)
    loss, grads = eng.backward_only(c.batch)
    masks = kept_masks(eng, drop)
    for m, p in zip(masks, drop):
        assert abs(m.mean() - (1 - p)) < 0.06, "keep rate"
    ref = ne.reference_of(c, masks=masks)
    assert_scalar_close(ref.loss32, ref.loss64, what="device dropout: the fp32 oracle's loss")
    assert_scalar_close(loss, ref.loss64, what="device dropout: loss")
    for k in ref.g64:
        floor = ref.terms.get(k, 0.0)
        assert_tensor_close(ref.g32[k], ref.g64[k], what=f"device dropout: the fp32 oracle's {k}", scale_floor=floor)
        assert_as_accurate_as_reference(grads[k].cpu().numpy(), ref.g32[k], ref.g64[k],
                                        what=f"device dropout: grad {k}", scale_floor=floor)
    users, items = c.batch[0], c.batch[1]
    scores = eng.model.predict(users, items).cpu().numpy()
    masks2 = kept_masks(eng, drop)
    assert not np.array_equal(masks2[0], masks[0]), "the next step draws other bytes"
    all2, _ = onp.ngcf_forward(c.w, c.adj, masks2, drop, dt=np.float64)
    assert_tensor_close(scores, (all2[users] * all2[c.U + items]).sum(1), what="device dropout: predict in train mode")
    twin = engine_of(c, "sgd", spmm, dropout_rng="device", dropout_seed=11)
    twin.backward_only(c.batch)
    for a, b in zip(kept_masks(twin, drop), masks):
        assert np.array_equal(a, b), "same seed, same step: same bytes"
    other = engine_of(c, "sgd", spmm, dropout_rng="device", dropout_seed=12)
    other.backward_only(c.batch)
    assert not np.array_equal(kept_masks(other, drop)[0], masks[0])


def test_limits(hip_device):
    """A hop width of 257 is refused by the library's plan check before anything is launched (the weights and the
    gradient buffer are as they were); seven hops are refused at construction; six run (test_width_chains[w16x7])."""
    from beta_recsys_amd._lib import HiprecError

    c = ne.fixture("n17")
    wide = make_engine(c.U, c.I, 16, [257, 16], [0.0, 0.0], "sgd", 0.05, 24, c.adj, c.decay)
    wide.model.train()
    before = wide.model.flat.clone()
    for call in (lambda: wide.backward_only(c.batch), lambda: wide.train_single_batch(c.batch),
                 lambda: wide.model(None), lambda: wide.model.predict(c.batch[0], c.batch[1])):
        with pytest.raises(HiprecError, match="hop width 257"):
            call()
    torch.cuda.synchronize()
    assert torch.equal(wide.model.flat, before), "the weights moved"
    assert float(wide._g_flat.abs().max()) == 0.0, "a gradient was written"
    with pytest.raises(ValueError):
        make_engine(c.U, c.I, 16, [16] * 7, [0.0] * 7, "sgd", 0.05, 24, c.adj, c.decay)
    six = ne.fixture("w16x7")
    assert len(six.dims) - 1 == ne.MAX_LAYERS
    check_backward(engine_of(six), six, ne.reference("w16x7"), "six hops after the refusals")


def test_older_forms_stay_correct(hip_device):
    """The three-launch forward hop and the per-hop backward at the shapes the fused kernels normally take:
    HIPREC_NGCF_UNFUSED_HOP, which only libhiprec_test.so (-DHIPREC_TEST_SWITCHES) reads (once per process: a fresh
    interpreter), under this file and the golden step test of tests/test_ngcf_gpu.py."""
    import os
    import subprocess
    import sys

    if os.environ.get("HIPREC_NGCF_UNFUSED_HOP"):
        pytest.skip("already running the older forms")
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run(
        [sys.executable, "-m", "pytest", os.path.join(here, "test_ngcf_edges_gpu.py"),
         os.path.join(here, "test_ngcf_gpu.py"), "-m", "gpu", "-x", "-q", "-k",
         "(step_matches_reference or edges) and not older_forms and not ml1m"],
        env=dict(os.environ, HIPREC_NGCF_UNFUSED_HOP="1", HIPREC_LIB="libhiprec_test.so"), capture_output=True,
        text=True, timeout=120)   # (the child takes 7 s on an MI355X)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "skipped" not in out.stdout.splitlines()[-1]
