"""BUIR's kernels at their tile edges (tests/buir_edges.py) against the fp64 restatement, with no allowance for a
reference's rounding: the loss to REL, every gradient to REL of its scale, all finite; the all-zero target rows; and the
moving target over 20 steps."""
import contextlib
import io

import numpy as np
import pytest
import torch

import buir_edges as edges
import buir_numpy as bx
from helpers import EPS32, assert_scalar_close, assert_tensor_close, float64_oracle, to64

pytestmark = pytest.mark.gpu
TRAINABLE = bx.TRAINABLE


def engine_of(c, **over):
    import beta_recsys_amd as hp

    rows, cols, vals, N = c["graph"]
    adj = torch.sparse_coo_tensor(np.vstack([rows, cols]), vals, (N, N))
    cfg = dict(n_users=c["U"], n_items=c["I"], emb_dim=c["D"], n_layers=c["L"], momentum=0.9, norm_adj=adj,
               batch_size=c["B"], optimizer="sgd", lr=0.05, device_str="cuda:0")
    cfg.update(over)
    with contextlib.redirect_stdout(io.StringIO()):
        return hp.BUIREngine({"model": cfg, "system": {"run_dir": "/tmp/hiprec_test_runs"}})


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def test_tile_is_the_librarys(hip_device):
    from beta_recsys_amd import _lib

    assert edges.TB == _lib.load().hiprec_buir_tile_b() == _lib.BUIR_TILE_B


@pytest.mark.parametrize("name", list(edges.CASES))
def test_edge_case_matches_fp64(hip_device, name):
    c = edges.build(name)
    with float64_oracle(bx):
        l64, g64 = bx.buir_grads(to64(c["w"]), c["graph"], c["L"], c["batch"])
        # D = 1: n(y) = +-1 whatever y is, the exact gradient is 0 and an fp32 one is rounding error of its terms
        floor = bx.term_scale(to64(c["w"]), c["graph"], c["L"], c["batch"]) if c["D"] == 1 else {}
    eng = engine_of(c)
    load_weights(eng, c["w"])
    loss, grads = eng.backward_only(c["batch"])
    print(f"{name}: loss {loss!r} vs {l64!r}")
    assert_scalar_close(loss, l64, what=f"{name} loss")
    assert set(grads) == set(TRAINABLE)
    for k in TRAINABLE:
        g = grads[k].cpu().numpy()
        assert np.isfinite(g).all(), f"{name}: NaN in grad {k}"
        print(f"  grad {k}: err {np.abs(g - g64[k]).max():.3e} of scale {max(np.abs(g64[k]).max(), floor.get(k, 0.0)):.3e}")
        assert_tensor_close(g, g64[k], what=f"{name} grad {k}", scale_floor=floor.get(k, 0.0))
    assert float(eng._g_flat.abs().max()) == 0.0
    # a second call gives the same loss: nothing of a step is left behind in the workspace
    assert_scalar_close(eng.backward_only(c["batch"])[0], l64, what=f"{name} loss, again")


def test_zero_target_rows_cost_exactly_two_and_add_no_gradient(hip_device):
    """A pair whose two target rows are all zero: n(t) = 0 / max(0, 1e-12) = 0, both cosines are 0, the loss is exactly
    4 and no gradient is produced anywhere."""
    c = edges.build("d100_l1_zero_target")
    eng = engine_of(c)
    load_weights(eng, c["w"])
    for B in (1, edges.TB + 1):
        batch = (np.full(B, c["U"] - 1), np.full(B, c["I"] - 1), np.zeros(B, dtype=np.int64))
        loss, grads = eng.backward_only(batch)
        if B == 1:
            assert loss == 4.0, loss           # one pair: (2 - 0) + (2 - 0), nothing rounds
        assert_scalar_close(loss, 4.0, what=f"{B} zero-target pairs")
        for k in TRAINABLE:
            assert not grads[k].cpu().numpy().any(), k


def test_moving_target_over_twenty_steps(hip_device):
    """update_target on: after every step the raw target is the restated moving average of the device's own previous
    target and new online tables -- two products and a sum, so within 2 ulp of the largest element whatever the device
    fuses --, the trained tensors moved, and after 20 steps ``pooled_target()``, which was only ever updated from pooled
    online rows, is the fp64 pool of the raw target to REL."""
    c = edges.build("d16_l2_three_blocks")
    eng = engine_of(c, update_target=True)
    load_weights(eng, c["w"])
    rng = np.random.default_rng(3)
    w_prev = get_weights(eng)
    for s in range(20):
        B = (1, edges.TB, c["B"])[s % 3]
        batch = (rng.integers(0, c["U"], B), rng.integers(0, c["I"], B), rng.integers(0, c["I"], B))
        assert np.isfinite(eng.train_single_batch(batch))
        w_now = get_weights(eng)
        want = {k: v.copy() for k, v in w_prev.items()}
        for k in bx.ONLINE:
            want[k] = w_now[k]
        bx.ema(want, 0.9)
        for o, t in zip(bx.ONLINE, bx.TARGET):
            assert np.abs(w_now[o] - w_prev[o]).max() > 0
            assert np.abs(w_now[t] - want[t]).max() <= 2 * EPS32 * np.abs(want[t]).max(), f"step {s} {t}"
        w_prev = w_now
    with float64_oracle(bx):
        P = bx.pooled(bx.tables(to64(w_prev), bx.TARGET), bx.dense_adj(c["graph"]), c["L"])
    assert_tensor_close(eng.pooled_target().cpu().numpy(), P, what="pooled target after 20 moving steps")
    # ... and the step that follows reads exactly that table
    batch = c["batch"]
    with float64_oracle(bx):
        l64, g64 = bx.buir_grads(to64(w_prev), c["graph"], c["L"], batch)
    loss, grads = eng.backward_only(batch)
    assert_scalar_close(loss, l64, what="loss on the moved target")
    for k in TRAINABLE:
        assert_tensor_close(grads[k].cpu().numpy(), g64[k], what=f"grad {k} on the moved target")
