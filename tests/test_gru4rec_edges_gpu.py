"""GRU4Rec on the GPU over every fixture of gru4rec_edges.py: loss, every gradient and the stored state against the
float64 restatement, to the bound the project holds its sequence models to (``helpers.assert_grads_as_accurate``: 1e-5
of the gradient's scale plus twice the float32 restatement's own error)."""
import contextlib
import io

import numpy as np
import pytest
import torch

import gru4rec_edges as ge
import gru4rec_torch as gt
from helpers import assert_grads_as_accurate, assert_scalar_close, assert_tensor_close

pytestmark = pytest.mark.gpu


def make_engine(f, optimizer="adam", lr=1e-3, w=None, **extra):
    import beta_recsys_amd as hp

    model = {"layers": list(f["layers"]), "constrained_embedding": not f["D"], "embedding": f["D"], "loss": f["loss"],
             "bpreg": f["bpreg"], "elu_param": f["elu"], "logq": f["logq"], "n_sample": f["S"], "sample_alpha": f["alpha"],
             "dropout_p_embed": f["pe"], "dropout_p_hidden": f["ph"], "batch_size": f["B"], "lr": lr,
             "optimizer": optimizer, "device_str": "cuda:0"}
    model.update(extra)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.GRU4RecEngine({"model": model, "dataset": {"n_items": f["I"]},
                                "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    load_weights(eng, f["w"] if w is None else w)
    eng.set_item_probs(f["p"])
    return eng


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def load_state(eng, state):
    for mine, s in zip(eng.model.reset_state(len(state[0])), state):
        mine.copy_(torch.from_numpy(np.asarray(s, dtype=np.float32)))


def get_state(eng):
    return [s.cpu().numpy() for s in eng.model.state]


def run_fixture(eng, f):
    load_state(eng, f["state"])
    return eng.backward_only(ge.batch_of(f), keep_masks=f["keeps"])


@pytest.mark.parametrize("name", ge.NAMES)
def test_fixture_against_the_restatement(hip_device, name):
    f = ge.fixture(name)
    l64, g64, s64, _, g32 = ge.reference(name)
    eng = make_engine(f)
    loss, grads = run_fixture(eng, f)
    grads = {k: v.cpu().numpy() for k, v in grads.items()}
    print(f"{name}: loss {loss!r} vs exact {l64!r}")
    for k in g64:
        print(f"  grad {k}: err vs exact {np.abs(grads[k].reshape(g64[k].shape) - g64[k]).max():.3e}, fp32 restatement's "
              f"{np.abs(g32[k] - g64[k]).max():.3e}, scale {np.abs(g64[k]).max():.3e}")
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())
    assert_scalar_close(loss, l64, what="loss")
    assert_grads_as_accurate(grads, g32, g64, what="grad")
    assert float(eng._g_flat.abs().max()) == 0.0
    for k, rows in ge.untouched_rows(f).items():
        assert rows.size and float(np.abs(grads[k][rows]).max()) == 0.0, f"{k}: a row that no id names holds a gradient"
    for l, (got, want) in enumerate(zip(get_state(eng), s64)):
        assert_tensor_close(got, want, what=f"stored state of layer {l}")


@pytest.mark.parametrize("name", ["defaults", "limits", "stacked", "repeats", "dropout", "logq", "tile_edges_B_129",
                                  "max_batch"])
def test_gradients_are_the_same_bits_from_run_to_run(hip_device, name):
    """Every gradient but the tables' (Wy, By, E: row atomics) is bit-identical between two calls, and so are the loss
    and the stored state."""
    f = ge.fixture(name)
    eng = make_engine(f)
    l1, g1 = run_fixture(eng, f)
    s1 = [s.clone() for s in eng.model.state]
    l2, g2 = run_fixture(eng, f)
    assert l1 == l2
    for k in g1:
        if k not in gt.TABLES:
            assert torch.equal(g1[k], g2[k]), f"grad {k} differs between two runs"
    for a, b in zip(s1, eng.model.state):
        assert torch.equal(a, b)


def test_the_keep_masks_are_checked(hip_device):
    f = ge.fixture("dropout")
    eng = make_engine(f)
    l64 = ge.reference("dropout")[0]
    plain = gt.grads(f["w"], ge.cfg_of(f), ge.batch_of(f), f["state"], None)[0]
    assert abs(l64 - plain) > 1e-3 * abs(l64), "the masks did nothing"
    load_state(eng, f["state"])
    with pytest.raises(ValueError):
        eng.backward_only(ge.batch_of(f), keep_masks=f["keeps"][:2])
    with pytest.raises(ValueError):
        eng.backward_only(ge.batch_of(f), keep_masks=[f["keeps"][0][:, :-1]] + f["keeps"][1:])
    with pytest.raises(ValueError):
        eng.backward_only(ge.batch_of(f), keep_masks=[f["keeps"][0], None, f["keeps"][2]])
    eng.model.eval()
    load_state(eng, f["state"])
    loss_eval, _ = eng.backward_only(ge.batch_of(f), keep_masks=f["keeps"])
    assert eng.last_keep_masks is None
    assert_scalar_close(loss_eval, plain, what="eval mode ignores the masks")


def test_a_step_needs_a_negative_and_fits_the_limits(hip_device):
    f = ge.fixture("tiny")
    eng = make_engine(f)
    with pytest.raises(ValueError):
        eng.backward_only((f["in_items"], f["targets"], f["reset"], f["samples"][:0]))      # N = 1
    with pytest.raises(ValueError):
        eng.backward_only((f["in_items"], f["targets"], f["reset"], np.zeros(ge.LIMITS["n_sample"] + 1, dtype=np.int64)))
    with pytest.raises(ValueError):
        eng.model.step(np.zeros(ge.LIMITS["batch"] + 1, dtype=np.int64))
    loss, _ = run_fixture(eng, f)
    assert_scalar_close(loss, ge.reference("tiny")[0], what="loss after the errors")
