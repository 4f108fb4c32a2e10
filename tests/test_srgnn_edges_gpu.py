"""SR-GNN on the GPU over every fixture of srgnn_edges.py: loss, every gradient and the query against the float64
restatement, to the bound the project holds its sequence models to (``helpers.assert_grads_as_accurate``: 1e-5 of the
gradient's scale plus twice the float32 restatement's own error); the builder's arrays bit for bit against numpy; the
bits of two runs."""
import contextlib
import io

import numpy as np
import pytest
import torch

import srgnn_edges as se
from helpers import assert_grads_as_accurate, assert_scalar_close, assert_tensor_close

pytestmark = pytest.mark.gpu


def make_engine(f, optimizer="adam", lr=1e-3, l2=0.0, w=None, **extra):
    import beta_recsys_amd as hp

    model = {"hidden_size": f["H"], "step": f["step"], "nonhybrid": f["nonhybrid"], "l2": l2, "lr": lr,
             "batch_size": min(f["B"], se.LIMITS["batch"]), "optimizer": optimizer, "device_str": "cuda:0"}
    model.update(extra)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.SRGNNEngine({"model": model, "dataset": {"n_node": f["n_node"]},
                              "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    load_weights(eng, f["w"] if w is None else w)
    return eng


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


@pytest.mark.parametrize("name", se.NAMES)
def test_fixture_against_the_restatement(hip_device, name):
    f = se.fixture(name)
    l64, g64, q64, _, _, g32 = se.reference(name)
    eng = make_engine(f)
    loss, grads = eng.backward_only(se.batch_of(f))
    grads = {k: v.cpu().numpy() for k, v in grads.items()}
    print(f"{name}: loss {loss!r} vs exact {l64!r}")
    for k in g64:
        print(f"  grad {k}: err vs exact {np.abs(grads[k].reshape(g64[k].shape) - g64[k]).max():.3e}, fp32 restatement's "
              f"{np.abs(g32[k] - g64[k]).max():.3e}, scale {np.abs(g64[k]).max():.3e}")
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())
    assert_scalar_close(loss, l64, what="loss")
    assert_grads_as_accurate(grads, g32, g64, what="grad")
    assert float(eng._g_flat.abs().max()) == 0.0
    assert float(np.abs(grads["embedding.weight"][0]).max()) == 0.0, "the padding row holds a gradient"
    if f["nonhybrid"]:
        assert not grads["linear_transform.weight"].any() and not grads["linear_transform.bias"].any()
    eng.model.eval()
    query = eng.model.query(f["seq"], f["lens"])
    assert_tensor_close(query.cpu().numpy(), q64, what="query")


@pytest.mark.parametrize("name", se.BUILDER)
def test_the_builder_is_bit_exact(hip_device, name):
    f = se.fixture(name)
    eng = make_engine(f)
    got = eng.model.graph(f["seq"], f["lens"])
    want = se.numpy_graph(f)
    from beta_recsys_amd.srgnn import GRAPH_FIELDS

    assert tuple(got) == GRAPH_FIELDS == tuple(want)
    for k in GRAPH_FIELDS:
        g = got[k].cpu().numpy()
        assert g.dtype == np.int32 and g.shape == want[k].shape, k
        assert np.array_equal(g, want[k]), f"{name}: {k} differs from the numpy restatement"


@pytest.mark.parametrize("name", se.SAME_BITS)
def test_gradients_are_the_same_bits_from_run_to_run(hip_device, name):
    """Every gradient but embedding.weight's (row atomics) is bit-identical between two calls, and so are the loss and
    the query."""
    f = se.fixture(name)
    eng = make_engine(f)
    l1, g1 = eng.backward_only(se.batch_of(f))
    q1 = eng.model.query(f["seq"], f["lens"]).clone()
    l2, g2 = eng.backward_only(se.batch_of(f))
    q2 = eng.model.query(f["seq"], f["lens"])
    assert l1 == l2 and torch.equal(q1, q2)
    for k in g1:
        if k != "embedding.weight":
            assert torch.equal(g1[k], g2[k]), f"grad {k} differs between two runs"
