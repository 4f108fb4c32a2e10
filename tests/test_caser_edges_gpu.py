"""Caser on the GPU over every fixture of caser_edges.py: loss, every gradient (with the l2 term) and the query vector
against the float64 restatement, to the bound the project holds its sequence models to
(``helpers.assert_grads_as_accurate``: 1e-5 of the gradient's scale plus twice the float32 restatement's own error)."""
import contextlib
import io

import numpy as np
import pytest
import torch

import caser_edges as ce
import caser_torch as ct
from helpers import assert_grads_as_accurate, assert_scalar_close, assert_tensor_close

pytestmark = pytest.mark.gpu


def make_engine(f, optimizer="adam", lr=1e-3, w=None, **extra):
    import beta_recsys_amd as hp

    model = {"n_users": f["U"], "n_items": f["I"], "emb_dim": f["d"], "L": f["L"], "T": f["T"], "neg_samples": f["N"],
             "n_v": f["n_v"], "n_h": f["n_h"], "ac_conv": f["ac_conv"], "ac_fc": f["ac_fc"], "dropout_rate": f["p"],
             "l2": f["l2"], "lr": lr, "optimizer": optimizer, "batch_size": f["B"], "device_str": "cuda:0"}
    model.update(extra)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.CaserEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    load_weights(eng, f["w"] if w is None else w)
    return eng


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def np_grads(grads):
    return {k: v.cpu().numpy() for k, v in grads.items()}


def untouched_rows(f):
    """Per table the rows no id of the batch names."""
    used = {"user_embeddings.weight": f["users"], "item_embeddings.weight": f["seq"],
            "W2.weight": np.concatenate([f["pos"].reshape(-1), f["neg"].reshape(-1)])}
    used["b2.weight"] = used["W2.weight"]
    out = {}
    for k, ids in used.items():
        ids = np.unique(ids)
        if k != "user_embeddings.weight":
            ids = ids[ids != 0]                      # 0 names no row: the padding rows are untouched
        out[k] = np.setdiff1d(np.arange(f["w"][k].shape[0]), ids)
    return out


@pytest.mark.parametrize("name", ce.NAMES)
def test_fixture_against_the_restatement(hip_device, name):
    f = ce.fixture(name)
    l64, g64, _, g32 = ce.reference(name)
    eng = make_engine(f)
    loss, grads = eng.backward_only(ce.batch_of(f), keep_masks=ce.keep_of(f))
    grads = np_grads(grads)
    print(f"{name}: loss {loss!r} vs exact {l64!r}")
    for k in g64:
        print(f"  grad {k}: err vs exact {np.abs(grads[k].reshape(g64[k].shape) - g64[k]).max():.3e}, fp32 restatement's "
              f"{np.abs(g32[k] - g64[k]).max():.3e}, scale {np.abs(g64[k]).max():.3e}")
    assert np.isfinite(loss) and all(np.isfinite(g).all() for g in grads.values())
    assert_scalar_close(loss, l64, what="loss")
    assert_grads_as_accurate(grads, g32, g64, what="grad")
    assert float(np.abs(grads["item_embeddings.weight"][0]).max()) == 0.0, "a gradient reached the padding row"
    assert float(eng._g_flat.abs().max()) == 0.0
    # a table row that no id names receives exactly l2 * w
    l2 = np.float32(f["l2"])
    for k, rows in untouched_rows(f).items():
        assert rows.size, f"{k}: the fixture touches every row"
        assert np.array_equal(grads[k][rows], l2 * f["w"][k][rows]), f"{k}: an untouched row holds more than l2 * w"
    # the query vector in eval mode
    if not f["p"]:
        x = eng.model.query(f["seq"], f["users"]).cpu().numpy()
        assert_tensor_close(x, ct.query(f["w"], f["seq"], f["users"], f["ac_conv"], f["ac_fc"]), what="query")


def test_rows_without_a_real_target_add_nothing(hip_device):
    """padding's last row has only 0 targets: without it the loss and every gradient but the tables' are the same
    bits (its sequence and user are never reached by a gradient)."""
    f = ce.fixture("padding")
    eng = make_engine(f)
    loss, grads = eng.backward_only(ce.batch_of(f))
    short, g_short = eng.backward_only(tuple(a[:-1] for a in ce.batch_of(f)))
    assert short == loss
    for k in grads:
        if k not in ct.TABLES:
            assert torch.equal(grads[k], g_short[k]), f"the row without a target moved grad {k}"


@pytest.mark.parametrize("name", ["defaults", "limits", "repeats", "dropout", "slabs", "tile_edges_4097"])
def test_gradients_are_the_same_bits_from_run_to_run(hip_device, name):
    """Every gradient but the three tables' (user_embeddings, item_embeddings, W2 / b2: row atomics) is bit-identical
    between two calls, and so are the tables' untouched rows."""
    f = ce.fixture(name)
    eng = make_engine(f)
    l1, g1 = eng.backward_only(ce.batch_of(f), keep_masks=ce.keep_of(f))
    l2, g2 = eng.backward_only(ce.batch_of(f), keep_masks=ce.keep_of(f))
    assert l1 == l2
    for k in g1:
        if k not in ct.TABLES:
            assert torch.equal(g1[k], g2[k]), f"grad {k} differs between two runs"
    for k, rows in untouched_rows(f).items():
        rows = torch.from_numpy(rows).cuda()
        assert torch.equal(g1[k][rows], g2[k][rows])


def test_the_keep_mask_is_checked(hip_device):
    f = ce.fixture("dropout")
    eng = make_engine(f)
    l64 = ce.reference("dropout")[0]
    plain = ct.grads(f["w"], f["seq"], f["users"], f["pos"], f["neg"], f["ac_conv"], f["ac_fc"], f["l2"])[0]
    assert abs(l64 - plain) > 1e-3 * abs(l64), "the mask did nothing"
    with pytest.raises(ValueError):
        eng.backward_only(ce.batch_of(f), keep_masks=[f["keep"][:, :-1]])
    with pytest.raises(ValueError):
        eng.backward_only(ce.batch_of(f), keep_masks=[f["keep"], f["keep"]])
    eng.model.eval()
    loss_eval, _ = eng.backward_only(ce.batch_of(f), keep_masks=ce.keep_of(f))
    assert eng.last_keep_masks is None
    assert_scalar_close(loss_eval, plain, what="eval mode ignores the mask")
