"""SimGCL's kernels at their tile edges (tests/simgcl_edges.py) against the fp64 restatement, with no allowance for a
reference's rounding: loss parts to REL (an InfoNCE part to REL x max(|part|, n_uniq)), gradients to REL of their scale."""
import contextlib
import io

import numpy as np
import pytest
import torch

import simgcl_edges as edges
import simgcl_numpy as sx
from helpers import assert_scalar_close, assert_tensor_close, float64_oracle, to64
from test_simgcl_gpu import assert_parts_close, load_weights

pytestmark = pytest.mark.gpu
KEYS = sx.KEYS


def engine_of(c):
    import beta_recsys_amd as hp

    rows, cols, vals, N = c["graph"]
    adj = torch.sparse_coo_tensor(np.vstack([rows, cols]), vals, (N, N))
    h = c["hp"]
    cfg = dict(n_users=c["U"], n_items=c["I"], emb_dim=c["D"], n_layer=h["L"], eps=h["eps"], reg=h["reg"], norm_adj=adj,
               batch_size=c["batch"][0].size, optimizer="sgd", lr=0.01, device_str="cuda:0", cl_temp=h["temp"],
               user_view=h["user_view"])
    cfg["lambda"] = h["lam"]
    with contextlib.redirect_stdout(io.StringIO()):
        return hp.SimGCLEngine({"model": cfg, "system": {"run_dir": "/tmp/hiprec_test_runs"}})


def test_tiles_are_the_librarys(hip_device):
    from beta_recsys_amd import _lib

    lib = _lib.load()
    assert (edges.TB, edges.TN) == (lib.hiprec_simgcl_tile_b(), lib.hiprec_simgcl_tile_n())


@pytest.mark.parametrize("name", list(edges.CASES))
def test_edge_case_matches_fp64(hip_device, name):
    c = edges.build(name)
    with float64_oracle(sx):
        parts, l64, g64 = sx.simgcl_grads(to64(c["w"]), c["graph"], c["hp"], c["batch"], c["noise"])
    eng = engine_of(c)
    load_weights(eng, c["w"])
    loss, grads = eng.backward_only(c["batch"], noise=c["noise"])
    got = eng.last_losses()
    print(f"{name}: loss {loss!r} vs {l64!r}; n_uniq {c['n_uniq']}")
    assert_parts_close(got, parts, c["batch"], name, row_floor=True)
    lam = c["hp"]["lam"]
    floor = lam * sum(max(abs(p), n) for p, n in zip(parts[2:], c["n_uniq"]))
    assert abs(loss - l64) <= 1e-5 * (abs(parts[0]) + abs(parts[1]) + floor), f"{name} loss: got {loss!r}, fp64 {l64!r}"
    for k in KEYS:
        g = grads[k].cpu().numpy()
        assert np.isfinite(g).all(), f"{name}: NaN in grad {k}"
        print(f"  grad {k}: err {np.abs(g - g64[k]).max():.3e} of scale {np.abs(g64[k]).max():.3e}")
        assert_tensor_close(g, g64[k], what=f"{name} grad {k}")
    if c["n_uniq"][0] == 1:
        assert abs(got[2]) <= 1e-5, "one unique user: the InfoNCE part is 0"
