"""The SimGCL restatement (tests/simgcl_numpy.py) against golden vectors captured from the real reference
(tests/golden/simgcl_*.npz, tools/gen_golden_simgcl.py): loss, gradients and optimizer steps on the recorded noise; that the
model is wired in; that shapes beyond a limit are refused.  CPU only."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

import simgcl_numpy as sx
from helpers import REL, assert_on_trajectory, assert_scalar_close, assert_sgd_exact, assert_step_close
from helpers import assert_tensor_close, copy_state, float64_oracle, load_golden, oracle_trajectory, to64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["simgcl_adam", "simgcl_sgd_hot_l3", "simgcl_rmsprop_d64_l1"]
KEYS = sx.KEYS


def sim_params(g, prefix):
    return {k: g[f"{prefix}/{k}"].astype(np.float32).copy() for k in KEYS}


def sim_meta(g):
    U, I, D, L, B, n_steps, seed = (int(x) for x in g["meta"])
    return dict(U=U, I=I, D=D, L=L, B=B, n_steps=n_steps, seed=seed)


def sim_hp(g, **over):
    eps, reg, lam, temp = (float(x) for x in g["hp"])
    return dict(dict(L=sim_meta(g)["L"], eps=eps, reg=reg, lam=lam, temp=temp, user_view="reference"), **over)


def sim_graph(g):
    m = sim_meta(g)
    return g["adj_row"], g["adj_col"], g["adj_val"], m["U"] + m["I"]


def sim_batch(g, s):
    return g["users"][s], g["pos"][s], g["neg"][s]


def sim_opt_state(g, step, opt):
    st = sx.new_opt_state(sim_params(g, "w0"), opt)
    st["step"] = step
    if step > 0 and opt == "adam":
        st["exp_avg"], st["exp_avg_sq"] = sim_params(g, f"m{step}"), sim_params(g, f"v{step}")
    elif step > 0 and opt == "rmsprop":
        st["square_avg"] = sim_params(g, f"v{step}")
    return st


def sim_band(w_prev, st_prev, g_ref, opt, lr, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel * its scale of g_ref (helpers.optimizer_band)."""
    outs = []
    for sign in (+1.0, -1.0):
        w = {k: v.copy() for k, v in w_prev.items()}
        st = copy_state(st_prev)
        gr = {k: (g_ref[k] + np.float32(sign * rel * float(np.abs(g_ref[k]).max()))).astype(np.float32) for k in KEYS}
        sx.opt_step(w, gr, st, opt, lr)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in KEYS}


def model_config(g, **over):
    m, hp = sim_meta(g), sim_hp(g)
    N = m["U"] + m["I"]
    adj = torch.sparse_coo_tensor(np.vstack([g["adj_row"], g["adj_col"]]), g["adj_val"], (N, N))
    cfg = dict(n_users=m["U"], n_items=m["I"], emb_dim=m["D"], n_layer=m["L"], eps=hp["eps"], reg=hp["reg"],
               batch_size=m["B"], norm_adj=adj, optimizer=str(g["optimizer"]), lr=float(g["lr"]), device_str="cpu")
    cfg["lambda"] = hp["lam"]
    cfg.update(over)
    return cfg


def make_engine(g, **over):
    import beta_recsys_amd as hp

    with contextlib.redirect_stdout(io.StringIO()):
        return hp.SimGCLEngine({"model": model_config(g, **over), "system": {"run_dir": "/tmp/hiprec_test_runs"}})


@pytest.mark.parametrize("case", CASES)
def test_every_step_in_isolation(case):
    g = load_golden(case)
    hp, graph, m = sim_hp(g), sim_graph(g), sim_meta(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    for s in range(m["n_steps"]):
        w0, st0 = sim_params(g, f"w{s}"), sim_opt_state(g, s, opt)
        parts, loss, grads = sx.simgcl_grads(w0, graph, hp, sim_batch(g, s), g["noise"][s])
        assert_scalar_close(loss, g["losses"][s], what=f"{case} loss step {s}")
        g_ref = sim_params(g, f"g{s + 1}")
        for k in KEYS:
            assert_tensor_close(grads[k], g_ref[k], what=f"{case} grad {k} step {s}")
        band = sim_band(w0, st0, g_ref, opt, lr)
        w1, st1 = {k: v.copy() for k, v in w0.items()}, copy_state(st0)
        sx.opt_step(w1, grads, st1, opt, lr)
        nxt = sim_opt_state(g, s + 1, opt)
        for k in KEYS:
            assert_step_close(w0[k], w1[k], g[f"w{s + 1}/{k}"], band[k], what=f"{case} weights {k} step {s}")
            for name in ("exp_avg", "exp_avg_sq", "square_avg"):
                if name in nxt:
                    assert_tensor_close(st1[name][k], nxt[name][k], REL if name == "exp_avg" else 2 * REL,
                                        f"{case} {name} {k} step {s}")


@pytest.mark.parametrize("case", CASES)
def test_chained_trajectory(case):
    g = load_golden(case)
    hp, graph, m = sim_hp(g), sim_graph(g), sim_meta(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])

    def grad_fn(w, s):
        return sx.simgcl_grads(w, graph, hp, sim_batch(g, s), g["noise"][s])[2]

    w0 = sim_params(g, "w0")
    w_ref, env, upd = oracle_trajectory(w0, list(range(m["n_steps"])), grad_fn,
                                        lambda w, gr, st: sx.opt_step(w, gr, st, opt, lr),
                                        lambda w: sx.new_opt_state(w, opt), trials=0 if opt == "sgd" else 8)
    ref_end = sim_params(g, f"w{m['n_steps']}")
    if opt == "sgd":
        assert_sgd_exact(w_ref, ref_end, w0, f"{case} final weights")
    else:
        assert_on_trajectory(w_ref, ref_end, env, upd, f"{case} trajectory")


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_and_reference_own_rounding(case):
    """The fp64 restatement reproduces the reference's own fp64 gradients (1e-9 of scale) and its loss, the recorded loss
    parts add up to it, and the reference's fp32 gradients lie within REL / 3 of the fp64 ones: the GPU test's bound --
    REL of scale plus twice that distance -- has room."""
    g = load_golden(case)
    hp, graph, m = sim_hp(g), sim_graph(g), sim_meta(g)
    for s in range(m["n_steps"]):
        with float64_oracle(sx):
            parts, l64, g64 = sx.simgcl_grads(to64(sim_params(g, f"w{s}")), graph, hp, sim_batch(g, s), g["noise"][s])
        assert g64[KEYS[0]].dtype == np.float64
        assert_scalar_close(l64, g["losses"][s], what=f"{case} loss step {s}")
        for got, ref in zip(parts, g["parts"][s]):
            assert_scalar_close(got, ref, 1e-9, what=f"{case} parts step {s}")
        assert_scalar_close(parts[0] + parts[1] + hp["lam"] * (parts[2] + parts[3]), l64, 1e-9)
        for k in KEYS:
            assert_tensor_close(g64[k], g[f"g64_{s + 1}/{k}"], 1e-9, f"{case} fp64 grad {k} step {s}")
            own = float(np.abs(g[f"g{s + 1}/{k}"] - g64[k]).max() / np.abs(g64[k]).max())
            assert own <= REL / 3, f"{case} step {s} {k}: the reference's own rounding is {own:.2e} of scale"


def test_hot_fixture_has_few_unique_ids():
    g = load_golden("simgcl_sgd_hot_l3")
    B = sim_meta(g)["B"]
    for s in range(3):
        assert len(set(g["users"][s])) <= 5 and len(set(g["pos"][s])) <= 7 and B == 64


def test_predict_reads_the_raw_tables():
    for case in CASES:
        g = load_golden(case)
        w = sim_params(g, f"w{sim_meta(g)['n_steps']}")
        assert_tensor_close(sx.simgcl_predict(w, g["predict_users"], g["predict_items"]), g["predict_scores"],
                            what=f"{case} predict")


def test_simgcl_is_wired_in():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib, compat, simgcl

    assert compat.MIRRORS["beta_rec.models.simgcl"] == "simgcl"
    assert simgcl.SimGCL is hp.SimGCL and simgcl.SimGCLEngine is hp.SimGCLEngine
    assert "simgcl.hip" in ge.EVIDENCE_GROUPS["simgcl"] and ge.evidence_group("simgcl_step") == "simgcl"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hiprec.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("hiprec_simgcl_plan_bytes", "hiprec_simgcl_ws_floats", "hiprec_simgcl_stamp_ints",
                 "hiprec_simgcl_batch_ws_floats", "hiprec_simgcl_noise", "hiprec_simgcl_predict", "hiprec_simgcl_grad",
                 "hiprec_simgcl_tile_b", "hiprec_simgcl_tile_n", "hiprec_simgcl_max_dim", "hiprec_simgcl_max_layers"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert (_lib.SIMGCL_TILE_B, _lib.SIMGCL_TILE_N) == (lib.hiprec_simgcl_tile_b(), lib.hiprec_simgcl_tile_n())
    assert (_lib.SIMGCL_MAX_DIM, _lib.SIMGCL_MAX_LAYERS) == (lib.hiprec_simgcl_max_dim(), lib.hiprec_simgcl_max_layers())
    assert sx.MAX_LAYERS == _lib.SIMGCL_MAX_LAYERS, "the restated draw keys (view, hop) with the library's stride"
    # one gradient table, no stored noise: seven [n, D] tables whatever L is
    assert lib.hiprec_simgcl_ws_floats(1000, 64) == 7 * 1000 * 64


def test_state_dict_and_initial_weights_are_the_references():
    """Same keys, and for the same torch seed the same N(0, 1) tables in the same order (simgcl.py:21-23)."""
    g = load_golden("simgcl_adam")
    torch.manual_seed(int(g["torch_seed"]))
    eng = make_engine(g)
    sd = eng.model.state_dict()
    assert list(sd) == list(KEYS)
    for k in KEYS:
        assert np.array_equal(sd[k].numpy(), g[f"w0/{k}"]), k
    assert eng.model.noise_seed == int(g["torch_seed"])


def test_shapes_beyond_a_limit_are_refused():
    """ValueError from Python before anything is allocated; the C entry points return an error code for the same shapes
    (no GPU is needed to be refused)."""
    import ctypes

    from beta_recsys_amd import _lib

    g = load_golden("simgcl_adam")
    for over, text in (({"emb_dim": 257}, "emb_dim"), ({"emb_dim": 0}, "emb_dim"), ({"n_layer": 0}, "n_layer"),
                       ({"n_layer": 5}, "n_layer"), ({"cl_temp": 0.0}, "cl_temp"), ({"user_view": "both"}, "user_view")):
        with pytest.raises(ValueError, match=text):
            make_engine(g, **over)
    lib = _lib.load()
    assert lib.hiprec_simgcl_noise(1, 0, 5, 10, 16, ctypes.c_void_p(8), None) != 0
    assert lib.hiprec_simgcl_noise(1, 0, 2, 10, 257, ctypes.c_void_p(8), None) != 0
    for dim, layers in ((257, 2), (16, 0), (16, 5)):
        p = _lib.SimgclPlan()
        p.n_users, p.n_items, p.dim, p.n_layers, p.e0 = 4, 6, dim, layers, 8
        assert lib.hiprec_simgcl_predict(ctypes.byref(p), None, None, 0, None, None, None) != 0
        with pytest.raises(_lib.HiprecError, match="supported"):
            _lib.check(lib.hiprec_simgcl_predict(ctypes.byref(p), None, None, 0, None, None, None))
