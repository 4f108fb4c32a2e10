"""The SGL restatement (tests/sgl_numpy.py) against golden vectors captured from the real reference
(tests/golden/sgl_*.npz, tools/gen_golden_sgl.py): its sub-graphs, loss parts, gradients and optimizer steps.  CPU only."""
import os
import re
import sys

import numpy as np
import pytest

import sgl_numpy as sx
from helpers import REL, assert_on_trajectory, assert_scalar_close, assert_sgd_exact, assert_step_close
from helpers import assert_tensor_close, copy_state, float64_oracle, load_golden, oracle_trajectory, to64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["sgl_both_edge_adam", "sgl_user_walk_sgd", "sgl_item_edge_rmsprop", "sgl_pretrain_adam", "sgl_hot_sgd",
         "sgl_refresh_walk_adam"]
KEYS = sx.KEYS


def sgl_params(g, prefix):
    return {k: g[f"{prefix}/{k}"].astype(np.float32).copy() for k in KEYS}


def sgl_meta(g):
    U, I, D, L, B, n_steps, seed, aug_type, pretrain = (int(x) for x in g["meta"])
    return dict(U=U, I=I, D=D, L=L, B=B, n_steps=n_steps, seed=seed, aug_type=aug_type, pretrain=pretrain)


def sgl_hp(g):
    m = sgl_meta(g)
    regs, ssl_reg, ssl_temp, ssl_ratio = (float(x) for x in g["hp"])
    return dict(L=m["L"], regs=regs, ssl_reg=ssl_reg, ssl_temp=ssl_temp, ssl_mode=str(g["ssl_mode"]), ssl_ratio=ssl_ratio,
                pretrain=m["pretrain"], aug_type=m["aug_type"])


def sgl_graph(g):
    m = sgl_meta(g)
    return g["adj_row"], g["adj_col"], g["adj_val"], m["U"] + m["I"]


def sgl_batch(g, s):
    return g["users"][s], g["pos"][s], g["neg"][s]


def sub_name(aug_type, v, l):
    return "sub%d" % (v + 1) + ("%d" % (l + 1) if aug_type == 2 else "")


def n_refreshes(g):
    return int(g["refresh_of_step"].max()) + 1


def recorded_coo(g, r, v, l):
    """The reference's sub-matrix of refresh r, view v, layer l: ``(rows, cols, vals)``."""
    nm = sub_name(sgl_meta(g)["aug_type"], v, l)
    idx = g[f"sub{r}/{nm}/idx"].astype(np.int64)
    return idx[0], idx[1], g[f"sub{r}/{nm}/val"]


def recorded_subs(g, r, dtype=np.float32):
    """``[view][layer]`` dense matrices of refresh r from the reference's recorded sub-matrices."""
    m = sgl_meta(g)
    N = m["U"] + m["I"]
    out = []
    for v in range(2):
        mats = []
        for l in range(max(m["L"], 1)):
            rows, cols, vals = recorded_coo(g, r, v, l)
            A = np.zeros((N, N), dtype=dtype)
            A[rows, cols] = vals
            mats.append(A)
        out.append(mats)
    return out


def reference_dict(g, r):
    """The reference's own ``sub_mat`` dict of refresh r, as its ``sub_mat_refresher`` returns it."""
    m = sgl_meta(g)
    N = m["U"] + m["I"]
    d = {}
    for v in range(2):
        for l in range(max(m["L"], 1) if m["aug_type"] == 2 else 1):
            nm = sub_name(m["aug_type"], v, l)
            d["adj_indices_" + nm] = np.asmatrix(g[f"sub{r}/{nm}/idx"])
            d["adj_values_" + nm] = g[f"sub{r}/{nm}/val"]
            d["adj_shape_" + nm] = (N, N)
    return d


def replayed_keeps(g):
    """The keep sets of every refresh, replayed from the fixture's numpy seed in the reference's call order."""
    m, hp = sgl_meta(g), sgl_hp(g)
    np.random.seed(int(g["numpy_seed"]))
    return [sx.keep_sets(g["inter_user"].size, m["U"], m["I"], m["aug_type"], hp["ssl_ratio"], m["L"])
            for _ in range(n_refreshes(g))]


def sgl_opt_state(g, step, opt):
    st = sx.new_opt_state(sgl_params(g, "w0"), opt)
    st["step"] = step
    if step > 0 and opt == "adam":
        st["exp_avg"], st["exp_avg_sq"] = sgl_params(g, f"m{step}"), sgl_params(g, f"v{step}")
    elif step > 0 and opt == "rmsprop":
        st["square_avg"] = sgl_params(g, f"v{step}")
    return st


def sgl_band(w_prev, st_prev, g_ref, opt, lr, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel * its scale of g_ref (helpers.optimizer_band)."""
    outs = []
    for sign in (+1.0, -1.0):
        w = {k: v.copy() for k, v in w_prev.items()}
        st = copy_state(st_prev)
        gr = {k: (g_ref[k] + np.float32(sign * rel * float(np.abs(g_ref[k]).max()))).astype(np.float32) for k in KEYS}
        sx.opt_step(w, gr, st, opt, lr)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in KEYS}


@pytest.mark.parametrize("case", CASES)
def test_every_step_in_isolation(case):
    g = load_golden(case)
    hp, graph, m = sgl_hp(g), sgl_graph(g), sgl_meta(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    for s in range(m["n_steps"]):
        subs = recorded_subs(g, int(g["refresh_of_step"][s]))
        w0, st0 = sgl_params(g, f"w{s}"), sgl_opt_state(g, s, opt)
        parts, loss, grads = sx.sgl_grads(w0, graph, subs, hp, sgl_batch(g, s))
        assert_scalar_close(loss, g["losses"][s], what=f"{case} loss step {s}")
        for got, ref, name in zip(parts, g["parts"][s], ("bpr", "emb", "ssl")):
            assert_scalar_close(got, ref, what=f"{case} {name} step {s}")
        g_ref = sgl_params(g, f"g{s + 1}")
        for k in KEYS:
            assert_tensor_close(grads[k], g_ref[k], what=f"{case} grad {k} step {s}")
        band = sgl_band(w0, st0, g_ref, opt, lr)
        w1, st1 = {k: v.copy() for k, v in w0.items()}, copy_state(st0)
        sx.opt_step(w1, grads, st1, opt, lr)
        nxt = sgl_opt_state(g, s + 1, opt)
        for k in KEYS:
            assert_step_close(w0[k], w1[k], g[f"w{s + 1}/{k}"], band[k], what=f"{case} weights {k} step {s}")
            for name in ("exp_avg", "exp_avg_sq", "square_avg"):
                if name in nxt:
                    assert_tensor_close(st1[name][k], nxt[name][k], REL if name == "exp_avg" else 2 * REL,
                                        f"{case} {name} {k} step {s}")


@pytest.mark.parametrize("case", ["sgl_both_edge_adam", "sgl_user_walk_sgd", "sgl_refresh_walk_adam"])
def test_chained_trajectory(case):
    g = load_golden(case)
    hp, graph, m = sgl_hp(g), sgl_graph(g), sgl_meta(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    subs = [recorded_subs(g, r) for r in range(n_refreshes(g))]

    def grad_fn(w, s):
        return sx.sgl_grads(w, graph, subs[int(g["refresh_of_step"][s])], hp, sgl_batch(g, s))[2]

    w0 = sgl_params(g, "w0")
    w_ref, env, upd = oracle_trajectory(w0, list(range(m["n_steps"])), grad_fn,
                                        lambda w, gr, st: sx.opt_step(w, gr, st, opt, lr),
                                        lambda w: sx.new_opt_state(w, opt), trials=0 if opt == "sgd" else 8)
    ref_end = sgl_params(g, f"w{m['n_steps']}")
    if opt == "sgd":
        assert_sgd_exact(w_ref, ref_end, w0, f"{case} final weights")
    else:
        assert_on_trajectory(w_ref, ref_end, env, upd, f"{case} trajectory")


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_and_reference_own_rounding(case):
    """The fp64 restatement reproduces the reference's own fp64 gradients (1e-9 of scale), and the reference's fp32
    gradients lie within REL / 3 of them: the GPU test's bound -- REL of scale plus twice that distance -- has room."""
    g = load_golden(case)
    hp, graph, m = sgl_hp(g), sgl_graph(g), sgl_meta(g)
    for s in range(m["n_steps"]):
        with float64_oracle(sx):
            subs = recorded_subs(g, int(g["refresh_of_step"][s]), np.float64)
            _, l64, g64 = sx.sgl_grads(to64(sgl_params(g, f"w{s}")), graph, subs, hp, sgl_batch(g, s))
        assert g64[KEYS[0]].dtype == np.float64
        assert_scalar_close(l64, g["losses"][s], what=f"{case} loss step {s}")
        for k in KEYS:
            assert_tensor_close(g64[k], g[f"g64_{s + 1}/{k}"], 1e-9, f"{case} fp64 grad {k} step {s}")
            own = float(np.abs(g[f"g{s + 1}/{k}"] - g64[k]).max() / np.abs(g64[k]).max())
            assert own <= REL / 3, f"{case} step {s} {k}: the reference's own rounding is {own:.2e} of scale"


@pytest.mark.parametrize("case", CASES)
def test_numpy_replay_gives_the_references_kept_sets_and_values(case):
    """The same ``np.random.seed``, drawn in the reference's order (view 1 then view 2, per layer for the random walk),
    keeps exactly the interactions its sub-matrices hold; the restated values match the recorded ones at rtol 1e-6
    (three fp32 roundings of 1.2e-7 each -- the power and two products -- rounded up)."""
    g = load_golden(case)
    m = sgl_meta(g)
    eu, ei = g["inter_user"], g["inter_item"]
    keeps = replayed_keeps(g)
    isolated = 0
    for r in range(n_refreshes(g)):
        for v in range(2):
            for l in range(max(m["L"], 1)):
                rows, cols, vals = recorded_coo(g, r, v, l)
                keep = keeps[r][v][l]
                on = keep != 0
                want = {(u, m["U"] + i) for u, i in zip(eu[on], ei[on])}
                want |= {(c, r_) for r_, c in want}
                assert set(zip(rows.tolist(), cols.tolist())) == want, f"{case} refresh {r} view {v} layer {l}"
                A = sx.sub_matrix(eu, ei, m["U"], m["I"], keep)
                np.testing.assert_allclose(A[rows, cols], vals, rtol=1e-6, atol=0)
                assert np.count_nonzero(A) == vals.size
                isolated += int((A.sum(axis=1) == 0).sum())
        if m["aug_type"] == 2 and m["L"] > 1:
            assert not np.array_equal(keeps[r][0][0], keeps[r][0][1]), "two layers drew the same walk"
        else:
            assert keeps[r][0][0] is keeps[r][0][-1]
        assert not np.array_equal(keeps[r][0][0], keeps[r][1][0]), "the two views drew the same set"
    if case == "sgl_both_edge_adam":
        assert isolated > 0, "no node is isolated by the dropout in this fixture"


def test_hot_fixture_repeats_one_user_and_one_item():
    g = load_golden("sgl_hot_sgd")
    B = sgl_meta(g)["B"]
    for s in range(3):
        assert len(set(g["users"][s][: B // 2])) == 1 and len(set(g["pos"][s][: B // 2])) == 1


def test_predict_is_the_reference_on_the_weights_it_last_propagated():
    """The reference's predict reads the tables of its last training forward -- the weights BEFORE the last step; the
    restatement on those weights reproduces it, and the restatement on the final weights (what the mirror returns)
    differs: the deviation INTEGRATION records."""
    for case in CASES:
        g = load_golden(case)
        hp, graph, m = sgl_hp(g), sgl_graph(g), sgl_meta(g)
        stale = sx.sgl_predict(sgl_params(g, f"w{m['n_steps'] - 1}"), graph, hp, g["predict_users"], g["predict_items"])
        assert_tensor_close(stale, g["predict_scores_stale"], what=f"{case} predict")
        fresh = sx.sgl_predict(sgl_params(g, f"w{m['n_steps']}"), graph, hp, g["predict_users"], g["predict_items"])
        assert np.abs(fresh - g["predict_scores_stale"]).max() > 10 * REL * np.abs(stale).max()


def test_sgl_is_wired_in():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib, compat, sgl

    assert compat.MIRRORS["beta_rec.models.sgl"] == "sgl"
    assert sgl.SGL is hp.SGL and sgl.SGLEngine is hp.SGLEngine
    for name in ("create_bpr_loss", "calc_ssl_loss_v2", "randint_choice", "l2_norm"):
        assert hasattr(sgl, name), name
    assert ge.EVIDENCE_GROUPS["sgl"] == ge._EVIDENCE_COMMON + ["sgl.hip", "lightgcn.hip", "spmm.hpp"]
    assert ge.evidence_group("sgl_step") == "sgl"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hiprec.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("hiprec_sgl_plan_bytes", "hiprec_sgl_sub_values", "hiprec_sgl_propagate", "hiprec_sgl_predict",
                 "hiprec_sgl_grad", "hiprec_sgl_tile_b", "hiprec_sgl_tile_n"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert (_lib.SGL_TILE_B, _lib.SGL_TILE_N) == (lib.hiprec_sgl_tile_b(), lib.hiprec_sgl_tile_n())
