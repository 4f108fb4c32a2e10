"""The numpy restatement of LCFN (tests/lcfn_numpy.py) against the reference's own vectors (tests/golden/lcfn_*.npz,
captured by tools/gen_golden_lcfn.py from beta_rec/models/lcfn.py with layer = 1, the only depth the reference runs)."""
import glob
import os
import re
import sys

import numpy as np
import pytest

import lcfn_numpy as lx
from helpers import GOLDEN, REL, assert_on_trajectory, assert_scalar_close, assert_sgd_exact, assert_step_close
from helpers import assert_tensor_close, copy_state, float64_oracle, load_golden, oracle_trajectory, to64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["lcfn_adam", "lcfn_sgd_hot", "lcfn_rmsprop_d64"]
KEYS = lx.KEYS
_cache = {}


def lcfn_golden(case):
    """A case's fixture; a case too large for one committed file keeps its per-step tensors in <case>_s<step>.npz."""
    if case not in _cache:
        g = load_golden(case)
        for path in sorted(glob.glob(os.path.join(GOLDEN, case + "_s*.npz"))):
            g.update(load_golden(os.path.basename(path)[:-4]))
        _cache[case] = g
    return _cache[case]


def lcfn_meta(g):
    U, I, D, Fu, Fi, L, B, n_steps, seed = (int(x) for x in g["meta"])
    return {"U": U, "I": I, "D": D, "Fu": Fu, "Fi": Fi, "L": L, "B": B, "n_steps": n_steps, "seed": seed}


def lcfn_hp(g):
    return {"L": lcfn_meta(g)["L"], "lamda": float(g["lamda"])}


def lcfn_bases(g):
    return g["P"], g["Q"]


def lcfn_tail(g):
    return {k: g[f"w0/{k}"].astype(np.float32).copy() for k in lx.tail_keys(lcfn_meta(g)["L"])}


def lcfn_params(g, prefix):
    """The two tables under ``prefix`` (w0, w1, g1, m1 ...)."""
    return {k: g[f"{prefix}/{k}"].astype(np.float32).copy() for k in KEYS}


def lcfn_weights(g, prefix):
    """The two tables under ``prefix`` and the tail (which the reference never moves)."""
    return {**lcfn_params(g, prefix), **lcfn_tail(g)}


def lcfn_batch(g, s):
    return g["users"][s], g["pos"][s], g["neg"][s]


def lcfn_opt_state(g, step, opt):
    st = lx.new_opt_state(lcfn_params(g, "w0"), opt)
    st["step"] = step
    if step > 0 and opt == "adam":
        st["exp_avg"], st["exp_avg_sq"] = lcfn_params(g, f"m{step}"), lcfn_params(g, f"v{step}")
    elif step > 0 and opt == "rmsprop":
        st["square_avg"] = lcfn_params(g, f"v{step}")
    return st


def lcfn_band(w_prev, st_prev, g_ref, opt, lr, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel * its scale of g_ref (helpers.optimizer_band)."""
    outs = []
    for sign in (+1.0, -1.0):
        w = {k: w_prev[k].copy() for k in KEYS}
        st = copy_state(st_prev)
        gr = {k: (g_ref[k] + np.float32(sign * rel * float(np.abs(g_ref[k]).max()))).astype(np.float32) for k in KEYS}
        lx.opt_step(w, gr, st, opt, lr)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in KEYS}


def lcfn_trajectory(g, trials):
    """helpers.oracle_trajectory of the restatement over a case's steps: ``(w_ref, env, upd)`` for the two tables."""
    hp, bases, m, tail = lcfn_hp(g), lcfn_bases(g), lcfn_meta(g), lcfn_tail(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    return oracle_trajectory(lcfn_params(g, "w0"), list(range(m["n_steps"])),
                             lambda w, s: lx.lcfn_grads({**w, **tail}, bases, hp, lcfn_batch(g, s))[2],
                             lambda w, gr, st: lx.opt_step(w, gr, st, opt, lr), lambda w: lx.new_opt_state(w, opt),
                             trials=trials)


@pytest.mark.parametrize("case", CASES)
def test_every_step_in_isolation(case):
    g = lcfn_golden(case)
    hp, bases, m = lcfn_hp(g), lcfn_bases(g), lcfn_meta(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    for s in range(m["n_steps"]):
        w0, st0 = lcfn_weights(g, f"w{s}"), lcfn_opt_state(g, s, opt)
        parts, loss, grads = lx.lcfn_grads(w0, bases, hp, lcfn_batch(g, s))
        assert_scalar_close(loss, g["losses"][s], what=f"{case} loss step {s}")
        for got, ref, name in zip(parts, g["parts"][s], ("bpr", "reg")):
            assert_scalar_close(got, ref, what=f"{case} {name} step {s}")
        g_ref = lcfn_params(g, f"g{s + 1}")
        assert set(grads) == set(KEYS)
        for k in KEYS:
            assert_tensor_close(grads[k], g_ref[k], what=f"{case} grad {k} step {s}")
        band = lcfn_band(w0, st0, g_ref, opt, lr)
        w1, st1 = {k: w0[k].copy() for k in KEYS}, copy_state(st0)
        lx.opt_step(w1, grads, st1, opt, lr)
        nxt = lcfn_opt_state(g, s + 1, opt)
        for k in KEYS:
            assert_step_close(w0[k], w1[k], g[f"w{s + 1}/{k}"], band[k], what=f"{case} weights {k} step {s}")
            for name in ("exp_avg", "exp_avg_sq", "square_avg"):
                if name in nxt:
                    assert_tensor_close(st1[name][k], nxt[name][k], REL if name == "exp_avg" else 2 * REL,
                                        f"{case} {name} {k} step {s}")


@pytest.mark.parametrize("case", CASES)
def test_chained_trajectory(case):
    g = lcfn_golden(case)
    m, opt = lcfn_meta(g), str(g["optimizer"])
    w_ref, env, upd = lcfn_trajectory(g, 0 if opt == "sgd" else 8)
    ref_end = lcfn_params(g, f"w{m['n_steps']}")
    if opt == "sgd":
        assert_sgd_exact(w_ref, ref_end, lcfn_params(g, "w0"), f"{case} final weights")
    else:
        assert_on_trajectory(w_ref, ref_end, env, upd, f"{case} trajectory")


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_and_reference_own_rounding(case):
    """The fp64 restatement reproduces the reference's own fp64 gradients (1e-9 of scale), and the reference's fp32
    gradients lie within REL / 3 of them: the GPU test's bound -- REL of scale plus twice that distance -- has room."""
    g = lcfn_golden(case)
    hp, bases, m = lcfn_hp(g), lcfn_bases(g), lcfn_meta(g)
    for s in range(m["n_steps"]):
        with float64_oracle(lx):
            _, l64, g64 = lx.lcfn_grads(to64(lcfn_weights(g, f"w{s}")), bases, hp, lcfn_batch(g, s))
        assert g64[KEYS[0]].dtype == np.float64
        assert_scalar_close(l64, g["losses"][s], what=f"{case} loss step {s}")
        for k in KEYS:
            assert_tensor_close(g64[k], g[f"g64_{s + 1}/{k}"], 1e-9, f"{case} fp64 grad {k} step {s}")
            own = float(np.abs(g[f"g{s + 1}/{k}"] - g64[k]).max() / np.abs(g64[k]).max())
            assert own <= REL / 3, f"{case} step {s} {k}: the reference's own rounding is {own:.2e} of scale"


def test_hot_fixture_repeats_every_row():
    g = lcfn_golden("lcfn_sgd_hot")
    for s in range(3):
        users, pos, neg = lcfn_batch(g, s)
        assert len(set(users)) <= 4 and len(set(pos) | set(neg)) <= 5
        assert min(np.bincount(users).max(), np.bincount(pos).max(), np.bincount(neg).max()) >= 2


def test_predict_is_the_reference_on_the_weights_it_last_propagated():
    """The reference's predict reads the tables of its last training forward -- the weights BEFORE the last step; the
    restatement on those weights reproduces it, and on the final weights (what the mirror returns) it differs."""
    for case in CASES:
        g = lcfn_golden(case)
        hp, bases, m = lcfn_hp(g), lcfn_bases(g), lcfn_meta(g)
        stale = lx.lcfn_predict(lcfn_weights(g, f"w{m['n_steps'] - 1}"), bases, hp, g["predict_users"], g["predict_items"])
        assert_tensor_close(stale, g["predict_scores_stale"], what=f"{case} predict")
        fresh = lx.lcfn_predict(lcfn_weights(g, f"w{m['n_steps']}"), bases, hp, g["predict_users"], g["predict_items"])
        assert np.abs(fresh - g["predict_scores_stale"]).max() > 10 * REL * np.abs(stale).max()


def test_fixture_files_stay_small():
    for path in glob.glob(os.path.join(GOLDEN, "lcfn_*.npz")):
        assert os.path.getsize(path) < (1 << 20), path


def test_lcfn_is_wired_in():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib, compat, lcfn

    assert compat.MIRRORS["beta_rec.models.lcfn"] == "lcfn"
    assert lcfn.LCFN is hp.LCFN and lcfn.LCFNEngine is hp.LCFNEngine
    assert ge.EVIDENCE_GROUPS["lcfn"] == ge._EVIDENCE_COMMON + ["lcfn.hip"]
    assert ge.evidence_group("lcfn_step") == "lcfn"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hiprec.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("hiprec_lcfn_plan_bytes", "hiprec_lcfn_ws_floats", "hiprec_lcfn_batch_ws_floats", "hiprec_lcfn_propagate",
                 "hiprec_lcfn_predict", "hiprec_lcfn_grad"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.hiprec_version() == 100
