"""The BUIR restatement (tests/buir_numpy.py) against golden vectors captured from the real reference
(tests/golden/buir_*.npz, tools/gen_golden_buir.py): loss, gradients, optimizer steps and the moving target; that the model
is wired in; that shapes beyond a limit are refused.  CPU only."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

import buir_numpy as bx
from helpers import REL, assert_on_trajectory, assert_scalar_close, assert_sgd_exact, assert_step_close
from helpers import assert_tensor_close, copy_state, float64_oracle, load_golden, oracle_trajectory, to64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["buir_adam", "buir_sgd_hot", "buir_rmsprop_d64", "buir_adam_ema"]
KEYS, TRAINABLE, TARGET, ONLINE = bx.KEYS, bx.TRAINABLE, bx.TARGET, bx.ONLINE


def bu_params(g, prefix, keys=KEYS):
    return {k: g[f"{prefix}/{k}"].astype(np.float32).copy() for k in keys}


def bu_meta(g):
    U, I, D, L, B, n_steps, seed = (int(x) for x in g["meta"])
    return dict(U=U, I=I, D=D, L=L, B=B, n_steps=n_steps, seed=seed, momentum=float(g["momentum"]), ema=bool(int(g["ema"])))


def bu_graph(g):
    m = bu_meta(g)
    return g["adj_row"], g["adj_col"], g["adj_val"], m["U"] + m["I"]


def bu_batch(g, s):
    return g["users"][s], g["pos"][s], g["neg"][s]


def bu_opt_state(g, step, opt):
    st = bx.new_opt_state(bu_params(g, "w0"), opt)
    st["step"] = step
    if step > 0 and opt == "adam":
        st["exp_avg"], st["exp_avg_sq"] = bu_params(g, f"m{step}", TRAINABLE), bu_params(g, f"v{step}", TRAINABLE)
    elif step > 0 and opt == "rmsprop":
        st["square_avg"] = bu_params(g, f"v{step}", TRAINABLE)
    return st


def bu_band(w_prev, st_prev, g_ref, opt, lr, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel * its scale of g_ref (helpers.optimizer_band)."""
    outs = []
    for sign in (+1.0, -1.0):
        w = {k: v.copy() for k, v in w_prev.items()}
        st = copy_state(st_prev)
        gr = {k: (g_ref[k] + np.float32(sign * rel * float(np.abs(g_ref[k]).max()))).astype(np.float32) for k in TRAINABLE}
        bx.opt_step(w, gr, st, opt, lr)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in TRAINABLE}


def bu_trajectory(g, ema=None):
    """helpers.oracle_trajectory over the restated step (the moving target after each optimizer step when recorded)."""
    m, graph = bu_meta(g), bu_graph(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    ema = m["ema"] if ema is None else ema

    def grad_fn(w, s):
        return {k: v for k, v in bx.buir_grads(w, graph, m["L"], bu_batch(g, s))[1].items() if k in TRAINABLE}

    def step_fn(w, gr, st):
        bx.opt_step(w, gr, st, opt, lr)
        if ema:
            bx.ema(w, m["momentum"])

    return oracle_trajectory(bu_params(g, "w0"), list(range(m["n_steps"])), grad_fn, step_fn,
                             lambda w: bx.new_opt_state(w, opt), trials=0 if opt == "sgd" else 8)


def model_config(g, **over):
    m = bu_meta(g)
    N = m["U"] + m["I"]
    adj = torch.sparse_coo_tensor(np.vstack([g["adj_row"], g["adj_col"]]), g["adj_val"], (N, N))
    cfg = dict(n_users=m["U"], n_items=m["I"], emb_dim=m["D"], momentum=m["momentum"], batch_size=m["B"], norm_adj=adj,
               optimizer=str(g["optimizer"]), lr=float(g["lr"]), device_str="cpu", update_target=m["ema"])
    cfg.update(over)
    return cfg


def make_engine(g, **over):
    import beta_recsys_amd as hp

    with contextlib.redirect_stdout(io.StringIO()):
        return hp.BUIREngine({"model": model_config(g, **over), "system": {"run_dir": "/tmp/hiprec_test_runs"}})


@pytest.mark.parametrize("case", CASES)
def test_every_step_in_isolation(case):
    g = load_golden(case)
    graph, m = bu_graph(g), bu_meta(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    for s in range(m["n_steps"]):
        w0, st0 = bu_params(g, f"w{s}"), bu_opt_state(g, s, opt)
        loss, grads = bx.buir_grads(w0, graph, m["L"], bu_batch(g, s))
        assert_scalar_close(loss, g["losses"][s], what=f"{case} loss step {s}")
        g_ref = bu_params(g, f"g{s + 1}", TRAINABLE)
        for k in TRAINABLE:
            assert_tensor_close(grads[k], g_ref[k], what=f"{case} grad {k} step {s}")
        for k in TARGET:
            assert not grads[k].any(), f"{case}: a gradient reached {k}"
        band = bu_band(w0, st0, g_ref, opt, lr)
        w1, st1 = {k: v.copy() for k, v in w0.items()}, copy_state(st0)
        bx.opt_step(w1, grads, st1, opt, lr)
        if m["ema"]:
            bx.ema(w1, m["momentum"])
        nxt = bu_opt_state(g, s + 1, opt)
        for k in TRAINABLE:
            assert_step_close(w0[k], w1[k], g[f"w{s + 1}/{k}"], band[k], what=f"{case} weights {k} step {s}")
            for name in ("exp_avg", "exp_avg_sq", "square_avg"):
                if name in nxt:
                    assert_tensor_close(st1[name][k], nxt[name][k], REL if name == "exp_avg" else 2 * REL,
                                        f"{case} {name} {k} step {s}")
        for o, t in zip(ONLINE, TARGET):
            if m["ema"]:   # (1 - m) x the online table's band, plus the rounding of the three operations
                assert_step_close(w0[t], w1[t], g[f"w{s + 1}/{t}"], (1 - m["momentum"]) * band[o],
                                  what=f"{case} target {t} step {s}")
            else:
                assert np.array_equal(w1[t], g[f"w{s + 1}/{t}"]) and np.array_equal(w0[t], w1[t]), f"{case} {t} moved"


@pytest.mark.parametrize("case", CASES)
def test_chained_trajectory(case):
    g = load_golden(case)
    m, opt = bu_meta(g), str(g["optimizer"])
    w0 = bu_params(g, "w0")
    w_ref, env, upd = bu_trajectory(g)
    ref_end = bu_params(g, f"w{m['n_steps']}")
    if opt == "sgd":
        assert_sgd_exact(w_ref, ref_end, w0, f"{case} final weights")
    else:
        assert_on_trajectory(w_ref, ref_end, env, upd, f"{case} trajectory")


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_and_reference_own_rounding(case):
    """The fp64 restatement reproduces the reference's own fp64 gradients (1e-9 of scale) and its loss, and the
    reference's fp32 gradients lie within REL / 3 of the fp64 ones: the GPU test's bound -- REL of scale plus twice that
    distance -- has room."""
    g = load_golden(case)
    graph, m = bu_graph(g), bu_meta(g)
    for s in range(m["n_steps"]):
        with float64_oracle(bx):
            l64, g64 = bx.buir_grads(to64(bu_params(g, f"w{s}")), graph, m["L"], bu_batch(g, s))
        assert g64[TRAINABLE[0]].dtype == np.float64
        assert_scalar_close(l64, g["losses"][s], what=f"{case} loss step {s}")
        for k in TRAINABLE:
            assert_tensor_close(g64[k], g[f"g64_{s + 1}/{k}"], 1e-9, f"{case} fp64 grad {k} step {s}")
            own = float(np.abs(g[f"g{s + 1}/{k}"] - g64[k]).max() / np.abs(g64[k]).max())
            assert own <= REL / 3, f"{case} step {s} {k}: the reference's own rounding is {own:.2e} of scale"


def test_hot_fixture_is_hot():
    g = load_golden("buir_sgd_hot")
    for s in range(3):
        assert len(set(g["users"][s])) <= 5 and len(set(g["pos"][s])) <= 7 and bu_meta(g)["B"] == 64


def test_the_moving_target_is_the_references_update():
    """buir_adam_ema: the recorded target tables are the reference's own ``_update_target`` after each step -- the
    restated ``ema`` applied to the recorded weights reproduces them bit for bit, and they do move."""
    g = load_golden("buir_adam_ema")
    m = bu_meta(g)
    assert m["ema"]
    for s in range(m["n_steps"]):
        w = bu_params(g, f"w{s}")
        for k in ONLINE:
            w[k] = g[f"w{s + 1}/{k}"].copy()     # _update_target reads the online tables AFTER the optimizer step
        bx.ema(w, m["momentum"])
        for t in TARGET:
            assert np.array_equal(w[t], g[f"w{s + 1}/{t}"]), f"step {s} {t}"
            assert not np.array_equal(g[f"w{s}/{t}"], g[f"w{s + 1}/{t}"])


def test_predict_reads_the_online_encoder():
    for case in CASES:
        g = load_golden(case)
        m = bu_meta(g)
        w = bu_params(g, f"w{m['n_steps']}")
        assert_tensor_close(bx.buir_predict(w, bu_graph(g), m["L"], g["predict_users"], g["predict_items"]),
                            g["predict_scores"], what=f"{case} predict")


def test_buir_is_wired_in():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib, buir, compat

    assert compat.MIRRORS["beta_rec.models.buir"] == "buir"
    assert buir.BUIR_NB is hp.BUIR_NB and buir.BUIREngine is hp.BUIREngine
    assert "buir.hip" in ge.EVIDENCE_GROUPS["buir"] and ge.evidence_group("buir_step") == "buir"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hiprec.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(hiprec_buir_\w+)\(", header))
    assert names == {"hiprec_buir_" + n for n in ("plan_bytes", "tile_b", "max_dim", "max_layers", "ws_floats",
                                                  "batch_ws_floats", "pool", "grad", "ema", "predict")}
    lib = _lib.load()
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert (_lib.BUIR_TILE_B, _lib.BUIR_MAX_DIM, _lib.BUIR_MAX_LAYERS) == (
        lib.hiprec_buir_tile_b(), lib.hiprec_buir_max_dim(), lib.hiprec_buir_max_layers())
    assert lib.hiprec_buir_plan_bytes() == __import__("ctypes").sizeof(_lib.BuirPlan)
    # the target is never propagated inside a step: five [n, D] tables whatever L is
    assert lib.hiprec_buir_ws_floats(1000, 64) == 5 * 1000 * 64
    assert lib.hiprec_buir_batch_ws_floats(65, 16) == 3 * (16 * 16 + 16)


def test_state_dict_and_initial_weights_are_the_references():
    """The recorded key list in the recorded order, and for the same torch seed bit-equal initial weights (buir.py:20-39:
    online user, online item, the target's two discarded draws, nn.Linear)."""
    for case in ("buir_adam", "buir_rmsprop_d64"):
        g = load_golden(case)
        torch.manual_seed(int(g["torch_seed"]))
        eng = make_engine(g)
        sd = eng.model.state_dict()
        assert list(sd) == [str(k) for k in g["state_dict_keys"]] == list(KEYS)
        for k in KEYS:
            assert np.array_equal(sd[k].numpy(), g[f"w0/{k}"]), k
        # the target tables sit behind everything the optimizer sweeps
        assert eng._sweep_floats() == sum(g[f"w0/{k}"].size for k in TRAINABLE) == eng.model.offset_of(TARGET[0])
        assert eng.model.flat.numel() == sum(g[f"w0/{k}"].size for k in KEYS)


def test_load_state_dict_round_trip_on_the_host():
    g = load_golden("buir_adam")
    eng = make_engine(g)
    w = bu_params(g, "w2")
    eng.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    for k, v in eng.model.state_dict().items():
        assert np.array_equal(v.numpy(), w[k]), k
    assert eng.model.online_encoder.embedding_dict["user_emb"].data_ptr() == eng.model.flat.data_ptr()


def test_shapes_beyond_a_limit_are_refused():
    """ValueError from Python before anything is allocated; the C entry points return an error code for the same shapes
    (no GPU is needed to be refused)."""
    import ctypes

    from beta_recsys_amd import _lib

    g = load_golden("buir_adam")
    for over, text in (({"emb_dim": 257}, "emb_dim"), ({"emb_dim": 0}, "emb_dim"), ({"n_layers": 0}, "n_layers"),
                       ({"n_layers": 5}, "n_layers")):
        with pytest.raises(ValueError, match=text):
            make_engine(g, **over)
    lib = _lib.load()
    for dim, layers in ((257, 3), (0, 3), (16, 0), (16, 5)):
        p = _lib.BuirPlan()
        p.n_users, p.n_items, p.dim, p.n_layers = 4, 6, dim, layers
        for call in (lambda: lib.hiprec_buir_predict(ctypes.byref(p), None, None, 0, None, None, None),
                     lambda: lib.hiprec_buir_pool(ctypes.byref(p), None, None, None, None),
                     lambda: lib.hiprec_buir_ema(ctypes.byref(p), None),
                     lambda: lib.hiprec_buir_grad(ctypes.byref(p), None, None, None, 0, None, None, 0, None)):
            assert call() != 0
            with pytest.raises(_lib.HiprecError, match="supported"):
                _lib.check(call())


def test_batches_are_checked_before_the_device_is():
    """A batch must be a 3-tuple of equal, non-zero lengths (the negatives are accepted and ignored); the data-parallel
    form is not built."""
    g = load_golden("buir_adam")
    eng = make_engine(g)
    eng._setup = lambda: None            # the checks run ahead of anything that needs the device
    u, p, n = bu_batch(g, 0)
    with pytest.raises(ValueError, match="users, pos_items, neg_items"):
        eng._enqueue_grad((u, p))
    with pytest.raises(ValueError, match="differ in length"):
        eng._enqueue_grad((u, p[:-1], n))
    with pytest.raises(ValueError, match="empty"):
        eng._enqueue_grad((u[:0], p[:0], n[:0]))
    eng._dp_world = 2
    with pytest.raises(NotImplementedError):
        eng._enqueue_grad((u, p, n))
