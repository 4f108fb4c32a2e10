"""Pin tests/cmn_numpy.py against golden vectors captured from the real reference's cmnEngine by
``tools/gen_golden_cmn.py``.  CPU only."""
import numpy as np
import pytest

import cmn_numpy as cn
from helpers import REL, assert_scalar_close, assert_step_close, assert_tensor_close, assert_update_close, copy_state
from helpers import float64_oracle
from helpers import assert_grads_as_accurate, load_golden, to64

CASES = ["cmn_adam", "cmn_rmsprop_mom", "cmn_sgd_hot_clip"]
KEYS = cn.KEYS
STATE_NAMES = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop_momentum": ("momentum_buffer", "square_avg"), "sgd": ()}


def n_steps(g):
    return int(g["meta"][4])


def cmn_params(case, g, step, tag="w"):
    """Tensor set ``tag`` (w / g / m / v) of the reference after ``step`` steps (w after 0 steps: the initial weights)."""
    if step == 0 and tag == "w":
        return {k: g[f"w0/{k}"].astype(np.float32).copy() for k in KEYS}
    s = load_golden(f"{case}_s{step}")
    return {k: s[f"{tag}/{k}"].astype(np.float32).copy() for k in KEYS}


def cmn_batch(g, s):
    lo, hi = int(g["batch_ptr"][s]), int(g["batch_ptr"][s + 1])
    return cn.padded_batch(g["rowptr"], g["col"], g["users"][lo:hi], g["pos"][lo:hi], g["neg"][lo:hi])


def cmn_triples(g, s):
    lo, hi = int(g["batch_ptr"][s]), int(g["batch_ptr"][s + 1])
    return g["users"][lo:hi], g["pos"][lo:hi], g["neg"][lo:hi]


def cmn_hyper(g):
    """(optimizer, lr, momentum, l2_lambda, grad_clip)"""
    return str(g["optimizer"]), float(g["lr"]), float(g["momentum"]), float(g["l2_lambda"]), float(g["grad_clip"])


def cmn_opt_state(case, g, step):
    opt = str(g["optimizer"])
    st = cn.new_opt_state(cmn_params(case, g, 0), opt)
    st["step"] = step
    if step > 0:
        for name, tag in zip(STATE_NAMES[opt], ("m", "v")):
            st[name] = cmn_params(case, g, step, tag)
    return st


def term_floors(w, batch, lam, clip):
    """Natural magnitude of the TERMS each dense-layer gradient sums (helpers.grad_scale_floor's reasoning): the two
    queries of a sample receive +ds and -ds, so with similar h+ and h- (constructed weights: every unit active) the
    2B terms of dw, dbd, dWd, db, dW cancel to a result orders of magnitude below them -- dbd to exactly zero -- while
    the fp32 rounding error of such a sum stays relative to the terms.  Per tensor the largest single term, from the
    exact (fp64) evaluation, scaled like the clipped gradient; the tables' row gradients get no floor."""
    with float64_oracle(cn):
        w64 = to64(w)
        _, g64, caches = cn.cmn_grads(w64, batch, lam, with_cache=True)
        total = float(np.sqrt(sum((v ** 2).sum() for v in g64.values())))
        coef = min(1.0, clip / (total + 1e-6))
        floors = {k: 0.0 for k in KEYS}
        for c in caches:
            dh, t = np.abs(c["dh"]), np.abs(c["t"])
            # dh = ds * w where the unit is active (h > 0), so |ds * h| = |dh / w| * h
            floors["out.weight"] = max(floors["out.weight"], float((dh / np.abs(w64["out.weight"][0])[None, :]
                                                                     * np.abs(c["h"])).max()))
            floors["dense.bias"] = max(floors["dense.bias"], float(dh.max()))
            floors["dense.weight"] = max(floors["dense.weight"], float(dh.max() * np.abs(c["x"]).max()))
            floors["mem_layer.hop_mapping.1.bias"] = max(floors["mem_layer.hop_mapping.1.bias"], float(t.max()))
            floors[cn.HOP_W] = max(floors[cn.HOP_W], float(t.max() * np.abs(c["z0"]).max()))
    return {k: v * coef for k, v in floors.items()}


def cmn_band(w_prev, st_prev, g_ref, opt, lr, momentum, rel=REL, floors=None):
    """Forward-error band of one optimizer step for a gradient within rel * its scale of g_ref
    (Adam / RMSprop are ill-conditioned where |g| is not >> eps; see helpers.optimizer_band)."""
    outs = []
    floors = floors or {}
    for sign in (+1.0, -1.0):
        w = {k: v.copy() for k, v in w_prev.items()}
        st = copy_state(st_prev)
        gp = {k: (g_ref[k] + np.float32(sign * rel * max(float(np.abs(g_ref[k]).max()), floors.get(k, 0.0)))
                  ).astype(np.float32) for k in KEYS}
        cn.opt_step(w, gp, st, opt, lr, momentum)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in KEYS}


def exact_grads(w, batch, lam, clip):
    """(loss, clipped gradients, pre-clip norm) of the restatement evaluated in fp64."""
    with float64_oracle(cn):
        loss, g64 = cn.cmn_grads(to64(w), batch, lam)
        total = float(np.sqrt(sum((v ** 2).sum() for v in g64.values())))
        coef = min(1.0, clip / (total + 1e-6))
    return loss, {k: v * coef for k, v in g64.items()}, total


@pytest.mark.parametrize("case", CASES)
def test_numpy_oracle_matches_reference(case):
    """Every step in isolation from the reference's own weights and optimizer state: loss, pre-clip norm, every clipped
    gradient, the new weights and the new optimizer state."""
    g = load_golden(case)
    opt, lr, mom, lam, clip = cmn_hyper(g)
    for s in range(n_steps(g)):
        w, st = cmn_params(case, g, s), cmn_opt_state(case, g, s)
        loss, grads = cn.cmn_grads(w, cmn_batch(g, s), lam)
        total, grads = cn.clip_grads(grads, clip)
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        assert_scalar_close(total, g["total_norms"][s], what=f"total norm step {s}")
        g_ref = cmn_params(case, g, s + 1, "g")
        # the dense layers' gradients are sums of +ds / -ds terms that cancel (h+ ~ h- at constructed weights): held to
        # the exact value as closely as the reference itself is, the project's rule for NCF / LightGCN
        _, g64, _ = exact_grads(cmn_params(case, g, s), cmn_batch(g, s), lam, clip)
        floors = term_floors(cmn_params(case, g, s), cmn_batch(g, s), lam, clip)
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}", floor_fn=floors.get)
        band = cmn_band(w, st, g_ref, opt, lr, mom, floors=floors)
        w_prev = {k: v.copy() for k, v in w.items()}
        cn.opt_step(w, grads, st, opt, lr, mom)
        w_ref = cmn_params(case, g, s + 1)
        for k in KEYS:
            assert_step_close(w_prev[k], w[k], w_ref[k], band[k], what=f"weights {k} step {s}")
        # the optimizer's arithmetic on its own, from the reference's gradient: new weights and new state (the state
        # is linear / quadratic in the gradient, so it inherits whatever distance two correct gradients have)
        w2, st2 = {k: v.copy() for k, v in w_prev.items()}, cmn_opt_state(case, g, s)
        cn.opt_step(w2, g_ref, st2, opt, lr, mom)
        nxt = cmn_opt_state(case, g, s + 1)
        for k in KEYS:
            assert_update_close(w_prev[k], w2[k], w_ref[k], what=f"weights from the reference's gradient {k} step {s}")
        for name in STATE_NAMES[opt]:
            for k in KEYS:
                assert_tensor_close(st2[name][k], nxt[name][k], 4e-5, f"{name} {k} step {s}")


@pytest.mark.parametrize("case", CASES)
def test_fixtures_hold_what_the_kernel_can_get_wrong(case):
    """List lengths around the wave and well beyond any chunk, an item on both sides of one batch, a user in many lists,
    u in N(i+), a short last batch; the clip active in the hot fixture only, where about half of each ReLU layer is
    inactive and no pre-activation of the exact evaluation sits within 1e-4 of its layer's scale from zero."""
    g = load_golden(case)
    opt, lr, mom, lam, clip = cmn_hyper(g)
    lens = np.diff(g["rowptr"])
    used = set(g["pos"].tolist()) | set(g["neg"].tolist())
    for n in (1, 2, 63, 64, 65):
        assert int(np.nonzero(lens == n)[0][0]) in used
    assert lens.max() >= 300 and int(np.argmax(lens)) in used
    u0, p0, n0 = cmn_triples(g, 0)
    assert set(p0.tolist()) & set(n0.tolist())
    in_lists = [0 in g["col"][g["rowptr"][i]:g["rowptr"][i + 1]] for i in range(len(lens))]
    assert sum(in_lists) >= len(lens) - 1
    assert any(u in g["col"][g["rowptr"][p]:g["rowptr"][p + 1]] for u, p in zip(u0, p0))
    sizes = np.diff(g["batch_ptr"])
    assert sizes[-1] < sizes[0] == int(g["meta"][3])
    hot = case == "cmn_sgd_hot_clip"
    assert (g["total_norms"] > clip).all() if hot else (g["total_norms"] < clip).all()
    for s in range(n_steps(g)):
        with float64_oracle(cn):
            _, _, caches = cn.cmn_grads(to64(cmn_params(case, g, s)), cmn_batch(g, s), lam, with_cache=True)
        for layer in ("pre1", "preh"):
            pre = np.concatenate([c[layer].reshape(-1) for c in caches])
            assert np.abs(pre).min() >= 1e-4 * np.abs(pre).max()
            if hot:
                assert 0.25 <= (pre <= 0).mean() <= 0.75
            else:
                assert (pre > 0).all()       # biases of 1.0: every unit active at constructed weights


@pytest.mark.parametrize("case", CASES)
def test_reference_own_rounding(case):
    """How far the reference's own fp32 gradients are from the exact (fp64) ones, relative to each tensor's scale: the
    yardstick ``assert_grads_as_accurate`` gives an implementation twice of on top of REL."""
    g = load_golden(case)
    _, _, _, lam, clip = cmn_hyper(g)
    worst = 0.0
    for s in range(n_steps(g)):
        _, g64, _ = exact_grads(cmn_params(case, g, s), cmn_batch(g, s), lam, clip)
        floors = term_floors(cmn_params(case, g, s), cmn_batch(g, s), lam, clip)
        g_ref = cmn_params(case, g, s + 1, "g")
        for k in KEYS:
            worst = max(worst, float(np.abs(g_ref[k] - g64[k]).max() / max(np.abs(g64[k]).max(), floors[k])))
    print(f"{case}: the reference's gradients are within {worst:.2e} of their scale of the exact ones")
    assert worst <= REL


def test_trajectory_from_initial_weights():
    """All steps chained from w0 (the oracle's own state carried along) stay on the reference's path."""
    case = "cmn_sgd_hot_clip"
    g = load_golden(case)
    opt, lr, mom, lam, clip = cmn_hyper(g)
    w = cmn_params(case, g, 0)
    st = cn.new_opt_state(w, opt)
    for s in range(n_steps(g)):
        loss, _ = cn.cmn_train_step(w, st, cmn_batch(g, s), lam, clip, opt, lr, mom)
        assert_scalar_close(loss, g["losses"][s], 5e-5, what=f"loss step {s}")
    w_ref = cmn_params(case, g, n_steps(g))
    for k in KEYS:
        assert_tensor_close(w[k], w_ref[k], 5e-5, what=f"final {k}")


def test_fp64_restatement_is_the_same_function():
    case = "cmn_adam"
    g = load_golden(case)
    w = cmn_params(case, g, 0)
    loss32, g32 = cn.cmn_grads(w, cmn_batch(g, 0), 0.001)
    with float64_oracle(cn):
        loss64, g64 = cn.cmn_grads(to64(w), cmn_batch(g, 0), 0.001)
    assert g64["user_output.weight"].dtype == np.float64
    assert_scalar_close(loss32, loss64, what="loss")
    floors = term_floors(w, cmn_batch(g, 0), 0.001, 5.0)
    for k in KEYS:
        assert_tensor_close(g32[k], g64[k], what=k, scale_floor=floors[k])


def test_constructor_weights_for_a_torch_seed():
    """Same torch seed, same pre-trained tables: the weights the reference's constructor builds (cmn_init), the
    reference's state_dict keys in its order, and config['max_neighbors'] set as the reference sets it."""
    import contextlib
    import io

    import torch

    import beta_recsys_amd as hp

    g = load_golden("cmn_init")
    for tag in ("a", "b"):
        U, I, D, seed = (int(x) for x in g[f"{tag}/meta"])
        rowptr, col = g[f"{tag}/rowptr"], g[f"{tag}/col"]
        lists = {i: col[rowptr[i]:rowptr[i + 1]].tolist() for i in range(I)}
        cfg = {"emb_dim": D, "device_str": "cpu", "regs": [1e-5], "batch_size": 14, "lr": 1e-4, "momentum": 0.9,
               "training_l2_lambda": 0.001, "grad_clip": 5.0, "neg_count": 4,
               "model": {"optimizer": "adam", "lr": 1e-4, "device_str": "cpu"},
               "system": {"run_dir": "/tmp/hiprec_test_runs"}}
        torch.manual_seed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            eng = hp.cmnEngine(cfg, g[f"{tag}/user_embeddings"], g[f"{tag}/item_embeddings"], lists)
        sd = eng.model.state_dict()
        assert tuple(sd) == KEYS == tuple(n for n, _ in eng.model.named_parameters())
        assert cfg["max_neighbors"] == 300 == eng.model.max_neighbors
        assert np.array_equal(sd["user_memory.weight"].numpy(), g[f"{tag}/user_embeddings"])
        assert np.array_equal(sd["item_memory.weight"].numpy(), g[f"{tag}/item_embeddings"])
        for k in KEYS[2:]:
            assert np.array_equal(sd[k].numpy(), g[f"{tag}/w/{k}"]), f"{tag} {k}"
        assert eng.optimizer.name == "adam"
        # no optimizer name the base class knows: the constructor's RMSprop with momentum stays
        cfg["model"]["optimizer"] = "default"
        with contextlib.redirect_stdout(io.StringIO()):
            eng = hp.cmnEngine(cfg, g[f"{tag}/user_embeddings"], g[f"{tag}/item_embeddings"], lists)
        assert (eng.optimizer.name, eng.optimizer.momentum, eng.optimizer.kind) == ("rmsprop", 0.9, 3)


def test_csr_of_the_item_user_list_and_host_side_checks():
    """Every list in its own order, an item the dict does not hold gets [item id]; the new entry points refuse bad
    arguments before they touch a GPU; the compat table routes the reference's module."""
    import ctypes

    from beta_recsys_amd import _lib, cmn, compat

    rowptr, col = cmn.neighborhood_csr({0: [5, 3, 9], 2: [7]}, 4)
    assert rowptr.tolist() == [0, 3, 4, 5, 6] and col.tolist() == [5, 3, 9, 1, 7, 3]
    with pytest.raises(IndexError):
        cmn.neighborhood_csr({4: [1]}, 4)
    assert compat.MIRRORS["beta_rec.models.cmn"] == "cmn" and "cmn" not in _lib.OPT_KINDS
    assert set(_lib.OPT_KINDS) == {"sgd", "adam", "rmsprop"}
    lib = _lib.load()
    assert lib.hiprec_cmn_tables_bytes() == ctypes.sizeof(_lib.CmnTables)
    assert lib.hiprec_cmn_workspace_bytes(64, 1024) >= 4 * 2 * 1024 * 6 * 64
    t = _lib.CmnTables(0, 0, 0, 0, 0, 0, 0, 0, 10, 5, 64, 0)
    rc = lib.hiprec_cmn_grad_csr(ctypes.byref(t), None, None, None, None, None, None, 4, 0.25, 0.0, None, None, None,
                                 None, 0, None, 0, None)
    assert rc == -1 and b"CSR" in lib.hiprec_last_error()
    rc = lib.hiprec_cmn_grad_padded(ctypes.byref(t), None, None, None, None, None, None, 0, None, None, 0, 4, 0.25, 0.0,
                                    None, None, None, None, 0, None, 0, None)
    assert rc == -1 and b"neighbourhoods" in lib.hiprec_last_error()
    rc = lib.hiprec_cmn_epoch(ctypes.byref(t), None, None, None, None, None, None, 8, 4, 0.0, 5.0, 3, 1e-4, 0.9, 0.99,
                              1e-8, None, None, None, None, 0, None, None, 0, None, 0, None, 0, None)
    assert rc == -1
    rc = lib.hiprec_opt_dense_step(3, None, None, None, None, 4, 0.1, 0.9, 0.99, 1e-8, None, None, -1, None)
    assert rc == -1
    with pytest.raises(ValueError):
        from beta_recsys_amd import HipOptimizer

        HipOptimizer("adam", 0.1, momentum=0.9)
