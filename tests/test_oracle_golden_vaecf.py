"""Pin tests/vaecf_numpy.py against golden vectors captured from the real reference's VAECFEngine by
``tools/gen_golden_vaecf.py``, and the host-side parts of the VAECF mirror: the noise draw, the constructor, the limits,
the loader, the registration, and the checks that a wrong implementation would be VISIBLE on the fixtures.  CPU only."""
import numpy as np
import pytest
import torch

import vaecf_edges as ve
import vaecf_numpy as vn
from helpers import REL, assert_grads_as_accurate, assert_scalar_close, assert_step_close
from helpers import copy_state, float64_oracle, load_golden, to64

CASES = ["vaecf_mult_tanh", "vaecf_bern_relu_wd", "vaecf_gaus_sigmoid_short", "vaecf_pois_relu6", "vaecf_mult_two_layers"]
MIN_MARGIN = 2.0      # a wrong implementation must move some gradient by more than this many GPU-test bounds


def meta(g):
    """(U, I, z_dim, B, config batch_size, steps, seed, hidden)"""
    m = [int(x) for x in g["meta"]]
    return tuple(m[:7]) + (m[7:],)


def hyper(g):
    """(likelihood, activation, weight_decay, lr, beta)"""
    return str(g["likelihood"]), str(g["activation"]), float(g["weight_decay"]), float(g["lr"]), float(g["beta"])


def keys_of(g):
    return vn.keys(len(meta(g)[7]))


def vc_params(case, g, step, tag="w"):
    """Tensor set ``tag`` (w / g / m / v) of the reference after ``step`` steps (w after 0 steps: the initial weights)."""
    if step == 0 and tag == "w":
        return {k: g[f"w0/{k}"].astype(np.float32).copy() for k in keys_of(g)}
    s = load_golden(f"{case}_s{step}")
    return {k: s[f"{tag}/{k}"].astype(np.float32).copy() for k in keys_of(g)}


def vc_opt_state(case, g, step):
    st = vn.new_opt_state(vc_params(case, g, 0), "adam")
    st["step"] = step
    if step > 0:
        st["exp_avg"], st["exp_avg_sq"] = vc_params(case, g, step, "m"), vc_params(case, g, step, "v")
    return st


def exact_grads(w, x, eps, beta, activation, likelihood, **variant):
    with float64_oracle(vn):
        return vn.vaecf_grads(to64(w), x, eps, beta, activation, likelihood, **variant)


def vc_band(w_prev, st_prev, g_ref, lr, wd, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel of its scale of g_ref
    (helpers.optimizer_band's rule on this model's keys)."""
    outs = []
    for sign in (+1.0, -1.0):
        w, st = {k: v.copy() for k, v in w_prev.items()}, copy_state(st_prev)
        gp = {k: (g_ref[k] + np.float32(sign * rel * float(np.abs(g_ref[k]).max()))).astype(np.float32) for k in w}
        vn.opt_step(w, gp, st, lr, wd)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in w_prev}


def model_config(U=9, I=11, activation="tanh", likelihood="mult", batch_size=6, lr=0.01, beta=0.2, weight_decay=0.0,
                 optimizer="adam", device="cpu", **extra):
    model = {"n_users": U, "n_items": I, "activation": activation, "likelihood": likelihood, "batch_size": batch_size,
             "lr": lr, "beta": beta, "weight_decay": weight_decay, "optimizer": optimizer, "device_str": device}
    model.update(extra)
    return {"model": model, "system": {"run_dir": "/tmp/hiprec_vaecf_runs"}}


def golden_config(g, device="cpu", **extra):
    U, I, Z, _, bs, _, _, hidden = meta(g)
    lik, activation, wd, lr, beta = hyper(g)
    return model_config(U, I, activation, lik, bs, lr, beta, wd, str(g["optimizer"]), device, z_dim=Z, hidden=hidden,
                        **extra)


def edge_config(shape, device="cpu", **extra):
    I, hidden, Z, B, activation, likelihood, _ = shape
    return model_config(max(B, 2), I, activation, likelihood, B, 0.01, ve.BETA, 0.0, "adam", device, z_dim=Z,
                        hidden=hidden, **extra)


@pytest.mark.parametrize("case", CASES)
def test_numpy_restatement_matches_reference(case):
    """Every step in isolation from the reference's own weights and optimizer state: the loss and its two parts, every
    gradient (in fp32 as accurate as the reference against the fp64 evaluation), the new weights."""
    g = load_golden(case)
    lik, activation, wd, lr, beta = hyper(g)
    for s in range(meta(g)[5]):
        w, st = vc_params(case, g, s), vc_opt_state(case, g, s)
        x, eps = g["x"][s], g[f"eps{s}"]
        loss, ll, kld, grads, _ = vn.vaecf_grads(w, x, eps, beta, activation, lik)
        loss64, ll64, kld64, g64, _ = exact_grads(w, x, eps, beta, activation, lik)
        for got, got64, ref, what in ((loss, loss64, g["losses"][s], "loss"), (ll, ll64, g["lls"][s], "ll"),
                                      (kld, kld64, g["klds"][s], "kld")):
            assert_scalar_close(got, ref, what=f"{what} step {s}")
            assert_scalar_close(got64, ref, what=f"fp64 {what} step {s}")
        g_ref = vc_params(case, g, s + 1, "g")
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}")
        band = vc_band(w, st, g_ref, lr, wd)
        w_prev = {k: v.copy() for k, v in w.items()}
        vn.opt_step(w, grads, st, lr, wd)
        w_ref = vc_params(case, g, s + 1)
        for k in w:
            assert_step_close(w_prev[k], w[k], w_ref[k], band[k], what=f"weights {k} step {s}")


@pytest.mark.parametrize("case", CASES)
def test_fixtures_are_well_conditioned(case):
    """In the fp64 evaluation at every step: the batch layout, the margins of the conditioning recipe, and the
    reference's own gradients within REL of their scale of the exact ones."""
    g = load_golden(case)
    lik, activation, _, _, beta = hyper(g)
    for s in range(meta(g)[5]):
        x = g["x"][s]
        ve.check_batch(x)
        _, _, _, g64, info = exact_grads(vc_params(case, g, s), x, g[f"eps{s}"], beta, activation, lik)
        g_ref = vc_params(case, g, s + 1, "g")
        worst = max(float(np.abs(g_ref[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in g_ref)
        print(f"{case} step {s}: min |pre| {info['min_abs_pre']:.3f}, max |logvar| {info['max_abs_logvar']:.3f}; the "
              f"reference's gradients are within {worst:.2e} of their scale of the exact ones")
        assert ve.margins_ok(info, activation)
        assert worst <= REL
    assert g["replay_ok"].all()
    assert bool(g["patched_A"]), "the fixture says whether .A had to be added to scipy's csr_matrix"


@pytest.mark.parametrize("shape", ve.SHAPES, ids=ve.shape_id)
def test_edge_inputs_are_well_conditioned(shape):
    w, x, eps = ve.synthetic(shape)
    I, hidden, Z, B, activation, likelihood, valued = shape
    if B >= 2:
        ve.check_batch(x, I in ve.EVERY_ITEM)
    assert (x != 0).sum(1).max() > 64 or I <= 65
    assert valued == bool(((x != 0) & (x != 1)).any())
    _, _, _, g64, info = exact_grads(w, x, eps, ve.BETA, activation, likelihood)
    _, _, _, g32, _ = vn.vaecf_grads(w, x, eps, ve.BETA, activation, likelihood)
    worst = max(float(np.abs(g32[k] - g64[k]).max() / (np.abs(g64[k]).max() + 1e-300)) for k in g64)
    print(f"{ve.shape_id(shape)}: min |pre| {info['min_abs_pre']:.3f}, max |logvar| {info['max_abs_logvar']:.3f}, max "
          f"|z| {info['max_abs_z']:.2f}; the fp32 restatement's gradients are within {worst:.2e} of their scale of the "
          f"exact ones")
    assert ve.margins_ok(info, activation)
    assert worst <= REL


def test_csr_helpers_round_trip():
    x = ve.make_x(np.random.default_rng(3), 7, 13, valued=True)
    row_ptr, items, values = vn.csr_of(x)
    assert row_ptr[0] == 0 and row_ptr[1] == 0 and row_ptr[-1] == len(items) == len(values)
    assert np.array_equal(vn.dense_of(row_ptr, items, values, 13), x)


# ---- noise, constructor, limits, loader, registration -------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_draw_noise_is_the_reference_eps_bit_for_bit(case):
    from beta_recsys_amd.vaecf import draw_noise

    g = load_golden(case)
    _, _, Z, B, _, steps, _, _ = meta(g)
    for s in range(steps):
        torch.set_rng_state(torch.from_numpy(g[f"rng_state{s}"]))
        noise = draw_noise(B, Z, "cpu").numpy()
        assert noise.shape == (B, Z) and np.array_equal(noise, g[f"eps{s}"])


@pytest.mark.parametrize("case", CASES)
def test_constructor_reproduces_the_reference_weights(case):
    """Same torch seed, same constructed weights (the fixture's ``winit``: before the conditioning recipe), same
    ``state_dict`` keys, shapes and order -- through the engine for the hard-coded network, through ``VAE(...)``
    directly for the two-layer one."""
    import contextlib
    import io

    import beta_recsys_amd as hp

    g = load_golden(case)
    U, I, Z, _, _, _, seed, hidden = meta(g)
    cfg = golden_config(g)
    torch.manual_seed(seed)
    if case == "vaecf_mult_two_layers":
        model = hp.VAE(Z, [I] + hidden, cfg["model"])
    else:
        del cfg["model"]["z_dim"], cfg["model"]["hidden"]            # the reference's hard-coded 10 and [20]
        with contextlib.redirect_stdout(io.StringIO()):
            model = hp.VAECFEngine(cfg).model
        assert (model.z_dim, model.hidden) == (10, [20])
    sd = model.state_dict()
    assert tuple(sd) == keys_of(g) == tuple(n for n, _ in model.named_parameters())
    for k, shape in vn.shapes(I, hidden, Z).items():
        assert tuple(sd[k].shape) == shape
        assert np.array_equal(sd[k].numpy(), g[f"winit/{k}"]), k
    model.load_state_dict({k: torch.from_numpy(g[f"w0/{k}"]) for k in keys_of(g)})
    assert np.array_equal(model.flat.numpy(), np.concatenate([g[f"w0/{k}"].ravel() for k in keys_of(g)]))


def test_config_limits_and_value_errors():
    import beta_recsys_amd as hp
    from beta_recsys_amd import vaecf

    def build(z=10, hidden=(20,), I=11, **kw):
        return hp.VAE(z, [I] + list(hidden), model_config(I=I, **kw)["model"])

    assert (vaecf.MAX_Z, vaecf.MAX_HIDDEN, vaecf.MAX_LAYERS) == (256, 512, 3)
    for bad in (dict(z=257), dict(z=0), dict(hidden=(513,)), dict(hidden=(0,)), dict(hidden=()), dict(hidden=(8, 8, 8, 8)),
                dict(activation="prelu"), dict(activation="lrelu"), dict(likelihood="normal"), dict(I=0), dict(U=0),
                dict(noise_rng="numpy"), dict(w0_gather="rows")):
        with pytest.raises(ValueError):
            build(**bad)
    m = build(z=256, hidden=(512, 1, 512), I=1)                       # the limits
    assert list(m.shape.hidden) == [512, 1, 512] and m.shape.n_hidden == 3
    assert [build(activation=a).shape.act for a in ("sigmoid", "tanh", "relu", "relu6")] == [0, 1, 2, 3]
    assert [build(likelihood=k).shape.likelihood for k in ("mult", "bern", "gaus", "pois")] == [0, 1, 2, 3]
    assert build(w0_gather="shadow").shape.w0_shadow == 1 and build().shape.w0_shadow == 0
    with pytest.raises(NotImplementedError, match="set_history"):
        build().ranking_factors()


def test_engine_is_always_adam_with_weight_decay():
    import contextlib
    import io

    import beta_recsys_amd as hp

    for name in ("sgd", "rmsprop", "adam", "whatever"):
        with contextlib.redirect_stdout(io.StringIO()):
            eng = hp.VAECFEngine(model_config(optimizer=name, weight_decay=0.01, lr=0.003))
        assert eng.optimizer.name == "adam" and eng.optimizer.lr == 0.003
        assert eng.optimizer.defaults["weight_decay"] == 0.01 and eng.wd == 0.01


def test_vae_loader_matches_the_reference_layout():
    from beta_recsys_amd import data

    users, items = np.array([3, 0, 3, 5, 0, 3]), np.array([1, 2, 1, 0, 4, 6])       # (3, 1) twice; users 1, 2, 4 absent
    user_indices, matrix = data.instance_vae_loader(users, items, 7, 8)
    assert np.array_equal(user_indices, [0, 3, 5]) and matrix.shape == (7, 8)
    dense = np.zeros((7, 8), dtype=np.float32)
    dense[users, items] = 1.0
    assert np.array_equal(matrix.toarray(), dense)
    with pytest.raises(IndexError):
        data.instance_vae_loader([0, 7], [0, 0], 7, 8)


def test_registration():
    import __graft_entry__ as ge
    from beta_recsys_amd import compat

    assert compat.MIRRORS["beta_rec.models.vaecf"] == "vaecf"
    assert ge.EVIDENCE_GROUPS["vaecf"] == ge._EVIDENCE_COMMON + ["vaecf.hip", "ncf.hip", "gemm.hpp"]
    assert ge.evidence_group("vaecf_step") == "vaecf"


def test_reference_predict_restated():
    """``predict`` taken literally is row 0's probabilities at the item ids: pairs of other users change nothing."""
    for case in CASES:
        g = load_golden(case)
        U, I = meta(g)[:2]
        lik, activation = hyper(g)[:2]
        w = vc_params(case, g, 0)
        got = vn.reference_predict(w, g["predict_users"], g["predict_items"], U, I, activation, lik)
        np.testing.assert_allclose(got, g["predict_out"], rtol=REL, atol=0)
        users0 = np.where(g["predict_users"] == 0, 0, 1)                          # move the other users' pairs elsewhere
        moved = vn.reference_predict(w, users0, g["predict_items"], U, I, activation, lik)
        assert np.array_equal(moved, got)


# ---- visibility: a wrong implementation must show on the fixtures --------------------------------------------------------
def _margin(g_wrong, g_ref, g64):
    """Largest distance of a wrong gradient from the exact one, in units of the GPU tests' bound for that tensor."""
    return max(float(np.abs(g_wrong[k] - g64[k]).max() /
                     (REL * np.abs(g64[k]).max() + 2.0 * np.abs(g_ref[k] - g64[k]).max() + 1e-300)) for k in g64)


def test_wrong_variants_are_visible():
    """EPS left out (where fp64 can see it: the likelihoods with a log; and on the LOSS, not only the gradient, where
    p + EPS differs from p); the KL's std taken from ``exp(logvar)``; the mean over the config batch size (on the
    short-batch fixture); the sparse correction dropped; the decay applied after Adam (on the fixtures with a decay)."""
    n_short = n_decay = 0
    for case in CASES:
        g = load_golden(case)
        lik, activation, wd, lr, beta = hyper(g)
        B, bs = meta(g)[3], meta(g)[4]
        for s in range(meta(g)[5]):
            w, x, eps = vc_params(case, g, s), g["x"][s], g[f"eps{s}"]
            g_ref = vc_params(case, g, s + 1, "g")
            g64 = exact_grads(w, x, eps, beta, activation, lik)[3]
            for variant in ("kl_from_logvar", "drop_sparse"):
                m = _margin(exact_grads(w, x, eps, beta, activation, lik, **{variant: True})[3], g_ref, g64)
                print(f"{case} step {s}: {variant} moves a gradient by {m:.1f} bounds")
                assert m > MIN_MARGIN, f"{case} step {s} {variant}"
            if B != bs:
                n_short += 1
                m = _margin(exact_grads(w, x, eps, beta, activation, lik, mean_over=bs)[3], g_ref, g64)
                print(f"{case} step {s}: the mean over the config batch size moves a gradient by {m:.1f} bounds")
                assert m > MIN_MARGIN
            if wd:
                n_decay += 1
                st = vc_opt_state(case, g, s)
                band = vc_band(w, st, g_ref, lr, wd)
                w_bad = {k: v.copy() for k, v in w.items()}
                vn.opt_step(w_bad, g_ref, copy_state(st), lr, wd, decay_after=True)
                w_ref = vc_params(case, g, s + 1)
                with pytest.raises(AssertionError):
                    for k in w:
                        assert_step_close(w[k], w_bad[k], w_ref[k], band[k], what=k)
    assert n_short == 3 and n_decay == 6


def test_eps_left_out_is_visible():
    """``log(p + 1e-10)`` against ``log(p)``: at probabilities around 0.1 the difference is 1e-9 of the loss, far below
    fp32, so on the fixtures the variant cannot show and no test could tell; it shows where a probability underflows.
    One input with a decoder bias of -120 on an item a row holds: ``p`` is 0 there, the reference's loss stays finite
    (``x log(1e-10)``), the variant's is infinite."""
    case = "vaecf_mult_tanh"
    g = load_golden(case)
    lik, activation, _, _, beta = hyper(g)
    w, x, eps = vc_params(case, g, 0), g["x"][0], g["eps0"]
    w["decoder.fc1.bias"][0] = -120.0
    assert x[1, 0] == 1
    loss, ll, _, grads, _ = vn.vaecf_grads(w, x, eps, beta, activation, lik)
    assert np.isfinite(loss) and all(np.isfinite(v).all() for v in grads.values())
    assert ll < x[:, 0].sum() * np.log(1e-10) / x.shape[0] + 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        bad = vn.vaecf_grads(w, x, eps, beta, activation, lik, no_eps=True)[0]
    assert not np.isfinite(bad)
