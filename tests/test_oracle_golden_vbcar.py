"""Pin tests/vbcar_numpy.py against golden vectors captured from the real reference's VBCAREngine by
``tools/gen_golden_vbcar.py``, and the host-side parts of the VBCAR mirror: the noise draw, the constructor, the limits,
the registration, and the checks that a wrong implementation would be VISIBLE on the inputs the GPU tests use.  CPU only."""
import numpy as np
import pytest
import torch

import vbcar_edges as ve
import vbcar_numpy as vn
from helpers import REL, assert_grads_as_accurate, assert_scalar_close, assert_step_close
from helpers import copy_state, float64_oracle, load_golden, to64

CASES = ["vbcar_rmsprop_tanh", "vbcar_adam_relu", "vbcar_sgd_sigmoid_short"]
STATE_NAMES = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg",), "sgd": ()}
STATE_TAGS = {"exp_avg": "m", "exp_avg_sq": "v", "square_avg": "v"}
BATCH_KEYS = ("pos_u", "pos_i_1", "pos_i_2", "neg_u", "neg_i_1", "neg_i_2")
MIN_MARGIN = 2.0      # a wrong implementation must move some gradient by more than this many GPU-test bounds


def meta(g):
    """(U, I, D, L, Fu, Fi, n_neg, B, config batch_size, steps, seed)"""
    return tuple(int(x) for x in g["meta"])


def hyper(g):
    """(optimizer, lr, activator, alpha, scale)"""
    return str(g["optimizer"]), float(g["lr"]), str(g["activator"]), float(g["alpha"]), 1.0 / (3 * meta(g)[8])


def vb_params(case, g, step, tag="w"):
    """Tensor set ``tag`` (w / g / m / v) of the reference after ``step`` steps (w after 0 steps: the initial weights)."""
    if step == 0 and tag == "w":
        return {k: g[f"w0/{k}"].astype(np.float32).copy() for k in vn.KEYS}
    s = load_golden(f"{case}_s{step}")
    return {k: s[f"{tag}/{k}"].astype(np.float32).copy() for k in vn.KEYS}


def vb_fea(g):
    return g["user_fea"], g["item_fea"]


def vb_batch(g, s):
    return tuple(g[k][s] for k in BATCH_KEYS)


def vb_eps(g, s):
    return [g[f"eps{s}/{i}"] for i in range(6)]


def vb_opt_state(case, g, step):
    opt = str(g["optimizer"])
    st = vn.new_opt_state(vb_params(case, g, 0), opt)
    st["step"] = step
    if step > 0:
        for name in STATE_NAMES[opt]:
            st[name] = vb_params(case, g, step, STATE_TAGS[name])
    return st


def exact_grads(w, fea, batch, eps, alpha, scale, activator, **variant):
    with float64_oracle(vn):
        return vn.vbcar_grads(to64(w), fea, batch, eps, alpha, scale, activator, **variant)


def vb_band(w_prev, st_prev, g_ref, opt, lr, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel of its scale of g_ref
    (helpers.optimizer_band's rule on this model's keys)."""
    outs = []
    for sign in (+1.0, -1.0):
        w, st = {k: v.copy() for k, v in w_prev.items()}, copy_state(st_prev)
        gp = {k: (g_ref[k] + np.float32(sign * rel * float(np.abs(g_ref[k]).max()))).astype(np.float32) for k in w}
        vn.opt_step(w, gp, st, opt, lr)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in w_prev}


def model_config(U=9, I=11, D=6, L=10, Fu=7, Fi=5, n_neg=3, batch_size=6, alpha=0.3, activator="tanh", optimizer="adam",
                 lr=1e-3, device="cpu", fea=None):
    fea = fea if fea is not None else (np.zeros((U, Fu), dtype=np.float32), np.zeros((I, Fi), dtype=np.float32))
    return {"model": {"n_users": U, "n_items": I, "late_dim": L, "emb_dim": D, "n_neg": n_neg, "batch_size": batch_size,
                      "alpha": alpha, "activator": activator, "optimizer": optimizer, "lr": lr, "device_str": device},
            "user_fea": fea[0], "item_fea": fea[1], "system": {"run_dir": "/tmp/hiprec_vbcar_runs"}}


def golden_config(g, device="cpu"):
    U, I, D, L, Fu, Fi, n_neg, _, bs, _, _ = meta(g)
    opt, lr, activator, alpha, _ = hyper(g)
    return model_config(U, I, D, L, Fu, Fi, n_neg, bs, alpha, activator, opt, lr, device, vb_fea(g))


def edge_config(shape, optimizer="sgd", lr=0.05, device="cpu", fea=None):
    U, I, D, L, Fu, Fi, B, n_neg, activator, alpha, bs = shape
    return model_config(U, I, D, L, Fu, Fi, n_neg, bs, alpha, activator, optimizer, lr, device, fea)


@pytest.mark.parametrize("case", CASES)
def test_numpy_restatement_matches_reference(case):
    """Every step in isolation from the reference's own weights and optimizer state: the loss and its two parts, every
    gradient (in fp32 as accurate as the reference against the fp64 evaluation), the new weights."""
    g = load_golden(case)
    opt, lr, activator, alpha, scale = hyper(g)
    fea = vb_fea(g)
    for s in range(meta(g)[9]):
        w, st = vb_params(case, g, s), vb_opt_state(case, g, s)
        batch, eps = vb_batch(g, s), vb_eps(g, s)
        loss, gen, kld, grads, _ = vn.vbcar_grads(w, fea, batch, eps, alpha, scale, activator)
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        assert_scalar_close(kld, g["kl_losses"][s], what=f"kl_loss step {s}")
        assert_scalar_close(gen, g["rec_losses"][s], what=f"rec_loss step {s}")
        g_ref = vb_params(case, g, s + 1, "g")
        loss64, gen64, kld64, g64, _ = exact_grads(w, fea, batch, eps, alpha, scale, activator)
        assert_scalar_close(loss64, g["losses"][s], what=f"fp64 loss step {s}")
        assert_scalar_close(kld64, g["kl_losses"][s], what=f"fp64 kl_loss step {s}")
        assert_scalar_close(gen64, g["rec_losses"][s], what=f"fp64 rec_loss step {s}")
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}")
        band = vb_band(w, st, g_ref, opt, lr)
        w_prev = {k: v.copy() for k, v in w.items()}
        vn.opt_step(w, grads, st, opt, lr)
        w_ref = vb_params(case, g, s + 1)
        for k in w:
            assert_step_close(w_prev[k], w[k], w_ref[k], band[k], what=f"weights {k} step {s}")


@pytest.mark.parametrize("case", CASES)
def test_fixtures_are_well_conditioned(case):
    """The two conditions of the fixtures, in the fp64 evaluation at every step: ``min |s| >= 0.25`` over every row a
    batch encodes, and the reference's own gradients within REL of their scale of the exact ones."""
    g = load_golden(case)
    _, _, activator, alpha, scale = hyper(g)
    for s in range(meta(g)[9]):
        batch = vb_batch(g, s)
        ve.check_batch(batch)
        _, _, _, g64, info = exact_grads(vb_params(case, g, s), vb_fea(g), batch, vb_eps(g, s), alpha, scale, activator)
        g_ref = vb_params(case, g, s + 1, "g")
        worst = max(float(np.abs(g_ref[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in g_ref)
        print(f"{case} step {s}: min |s| {info['min_abs_s']:.3f}; the reference's gradients are within {worst:.2e} of "
              f"their scale of the exact ones")
        assert info["min_abs_s"] >= ve.MIN_ABS_S
        assert worst <= REL
    assert g["replay_ok"].all()


@pytest.mark.parametrize("shape", ve.SHAPES, ids=ve.shape_id)
def test_edge_inputs_are_well_conditioned(shape):
    w, fea, batch, eps = ve.synthetic(shape)
    if shape[6] >= 2:
        ve.check_batch(batch)
    activator, alpha, scale = ve.hyper(shape)
    _, _, _, g64, info = exact_grads(w, fea, batch, eps, alpha, scale, activator)
    _, _, _, g32, _ = vn.vbcar_grads(w, fea, batch, eps, alpha, scale, activator)
    worst = max(float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in g64)
    print(f"{ve.shape_id(shape)}: min |s| {info['min_abs_s']:.3f}; the fp32 restatement's gradients are within "
          f"{worst:.2e} of their scale of the exact ones")
    assert info["min_abs_s"] >= ve.MIN_ABS_S
    assert worst <= REL


# ---- noise, constructor, limits, registration ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_draw_noise_is_the_reference_eps_bit_for_bit(case):
    from beta_recsys_amd.vbcar import draw_noise

    g = load_golden(case)
    _, _, D, _, _, _, n_neg, B, _, steps, _ = meta(g)
    for s in range(steps):
        torch.set_rng_state(torch.from_numpy(g[f"rng_state{s}"]))
        noise = draw_noise(B, n_neg, D, "cpu").numpy()
        assert noise.shape == (3 * B * (1 + n_neg), D)
        assert np.array_equal(noise, np.concatenate(vb_eps(g, s)))


@pytest.mark.parametrize("case", CASES)
def test_constructor_reproduces_the_reference_weights(case):
    """Same torch seed, same constructed weights (the fixture's ``winit``: before the conditioning recipe), same
    ``state_dict`` keys, shapes and order; checkpoints load in both directions."""
    import beta_recsys_amd as hp

    g = load_golden(case)
    cfg = golden_config(g)
    torch.manual_seed(meta(g)[10])
    model = hp.VBCAR(cfg["model"], cfg["user_fea"], cfg["item_fea"])
    sd = model.state_dict()
    assert tuple(sd) == vn.KEYS == tuple(n for n, _ in model.named_parameters())
    for k, shape in vn.shapes(*meta(g)[:6]).items():
        assert tuple(sd[k].shape) == shape
        assert np.array_equal(sd[k].numpy(), g[f"winit/{k}"]), k
    model.load_state_dict({k: torch.from_numpy(g[f"w0/{k}"]) for k in vn.KEYS})
    assert np.array_equal(model.flat.numpy(), np.concatenate([g[f"w0/{k}"].ravel() for k in vn.KEYS]))
    ref_like = {k: torch.zeros(shape) for k, shape in vn.shapes(*meta(g)[:6]).items()}
    for k, v in model.state_dict().items():                  # the other direction: a reference module's load_state_dict
        ref_like[k].copy_(v)
    assert model.user_fea.dtype == torch.float32 and "user_fea" not in sd


def test_config_limits_and_value_errors():
    import beta_recsys_amd as hp
    from beta_recsys_amd import vbcar

    def build(**kw):
        cfg = model_config(**kw)
        return hp.VBCAR(cfg["model"], cfg["user_fea"], cfg["item_fea"])

    assert (vbcar.MAX_DIM, vbcar.MAX_LATE) == (128, 512)
    for bad in (dict(D=129), dict(D=0), dict(L=513), dict(L=0), dict(activator="prelu"), dict(n_neg=0), dict(U=0)):
        with pytest.raises(ValueError):
            build(**bad)
    with pytest.raises(ValueError):
        build(fea=(np.zeros((8, 7)), np.zeros((11, 5))))       # one feature row per user
    with pytest.raises(ValueError):
        build(fea=(np.zeros((9, vbcar.MAX_FEA + 1), dtype=np.float32), np.zeros((11, 5))))
    m = build(D=128, L=512, Fu=1030, Fi=3, activator="whatever")    # the limits, any feature width, identity
    assert m.shape.act == 0 and m.user_fea_dim == 1030
    assert build(fea=(np.zeros((9, 7), dtype=np.float64), np.zeros((11, 5), dtype=np.float16))).item_fea.dtype == torch.float32
    assert [build(activator=a).shape.act for a in ("tanh", "sigmoid", "relu", "lrelu")] == [1, 2, 3, 4]


def test_registration():
    import __graft_entry__ as ge
    from beta_recsys_amd import compat

    assert compat.MIRRORS["beta_rec.models.vbcar"] == "vbcar"
    assert ge.EVIDENCE_GROUPS["vbcar"] == ge._EVIDENCE_COMMON + ["vbcar.hip", "ncf.hip", "gemm.hpp"]
    assert ge.evidence_group("vbcar_step") == "vbcar"


# ---- visibility: a wrong implementation must show on the inputs the GPU tests use ---------------------------------------
def _inputs():
    """(name, weights, fea, batch, eps, activator, alpha, scale, B, config batch, reference fp32 gradients) of every
    fixture step and every edge shape."""
    for case in CASES:
        g = load_golden(case)
        _, _, activator, alpha, scale = hyper(g)
        for s in range(meta(g)[9]):
            yield (f"{case} step {s}", vb_params(case, g, s), vb_fea(g), vb_batch(g, s), vb_eps(g, s), activator, alpha,
                   scale, meta(g)[7], meta(g)[8], vb_params(case, g, s + 1, "g"))
    for shape in ve.SHAPES:
        w, fea, batch, eps = ve.synthetic(shape)
        activator, alpha, scale = ve.hyper(shape)
        yield (ve.shape_id(shape), w, fea, batch, eps, activator, alpha, scale, shape[6], shape[10],
               vn.vbcar_grads(w, fea, batch, eps, alpha, scale, activator)[3])


def _margin(g_wrong, g_ref, g64):
    """Largest distance of a wrong gradient from the exact one, in units of the GPU tests' bound for that tensor."""
    return max(float(np.abs(g_wrong[k] - g64[k]).max() /
                     (REL * np.abs(g64[k]).max() + 2.0 * np.abs(g_ref[k] - g64[k]).max() + 1e-300)) for k in g64)


def test_wrong_variants_are_visible():
    """KL from ``exp(0.5 s)`` instead of the raw ``s``; the ``neg_i_1`` / ``neg_i_2`` noise blocks swapped; each
    positive scored against one other vector; ``scale`` from the actual batch (on the short-batch inputs).

    At the default ``alpha = 0.001`` the KL term is a thousandth of the loss.  The KL variant is asserted on every input
    all the same -- it moves ``s`` by orders of magnitude more than the bound there too -- and the inputs are counted."""
    n_all = n_short = 0
    for name, w, fea, batch, eps, activator, alpha, scale, B, bs, g_ref in _inputs():
        g64 = exact_grads(w, fea, batch, eps, alpha, scale, activator)[3]
        n_all += 1
        for variant in ("kl_from_std", "swap_eps", "pos_single"):
            m = _margin(exact_grads(w, fea, batch, eps, alpha, scale, activator, **{variant: True})[3], g_ref, g64)
            print(f"{name}: {variant} moves a gradient by {m:.1f} bounds")
            assert m > MIN_MARGIN, f"{name} {variant}"
        if B != bs:
            n_short += 1
            m = _margin(exact_grads(w, fea, batch, eps, alpha, 1.0 / (3 * B), activator)[3], g_ref, g64)
            print(f"{name}: scale from the actual batch moves a gradient by {m:.1f} bounds")
            assert m > MIN_MARGIN, f"{name} scale"
    assert n_all == 9 + len(ve.SHAPES) and n_short >= 3 + 2
