"""Pin tests/tvbr_numpy.py against golden vectors captured from the real reference's TVBREngine by
``tools/gen_golden_tvbr.py``, and the host-side parts of the TVBR mirror: the noise draw, the constructor, the limits,
the registration, and the checks that a wrong implementation would be VISIBLE on the inputs the GPU tests use.  CPU only."""
import numpy as np
import pytest
import torch

import tvbr_edges as te
import tvbr_numpy as tn
from helpers import EPS32, REL, assert_as_accurate_as_reference, assert_grads_as_accurate, assert_scalar_close
from helpers import assert_step_close, copy_state, float64_oracle, load_golden, to64

CASES = ["tvbr_rmsprop_tanh", "tvbr_adam_relu", "tvbr_sgd_prelu_short"]
STATE_NAMES = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg",), "sgd": ()}
STATE_TAGS = {"exp_avg": "m", "exp_avg_sq": "v", "square_avg": "v"}
BATCH_KEYS = ("pos_u", "pos_i_1", "pos_i_2", "neg_u", "neg_i_1", "neg_i_2", "pos_t", "neg_t")
FORMS = (True, False)  # every row its own t / one t for the whole batch
MIN_MARGIN = 2.0      # a wrong implementation must move some gradient by more than this many GPU-test bounds


def meta(g):
    """(U, I, D, T, Fu, Fi, n_neg, B, config batch_size, steps, seed)"""
    return tuple(int(x) for x in g["meta"])


def hyper(g):
    """(optimizer, lr, activator, alpha, scale)"""
    return str(g["optimizer"]), float(g["lr"]), str(g["activator"]), float(g["alpha"]), 1.0 / (3 * meta(g)[8])


def keys_of(g):
    return tn.keys(str(g["activator"]) == "prelu")


def tv_params(case, g, step, tag="w"):
    """Tensor set ``tag`` (w / g / m / v) of the reference after ``step`` steps (w after 0 steps: the initial weights)."""
    if step == 0 and tag == "w":
        return {k: g[f"w0/{k}"].astype(np.float32).copy() for k in keys_of(g)}
    s = load_golden(f"{case}_s{step}")
    return {k: s[f"{tag}/{k}"].astype(np.float32).copy() for k in keys_of(g)}


def tv_fea(g):
    return g["user_fea"], g["item_fea"]


def tv_batch(g, s):
    return tuple(g[k][s] for k in BATCH_KEYS)


def tv_eps(g, s):
    return [g[f"eps{s}/{i}"] for i in range(6)]


def tv_opt_state(case, g, step):
    opt = str(g["optimizer"])
    st = tn.new_opt_state(tv_params(case, g, 0), opt)
    st["step"] = step
    if step > 0:
        for name in STATE_NAMES[opt]:
            st[name] = tv_params(case, g, step, STATE_TAGS[name])
    return st


def exact_grads(w, fea, batch, eps, alpha, scale, activator, **variant):
    with float64_oracle(tn):
        return tn.tvbr_grads(to64(w), fea, batch, eps, alpha, scale, activator, **variant)


def assert_kl_as_accurate(got, ref, exact, what=""):
    """``kl_loss`` adds up ``log(var2 / var1) - 1 + var1 / var2 + ...`` per row and column: terms of magnitude 1 that
    cancel where prior and posterior are close, so that its fp32 evaluation is ill-conditioned -- the reference's own
    ``kl_loss`` is up to 3.9e-5 of its value away from the fp64 one on the piecewise fixtures (rec_loss and the loss:
    below 1e-7).  It is therefore held to the gradients' rule: within REL of the exact value plus twice the distance the
    reference itself is from it."""
    assert_as_accurate_as_reference(np.float64(got), np.float64(ref), np.float64(exact), what=what)


def tv_band(w_prev, st_prev, g_ref, opt, lr, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel of its scale of g_ref
    (helpers.optimizer_band's rule on this model's keys)."""
    outs = []
    for sign in (+1.0, -1.0):
        w, st = {k: v.copy() for k, v in w_prev.items()}, copy_state(st_prev)
        gp = {k: (g_ref[k] + np.float32(sign * rel * float(np.abs(g_ref[k]).max()))).astype(np.float32) for k in w}
        tn.opt_step(w, gp, st, opt, lr)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in w_prev}


def model_config(U=9, I=11, D=6, T=4, Fu=7, Fi=5, n_neg=3, batch_size=6, alpha=0.3, activator="tanh", optimizer="adam",
                 lr=1e-3, device="cpu", fea=None):
    fea = fea if fea is not None else (np.zeros((U, Fu), dtype=np.float32), np.zeros((I, Fi), dtype=np.float32))
    return {"model": {"n_users": U, "n_items": I, "late_dim": 10, "emb_dim": D, "n_neg": n_neg, "time_step": T,
                      "batch_size": batch_size, "alpha": alpha, "activator": activator, "optimizer": optimizer, "lr": lr,
                      "device_str": device},
            "user_fea": fea[0], "item_fea": fea[1], "system": {"run_dir": "/tmp/hiprec_tvbr_runs"}}


def golden_config(g, device="cpu"):
    U, I, D, T, Fu, Fi, n_neg, _, bs, _, _ = meta(g)
    opt, lr, activator, alpha, _ = hyper(g)
    return model_config(U, I, D, T, Fu, Fi, n_neg, bs, alpha, activator, opt, lr, device, tv_fea(g))


def edge_config(shape, optimizer="sgd", lr=0.05, device="cpu", fea=None):
    U, I, D, T, Fu, Fi, B, n_neg, activator, alpha, bs = shape
    return model_config(U, I, D, T, Fu, Fi, n_neg, bs, alpha, activator, optimizer, lr, device, fea)


def form_id(mixed):
    return "mixed-t" if mixed else "one-t"


@pytest.mark.parametrize("case", CASES)
def test_numpy_restatement_matches_reference(case):
    """Every step in isolation from the reference's own weights and optimizer state: the loss and its two parts, every
    gradient (in fp32 as accurate as the reference against the fp64 evaluation), the new weights."""
    g = load_golden(case)
    opt, lr, activator, alpha, scale = hyper(g)
    fea = tv_fea(g)
    for s in range(meta(g)[9]):
        w, st = tv_params(case, g, s), tv_opt_state(case, g, s)
        batch, eps = tv_batch(g, s), tv_eps(g, s)
        loss, rec, kl, grads, _ = tn.tvbr_grads(w, fea, batch, eps, alpha, scale, activator)
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        assert_scalar_close(rec, g["rec_losses"][s], what=f"rec_loss step {s}")
        g_ref = tv_params(case, g, s + 1, "g")
        loss64, rec64, kl64, g64, info = exact_grads(w, fea, batch, eps, alpha, scale, activator)
        assert_kl_as_accurate(kl, g["kl_losses"][s], kl64, what=f"kl_loss step {s}")
        assert_scalar_close(loss64, g["losses"][s], what=f"fp64 loss step {s}")
        # the reference's fp32 kl_loss against the exact one: an fp32 sum of terms whose magnitudes add up to kl_terms
        kl_err, kl_tol = abs(kl64 - float(g["kl_losses"][s])), REL * abs(kl64) + 8 * EPS32 * info["kl_terms"]
        print(f"{case} step {s}: kl_loss {kl64!r}, the reference's is {kl_err:.2e} away (bound {kl_tol:.2e}, terms "
              f"{info['kl_terms']:.2f})")
        assert kl_err <= kl_tol
        assert_scalar_close(rec64, g["rec_losses"][s], what=f"fp64 rec_loss step {s}")
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}")
        band = tv_band(w, st, g_ref, opt, lr)
        w_prev = {k: v.copy() for k, v in w.items()}
        tn.opt_step(w, grads, st, opt, lr)
        w_ref = tv_params(case, g, s + 1)
        for k in w:
            assert_step_close(w_prev[k], w[k], w_ref[k], band[k], what=f"weights {k} step {s}")


@pytest.mark.parametrize("case", CASES)
def test_fixtures_are_well_conditioned(case):
    """The conditions of the fixtures, in the fp64 evaluation at every step: the batch holds every collision, every
    pre-activation of a piecewise activator is ``MIN_KINK_GAP`` from a kink, the reference's own gradients are within REL
    of their scale of the exact ones, the time table is off the identity, steps 0 and 1 mix ``t`` and step 2 does not."""
    g = load_golden(case)
    U, I, _, T = meta(g)[:4]
    _, _, activator, alpha, scale = hyper(g)
    assert float(np.abs(g["w0/time_embdding.weight"] - np.eye(T + 1)).max()) > 0.05
    assert np.array_equal(g["winit/time_embdding.weight"], np.eye(T + 1, dtype=np.float32))
    for s in range(meta(g)[9]):
        batch = tv_batch(g, s)
        te.check_batch(batch, U, I, T, mixed=s < 2)
        _, _, _, g64, info = exact_grads(tv_params(case, g, s), tv_fea(g), batch, tv_eps(g, s), alpha, scale, activator)
        g_ref = tv_params(case, g, s + 1, "g")
        worst = max(float(np.abs(g_ref[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in g_ref)
        print(f"{case} step {s}: min kink gap {info['min_kink_gap']:.3f}; the reference's gradients are within "
              f"{worst:.2e} of their scale of the exact ones")
        assert info["min_kink_gap"] >= te.MIN_KINK_GAP
        assert worst <= REL
        for row in te.unused_time_rows(batch, T):
            assert not g_ref["time_embdding.weight"][row].any(), "the reference's gradient reaches an unused time row"
    assert g["replay_ok"].all()


@pytest.mark.parametrize("mixed", FORMS, ids=form_id)
@pytest.mark.parametrize("shape", te.SHAPES, ids=te.shape_id)
def test_edge_inputs_are_well_conditioned(shape, mixed):
    w, fea, batch, eps = te.synthetic(shape, mixed)
    U, I, _, T = shape[:4]
    te.check_batch(batch, U, I, T, mixed)
    activator, alpha, scale = te.hyper(shape)
    _, _, _, g64, info = exact_grads(w, fea, batch, eps, alpha, scale, activator)
    _, _, _, g32, _ = tn.tvbr_grads(w, fea, batch, eps, alpha, scale, activator)
    worst = max(float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in g64)
    print(f"{te.shape_id(shape)} {form_id(mixed)}: min kink gap {info['min_kink_gap']:.3f}; the fp32 restatement's "
          f"gradients are within {worst:.2e} of their scale of the exact ones")
    assert info["min_kink_gap"] >= te.MIN_KINK_GAP
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
        assert np.array_equal(noise, np.concatenate(tv_eps(g, s)))


@pytest.mark.parametrize("case", CASES)
def test_constructor_reproduces_the_reference_weights(case):
    """Same torch seed, same constructed weights (the fixture's ``winit``), same ``state_dict`` keys, shapes and order
    -- under prelu with the four ``.1.weight`` slopes; checkpoints load in both directions."""
    import beta_recsys_amd as hp

    g = load_golden(case)
    keys = keys_of(g)
    cfg = golden_config(g)
    torch.manual_seed(meta(g)[10])
    model = hp.TVBR(cfg["model"], cfg["user_fea"], cfg["item_fea"])
    sd = model.state_dict()
    assert tuple(sd) == keys == tuple(n for n, _ in model.named_parameters())
    assert ("time2std_i.1.weight" in keys) == (case == "tvbr_sgd_prelu_short") and "time_embdding.weight" in keys
    shapes = tn.shapes(*meta(g)[:6], prelu=str(g["activator"]) == "prelu")
    for k, shape in shapes.items():
        assert tuple(sd[k].shape) == shape
        assert np.array_equal(sd[k].numpy(), g[f"winit/{k}"]), k
    model.load_state_dict({k: torch.from_numpy(g[f"w0/{k}"]) for k in keys})
    assert np.array_equal(model.flat.numpy(), np.concatenate([g[f"w0/{k}"].ravel() for k in keys]))
    ref_like = {k: torch.zeros(shape) for k, shape in shapes.items()}
    for k, v in model.state_dict().items():                  # the other direction: a reference module's load_state_dict
        ref_like[k].copy_(v)
    assert model.user_fea.dtype == torch.float32 and "user_fea" not in sd


def test_config_limits_and_value_errors():
    import beta_recsys_amd as hp
    from beta_recsys_amd import tvbr

    def build(**kw):
        cfg = model_config(**kw)
        return hp.TVBR(cfg["model"], cfg["user_fea"], cfg["item_fea"])

    assert (tvbr.MAX_DIM, tvbr.MAX_FEA, tvbr.MAX_TIME) == (128, 65536, 255)
    for bad in (dict(D=129), dict(D=0), dict(T=256), dict(T=0), dict(activator="none"), dict(activator="elu"),
                dict(n_neg=0), dict(U=0)):
        with pytest.raises(ValueError):
            build(**bad)
    with pytest.raises(ValueError):
        build(fea=(np.zeros((8, 7)), np.zeros((11, 5))))       # one feature row per user
    with pytest.raises(ValueError):
        build(fea=(np.zeros((9, tvbr.MAX_FEA + 1), dtype=np.float32), np.zeros((11, 5))))
    m = build(D=128, T=255, Fu=1030, Fi=3, activator="prelu")    # the limits, any feature width
    assert m.shape.act == 7 and m.user_fea_dim == 1030 and m.shape.time_step == 255
    assert build(fea=(np.zeros((9, 7), dtype=np.float64), np.zeros((11, 5), dtype=np.float16))).item_fea.dtype == torch.float32
    names = ("tanh", "hardtanh", "logsigmoid", "sigmoid", "relu", "lrelu", "prelu")
    assert names == tn.ACTIVATORS and [build(activator=a).shape.act for a in names] == [1, 2, 3, 4, 5, 6, 7]
    cfg = model_config()
    del cfg["model"]["late_dim"]                                 # read nowhere
    hp.TVBR(cfg["model"], cfg["user_fea"], cfg["item_fea"])


def test_registration():
    import __graft_entry__ as ge
    import beta_recsys_amd as hp
    from beta_recsys_amd import compat

    assert compat.MIRRORS["beta_rec.models.tvbr"] == "tvbr"
    assert ge.EVIDENCE_GROUPS["tvbr"] == ge._EVIDENCE_COMMON + ["tvbr.hip", "ncf.hip", "gemm.hpp"]
    assert ge.evidence_group("tvbr_step") == "tvbr"
    assert hp.TVBREngine.__module__ == "beta_recsys_amd.tvbr"


def test_library_rejects_shapes_beyond_the_limits():
    """The C entry points themselves (no GPU is touched): declared, bound and exported; a shape beyond a limit is -1 /
    0 bytes with the limit named in ``hiprec_last_error``; the flat layout of a good shape is the Python one."""
    import ctypes
    import os

    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hiprec.h")).read()
    lib = _lib.load()
    for name in ("hiprec_tvbr_shape_bytes", "hiprec_tvbr_param_floats", "hiprec_tvbr_workspace_bytes", "hiprec_tvbr_grad",
                 "hiprec_tvbr_encode_workspace_bytes", "hiprec_tvbr_encode", "hiprec_tvbr_predict"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "#define HIPREC_STATUS_TIME_OOB 128u" in header and _lib.STATUS_TIME_OOB == 128
    assert lib.hiprec_tvbr_shape_bytes() == ctypes.sizeof(_lib.TvbrShape)

    def shape(U=9, I=11, D=6, T=4, Fu=7, Fi=5, act=1):
        return ctypes.byref(_lib.TvbrShape(U, I, D, T, Fu, Fi, act, 0))

    for bad, word in ((dict(D=129), b"emb_dim"), (dict(D=0), b"emb_dim"), (dict(T=256), b"time_step"),
                      (dict(T=0), b"time_step"), (dict(Fu=65537), b"feature"), (dict(Fi=0), b"feature"),
                      (dict(act=0), b"activation"), (dict(act=8), b"activation"), (dict(U=0), b"n_users")):
        assert lib.hiprec_tvbr_param_floats(shape(**bad)) == -1 and word in lib.hiprec_last_error(), bad
        assert lib.hiprec_tvbr_workspace_bytes(shape(**bad), 6, 3) == 0
        assert lib.hiprec_tvbr_encode_workspace_bytes(shape(**bad), 6, 1) == 0
    assert lib.hiprec_tvbr_workspace_bytes(shape(), 0, 3) == 0 and lib.hiprec_tvbr_workspace_bytes(shape(), 6, -1) == 0
    assert lib.hiprec_tvbr_workspace_bytes(shape(D=128, T=255, Fu=65536, Fi=65536), 1 << 14, 5) == 0    # 2^31 elements
    assert b"2^31" in lib.hiprec_last_error()
    assert lib.hiprec_tvbr_workspace_bytes(shape(D=128, T=255, Fu=65536, Fi=65536), 256, 5) > 0
    for activator in ("tanh", "prelu"):
        cfg = model_config(activator=activator)
        m = hp.TVBR(cfg["model"], cfg["user_fea"], cfg["item_fea"])
        assert lib.hiprec_tvbr_param_floats(ctypes.byref(m.shape)) == m.flat.numel()
        assert m.flat.numel() == sum(int(np.prod(s)) for s in tn.shapes(9, 11, 6, 4, 7, 5, activator == "prelu").values())


# ---- visibility: a wrong implementation must show on the inputs the GPU tests use ---------------------------------------
def _inputs():
    """(name, weights, fea, batch, eps, activator, alpha, scale, B, config batch, reference fp32 gradients) of every
    fixture step and every edge shape in both forms."""
    for case in CASES:
        g = load_golden(case)
        _, _, activator, alpha, scale = hyper(g)
        for s in range(meta(g)[9]):
            yield (f"{case} step {s}", tv_params(case, g, s), tv_fea(g), tv_batch(g, s), tv_eps(g, s), activator, alpha,
                   scale, meta(g)[7], meta(g)[8], tv_params(case, g, s + 1, "g"))
    for shape in te.SHAPES:
        for mixed in FORMS:
            w, fea, batch, eps = te.synthetic(shape, mixed)
            activator, alpha, scale = te.hyper(shape)
            yield (f"{te.shape_id(shape)} {form_id(mixed)}", w, fea, batch, eps, activator, alpha, scale, shape[6],
                   shape[10], tn.tvbr_grads(w, fea, batch, eps, alpha, scale, activator)[3])


def _margin(g_wrong, g_ref, g64):
    """Largest distance of a wrong gradient from the exact one, in units of the GPU tests' bound for that tensor."""
    return max(float(np.abs(g_wrong[k] - g64[k]).max() /
                     (REL * np.abs(g64[k]).max() + 2.0 * np.abs(g_ref[k] - g64[k]).max() + 1e-300)) for k in g64)


def test_wrong_variants_are_visible():
    """``z`` from ``std`` directly; prior and posterior time rows swapped; the time table taken as one-hot; the KL sign;
    the negative groups' KL mean over ``B``; ``scale`` from the actual batch (on the short-batch inputs).

    The two KL variants are asserted where ``alpha >= 0.3`` and printed elsewhere (at the default ``alpha = 0.001`` the
    KL term is a thousandth of the loss); the inputs are counted."""
    n_all = n_kl = n_short = 0
    for name, w, fea, batch, eps, activator, alpha, scale, B, bs, g_ref in _inputs():
        g64 = exact_grads(w, fea, batch, eps, alpha, scale, activator)[3]
        n_all += 1
        for variant in ("z_from_std", "swap_time", "time_onehot", "kl_sign", "neg_kl_over_b"):
            m = _margin(exact_grads(w, fea, batch, eps, alpha, scale, activator, **{variant: True})[3], g_ref, g64)
            print(f"{name}: {variant} moves a gradient by {m:.1f} bounds")
            if variant.startswith(("kl_", "neg_kl")) and alpha < 0.3:
                continue
            if variant == "neg_kl_over_b" and batch[3].size == B:
                continue      # n_neg = 1: B n_neg is B, the variant IS the reference
            n_kl += variant == "kl_sign"
            assert m > MIN_MARGIN, f"{name} {variant}"
        if B != bs:
            n_short += 1
            m = _margin(exact_grads(w, fea, batch, eps, alpha, 1.0 / (3 * B), activator)[3], g_ref, g64)
            print(f"{name}: scale from the actual batch moves a gradient by {m:.1f} bounds")
            assert m > MIN_MARGIN, f"{name} scale"
    assert n_all == 9 + 2 * len(te.SHAPES) and n_kl == 6 + 2 * 7 and n_short == 3 + 2 * 2
