"""GPU parity tests of VAECF (csrc/vaecf.hip): forward + loss + backward, the full step and chained steps vs golden
vectors from the real reference's VAECFEngine (tests/golden/vaecf_*.npz) with the captured noise injected; synthetic
shapes that straddle every kernel constant (tests/vaecf_edges.py) against the fp64 restatement; the epoch loop and its
log line; predict / score / ranking_factors / recommend; the bounds check; the ValueError cases; the checkpoint round
trip; the struct size; and the workspace condition that shows no [B, n_items] buffer exists.

No gradient is bit-reproducible between runs and no test asks for that: the last layer's backward adds its tiles up
with atomics, and every other gradient is downstream of its dHd.  The two loss parts are sums in a fixed order and are
compared bitwise between two runs."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

import topk_reference as tk
import vaecf_edges as ve
import vaecf_numpy as vn
from helpers import assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_step_close
from helpers import assert_tensor_close, float64_oracle, load_golden, oracle_trajectory, to64
from test_oracle_golden_vaecf import CASES, edge_config, exact_grads, golden_config, hyper, keys_of, meta, vc_band
from test_oracle_golden_vaecf import vc_opt_state, vc_params

pytestmark = pytest.mark.gpu


def engine_for(cfg, w=None):
    import beta_recsys_amd as hp

    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.VAECFEngine(cfg)
    if w is not None:
        load_weights(eng, w)
    return eng


def golden_engine(case, g, **extra):
    return engine_for(golden_config(g, device="cuda:0", **extra), vc_params(case, g, 0))


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def load_opt_state(eng, st):
    eng.load_optimizer_state(st["step"], st.get("exp_avg"), st.get("exp_avg_sq"))


def np_grads(grads):
    return {k: v.cpu().numpy() for k, v in grads.items()}


def report(grads, g_ref, g64):
    for k in g64:
        print(f"  grad {k}: err vs exact {np.abs(grads[k].reshape(g64[k].shape) - g64[k]).max():.3e}, reference's own "
              f"{np.abs(g_ref[k] - g64[k]).max():.3e}, scale {np.abs(g64[k]).max():.3e}")


def untouched_columns_are_zero(grads, x, what):
    untouched = np.flatnonzero((x != 0).sum(0) == 0)
    assert float(np.abs(grads["encoder.fc0.weight"][:, untouched]).max(initial=0.0)) == 0.0, \
        f"{what}: a gradient reached a W0 column no row touches"
    return len(untouched)


@pytest.mark.parametrize("gather", ["strided", "shadow"])
@pytest.mark.parametrize("case", CASES)
def test_step_matches_reference(hip_device, case, gather):
    """Each step from the reference's own weights and optimizer state, its captured noise injected, with either form of
    the first layer's gather: the loss and its two parts, every gradient (as accurate as the reference against the fp64
    evaluation), W0 columns of untouched items exactly zero, the gradient buffer cleared after the sweep, the stepped
    weights inside the band."""
    g = load_golden(case)
    lik, activation, wd, lr, beta = hyper(g)
    eng = golden_engine(case, g, w0_gather=gather)
    for s in range(meta(g)[5]):
        x, eps = g["x"][s], g[f"eps{s}"]
        w0, st0 = vc_params(case, g, s), vc_opt_state(case, g, s)
        load_weights(eng, w0)
        load_opt_state(eng, st0)
        eng.model.next_noise = eps
        loss, grads = eng.backward_only(torch.from_numpy(x))
        grads = np_grads(grads)
        print(f"{case} step {s}: loss {loss!r} vs {float(g['losses'][s])!r}, ll {eng.model.ll!r} vs "
              f"{float(g['lls'][s])!r}, kld {eng.model.kld!r} vs {float(g['klds'][s])!r}")
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        assert_scalar_close(eng.model.ll, g["lls"][s], what=f"ll step {s}")
        assert_scalar_close(eng.model.kld, g["klds"][s], what=f"kld step {s}")
        g_ref = vc_params(case, g, s + 1, "g")
        g64 = exact_grads(w0, x, eps, beta, activation, lik)[3]
        report(grads, g_ref, g64)
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}")
        assert untouched_columns_are_zero(grads, x, f"step {s}") >= 1, "the fixture leaves an item out"
        assert float(eng._g_flat.abs().max()) == 0.0
        assert eng.model.next_noise is None, "injected noise serves one step"
        # the full step, the batch as a CSR triple this time
        load_opt_state(eng, st0)
        eng.model.next_noise = torch.from_numpy(eps)
        loss = eng.train_single_batch(vn.csr_of(x))
        assert isinstance(loss, float)
        assert_scalar_close(loss, g["losses"][s], what=f"loss (step) {s}")
        band = vc_band(w0, st0, g_ref, lr, wd)
        w1, w_ref = get_weights(eng), vc_params(case, g, s + 1)
        for k in w_ref:
            assert_step_close(w0[k], w1[k], w_ref[k], band[k], what=f"weights {k} step {s}")
        assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"


@pytest.mark.parametrize("case", CASES)
def test_trajectory_matches_reference(hip_device, case):
    """Three steps chained from w0: every element inside the oracle's perturbed-gradient envelope around the reference's
    end point."""
    g = load_golden(case)
    lik, activation, wd, lr, beta = hyper(g)
    steps = meta(g)[5]
    eng = golden_engine(case, g)
    w0 = vc_params(case, g, 0)
    batches = [(g["x"][s], g[f"eps{s}"]) for s in range(steps)]
    for s, (x, eps) in enumerate(batches):
        eng.model.next_noise = eps
        loss = eng.train_single_batch(torch.from_numpy(x))
        print(f"{case} chained step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        if s == 0:
            assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
    _, env, upd = oracle_trajectory(
        w0, batches, lambda w, b: vn.vaecf_grads(w, b[0], b[1], beta, activation, lik)[3],
        lambda w, gr, st: vn.opt_step(w, gr, st, lr, wd), lambda w: vn.new_opt_state(w, "adam"))
    assert_on_trajectory(get_weights(eng), vc_params(case, g, steps), env, upd, f"{case} trajectory")


@pytest.mark.parametrize("shape", ve.SHAPES, ids=ve.shape_id)
def test_shapes_against_the_restatement(hip_device, shape):
    """Loss, its parts, gradients, the inference encoder and the decoded entries at the shapes of vaecf_edges.py against
    the restatement in fp64, as accurate as its fp32 self; what is summed in a fixed order bitwise equal in two runs."""
    I, hidden, Z, B, activation, likelihood, valued = shape
    w, x, eps = ve.synthetic(shape)
    eng = engine_for(edge_config(shape, device="cuda:0"), w)
    g32 = vn.vaecf_grads(w, x, eps, ve.BETA, activation, likelihood)[3]
    loss64, ll64, kld64, g64, info64 = exact_grads(w, x, eps, ve.BETA, activation, likelihood)
    floor = ll_floor(info64, x, likelihood)
    eng.model.next_noise = eps
    loss, grads = eng.backward_only(vn.csr_of(x))
    grads = np_grads(grads)
    parts = (eng.model.ll, eng.model.kld)
    print(f"{ve.shape_id(shape)}: loss {loss!r} vs exact {loss64!r}")
    report(grads, g32, g64)
    assert_tensor_close([loss], [loss64], what="loss", scale_floor=floor)
    assert_tensor_close([eng.model.ll], [ll64], what="ll", scale_floor=floor)
    assert_scalar_close(eng.model.kld, kld64, what="kld")
    assert_grads_as_accurate(grads, g32, g64, what="grad")
    untouched_columns_are_zero(grads, x, ve.shape_id(shape))
    eng.model.next_noise = eps
    again = np_grads(eng.backward_only(torch.from_numpy(x))[1])          # the dense form of the same batch
    assert parts == (eng.model.ll, eng.model.kld), "the loss parts are fixed-order sums"
    assert_grads_as_accurate(again, g32, g64, what="grad (dense batch)")
    # inference
    with float64_oracle(vn):
        p64, hd64 = vn.predict_scores(to64(w), x, activation, likelihood)
        mu64 = vn.encode(to64(w), x.astype(np.float64), activation)[0]
    mu, hd = eng.model.encode(torch.from_numpy(x))
    assert tuple(mu.shape) == (B, Z) and tuple(hd.shape) == (B, hidden[0])
    assert_tensor_close(mu.cpu().numpy(), mu64, what="mu")
    assert_tensor_close(hd.cpu().numpy(), hd64, what="Hd(mu)")
    rows, items = np.repeat(np.arange(B), min(I, 3)), np.tile(np.array([0, I // 2, I - 1])[:min(I, 3)], B)
    got = eng.model.decode(hd, rows, items).cpu().numpy()
    assert_tensor_close(got, p64[rows, items], what="decoded entries")


def ll_floor(info, x, likelihood):
    """Scale floor of ``ll`` (and of the loss that holds it) for ``mult``: ``log p_bi`` is the difference ``logit_bi -
    lse_b``, so its fp32 rounding error is relative to the two terms, not to the (possibly cancelled) result -- with one
    item in the catalogue ``ll`` is 1e-10 while the logit is of order one (helpers.grad_scale_floor's reasoning)."""
    if likelihood != "mult":
        return 0.0
    logits = info["logits"]
    m = logits.max(1, keepdims=True)
    lse = m + np.log(np.exp(logits - m).sum(1, keepdims=True))
    return float((np.abs(x) * (np.abs(logits) + np.abs(lse))).sum() / x.shape[0])


def test_eps_sits_where_the_reference_puts_it(hip_device):
    """The input of test_eps_left_out_is_visible: a probability that underflows on an item a row holds.  The loss is
    finite and equals the restatement's (``x log(0 + 1e-10)``), the gradients are finite and as accurate."""
    case = "vaecf_mult_tanh"
    g = load_golden(case)
    lik, activation, _, _, beta = hyper(g)
    w, x, eps = vc_params(case, g, 0), g["x"][0], g["eps0"]
    w["decoder.fc1.bias"][0] = -120.0
    eng = golden_engine(case, g)
    load_weights(eng, w)
    g32 = vn.vaecf_grads(w, x, eps, beta, activation, lik)[3]
    loss64, ll64, _, g64, _ = exact_grads(w, x, eps, beta, activation, lik)
    eng.model.next_noise = eps
    loss, grads = eng.backward_only(torch.from_numpy(x))
    assert np.isfinite(loss)
    assert_scalar_close(loss, loss64, what="loss")
    assert_scalar_close(eng.model.ll, ll64, what="ll")
    assert_grads_as_accurate(np_grads(grads), g32, g64, what="grad")


def test_epoch_follows_the_reference_loop(hip_device):
    """``train_an_epoch`` on the fixture's 9-user matrix at batch size 6 (a short last batch), values 3 binarised, the
    noise from ``draw_noise`` under the fixture's RNG state: the printed line and the logged scalar against the
    reference's, the end weights on the restatement's trajectory, the matrix remembered as the history."""
    from scipy.sparse import csr_matrix

    case = "vaecf_mult_tanh"
    g = load_golden(case)
    lik, activation, wd, lr, beta = hyper(g)
    U, bs = meta(g)[0], meta(g)[4]
    eng = golden_engine(case, g)
    matrix = csr_matrix(g["epoch_matrix"] * 3.0)
    torch.set_rng_state(torch.from_numpy(g["epoch_rng_state"]))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        eng.train_an_epoch((np.arange(U), matrix), 7)
    line = [ln for ln in out.getvalue().splitlines() if ln.startswith("[Training Epoch 7], Loss ")]
    assert len(line) == 1
    print(f"printed {line[0]!r}; the reference printed {str(g['epoch_printed'])!r}")
    assert_scalar_close(float(line[0].split("Loss ")[1]), g["epoch_loss"], what="printed loss")
    tag, value, step = eng.writer.scalars[-1]
    assert (tag, step) == ("model/loss", 7)
    assert_scalar_close(value, g["epoch_loss"], what="logged loss")
    # the same epoch through the restatement, for the envelope
    from beta_recsys_amd.vaecf import draw_noise

    torch.set_rng_state(torch.from_numpy(g["epoch_rng_state"]))
    xb = [g["epoch_matrix"][s:s + bs] for s in range(0, U, bs)]
    batches = [(x, draw_noise(len(x), meta(g)[2], "cpu").numpy()) for x in xb]
    assert [len(x) for x in xb] == [6, 3]
    _, env, upd = oracle_trajectory(
        vc_params(case, g, 0), batches, lambda w, b: vn.vaecf_grads(w, b[0], b[1], beta, activation, lik)[3],
        lambda w, gr, st: vn.opt_step(w, gr, st, lr, wd), lambda w: vn.new_opt_state(w, "adam"))
    ref_end = {k: g[f"epoch_w/{k}"] for k in keys_of(g)}
    assert_on_trajectory(get_weights(eng), ref_end, env, upd, "epoch end")
    # a second epoch reuses the upload; a subset of users in another order goes through the gather of rows
    assert eng._epoch_cache[0] is matrix and eng.model._history is not None
    with contextlib.redirect_stdout(io.StringIO()):
        eng.train_an_epoch((np.array([4, 1, 8]), matrix), 8)
    assert eng.writer.scalars[-1][2] == 8 and np.isfinite(eng.writer.scalars[-1][1])


@pytest.mark.parametrize("case", CASES)
def test_predict_reproduces_the_reference(hip_device, case):
    g = load_golden(case)
    eng = golden_engine(case, g)
    got = eng.model.predict(g["predict_users"], torch.from_numpy(g["predict_items"]))
    assert got.dtype == torch.float32 and tuple(got.shape) == g["predict_out"].shape
    print(f"{case}: predict {got.cpu().numpy()} vs {g['predict_out']}")
    assert_tensor_close(got.cpu().numpy(), g["predict_out"], what="predict")
    assert got[0] == got[1], "the duplicate pair"
    with pytest.raises(ValueError):
        eng.model.predict([0, 1], [0])
    with pytest.raises(IndexError):
        eng.model.predict([0], [meta(g)[1]])


@pytest.mark.parametrize("case", ["vaecf_mult_tanh", "vaecf_bern_relu_wd"])
def test_score_ranking_factors_and_recommend(hip_device, case):
    """Against the fp64 restatement: per-pair scores from each user's history row; the factors; the top-K through
    tests/topk_reference.py, which compares ids only where the reference scores are separated by more than the bound."""
    g = load_golden(case)
    U, I = meta(g)[:2]
    lik, activation = hyper(g)[:2]
    n = len(meta(g)[7])
    w = vc_params(case, g, 0)
    eng = golden_engine(case, g)
    with pytest.raises(NotImplementedError, match="set_history"):
        eng.model.ranking_factors()
    with pytest.raises(NotImplementedError):
        eng.recommend([0], 3)
    history = ve.make_x(np.random.default_rng(11), U, I)
    eng.model.set_history(vn.csr_of(history * 2.0))                      # binarised
    with float64_oracle(vn):
        p64, hd64 = vn.predict_scores(to64(w), history, activation, lik)
    logits64 = hd64 @ w[f"decoder.fc{n}.weight"].astype(np.float64).T + w[f"decoder.fc{n}.bias"]
    users, items = np.repeat(np.arange(U), I)[::-1].copy(), np.tile(np.arange(I), U)
    got = eng.model.score(users.tolist(), torch.from_numpy(items))
    assert got.dtype == torch.float32 and tuple(got.shape) == (U * I,)
    assert_tensor_close(got.cpu().numpy(), p64[users, items], what="score")
    Uf, If, a, bias = eng.model.ranking_factors()
    assert a == 1.0 and tuple(Uf.shape) == (U, 20) and tuple(If.shape) == (I, 20) and tuple(bias.shape) == (I,)
    assert_tensor_close(Uf.cpu().numpy(), hd64, what="user factors")
    assert np.array_equal(If.cpu().numpy(), w[f"decoder.fc{n}.weight"]) and np.array_equal(bias.cpu().numpy(),
                                                                                           w[f"decoder.fc{n}.bias"])
    k = 5
    q = np.array([3, 0, 8, 3])
    got_i, got_s = eng.recommend(q, k)
    tk.check_against_float64(got_i.cpu().numpy(), got_s.cpu().numpy(), logits64[q], None, "recommend")
    seen_u, seen_i = np.nonzero(history)
    got_i, got_s = eng.recommend(q, 3, seen=(seen_u, seen_i))
    seen = [np.flatnonzero(history[u]) for u in q]
    tk.check_against_float64(got_i.cpu().numpy(), got_s.cpu().numpy(), logits64[q], seen, "recommend with seen")
    with pytest.raises(ValueError):
        eng.model.score([0, 1], [0])
    with pytest.raises(IndexError):
        eng.model.score([U], [0])
    with pytest.raises(IndexError):
        eng.model.score([0], [I])


def test_out_of_range_items_raise_and_leave_the_engine_usable(hip_device):
    case = "vaecf_mult_tanh"
    g = load_golden(case)
    I = meta(g)[1]
    eng = golden_engine(case, g)
    x = g["x"][0]
    row_ptr, items, values = vn.csr_of(x)
    before = eng.model.flat.clone()
    for value in (I, -1, I + 1000):
        bad = items.copy()
        bad[-1] = value
        eng.model.next_noise = g["eps0"]
        with pytest.raises(IndexError):
            eng.backward_only((row_ptr, bad, values))
        assert torch.equal(eng.model.flat, before), "the weights moved"
        assert float(eng._g_flat.abs().max()) == 0.0, "a partial gradient was kept"
    bad = items.copy()
    bad[0] = I + 7
    with pytest.raises(IndexError):
        eng.train_single_batch((row_ptr, bad))
    assert float(eng._g_flat.abs().max()) == 0.0
    short_ptr = row_ptr.copy()
    short_ptr[-1] += 5                                             # a row that runs past the arrays
    with pytest.raises(IndexError):
        eng.train_single_batch((short_ptr, items, values))
    with pytest.raises(IndexError):
        eng.model.encode((row_ptr, bad))
    load_weights(eng, vc_params(case, g, 0))
    eng.load_optimizer_state(0)
    eng.model.next_noise = g["eps0"]
    loss = eng.train_single_batch((row_ptr, items, values))
    assert_scalar_close(loss, g["losses"][0], what="loss after the errors")


def test_value_errors(hip_device):
    """What the reference cannot run, and what is beyond the library's limits."""
    case = "vaecf_mult_tanh"
    g = load_golden(case)
    eng = golden_engine(case, g)
    x = g["x"][0]
    for extra in (dict(activation="prelu"), dict(likelihood="normal"), dict(z_dim=257), dict(hidden=[513]),
                  dict(hidden=[4, 4, 4, 4]), dict(hidden=[])):
        cfg = golden_config(g, device="cuda:0")
        cfg["model"].update(extra)
        with pytest.raises(ValueError):
            engine_for(cfg)
    for bad in (x[:, :-1], x[0], (np.array([0]), np.array([], dtype=np.int64)),
                (np.array([0, 1]), np.array([0]), np.array([1.0, 1.0])), (np.array([0, 1]),)):
        with pytest.raises(ValueError):
            eng.train_single_batch(bad if isinstance(bad, tuple) else torch.from_numpy(bad))
    eng.model.next_noise = g["eps0"][:-1]
    with pytest.raises(ValueError):
        eng.train_single_batch(torch.from_numpy(x))
    eng.model.next_noise = g["eps0"]
    assert_scalar_close(eng.train_single_batch(torch.from_numpy(x)), g["losses"][0], what="loss after the errors")


def test_device_noise_and_forward(hip_device):
    """``noise_rng = "device"`` draws on the GPU (kept as ``last_noise``); ``forward`` returns the loss of that noise."""
    case = "vaecf_pois_relu6"
    g = load_golden(case)
    lik, activation, _, _, beta = hyper(g)
    eng = golden_engine(case, g, noise_rng="device")
    x = g["x"][0]
    loss = eng.forward(torch.from_numpy(x))
    eps = eng.model.last_noise
    assert eps.is_cuda and tuple(eps.shape) == (meta(g)[3], meta(g)[2])
    loss64 = exact_grads(vc_params(case, g, 0), x, eps.cpu().numpy(), beta, activation, lik)[0]
    assert loss.dim() == 0 and loss.is_cuda
    assert_scalar_close(float(loss), loss64, what="forward")


def test_checkpoint_round_trip(hip_device, tmp_path):
    """Save, load into a fresh engine (weights and optimizer state): the reference's keys, the same next step."""
    case = "vaecf_bern_relu_wd"
    g = load_golden(case)
    eng = golden_engine(case, g)
    eng.model.next_noise = g["eps0"]
    eng.train_single_batch(torch.from_numpy(g["x"][0]))
    path = str(tmp_path / "vaecf.pt")
    eng.save_checkpoint(path, optimizer_state=True)
    assert tuple(torch.load(path)) == keys_of(g)
    other = golden_engine(case, g)
    with contextlib.redirect_stdout(io.StringIO()):
        other.resume_checkpoint(path, optimizer_state=True)
    assert torch.equal(other.model.flat, eng.model.flat)
    for e in (eng, other):
        e.model.next_noise = g["eps1"]
    a = eng.train_single_batch(torch.from_numpy(g["x"][1]))
    b = other.train_single_batch(torch.from_numpy(g["x"][1]))
    assert_scalar_close(b, a, 1e-6, "loss after the reload")
    assert_tensor_close(other.model.flat.cpu().numpy(), eng.model.flat.cpu().numpy(), 1e-6, "weights after the step")


def test_shape_struct_and_workspace(hip_device):
    """The struct's size on both sides of the ABI; the flat layout; beyond the limits the workspace call returns 0 and
    says why; and a condition, not a measurement: at n_items = 2^20, B = 1024, nnz = 64 B the workspace is below the
    4 B n_items bytes of ONE [B, n_items] fp32 buffer, with either form of the first layer's gather."""
    from beta_recsys_amd import _lib

    lib = _lib.load()
    assert lib.hiprec_vaecf_shape_bytes() == ctypes.sizeof(_lib.VaecfShape) == 48

    def shape(I=11, Z=10, hidden=(20,), shadow=0, act=1, lik=0):
        h = list(hidden) + [0] * (3 - len(hidden))
        return _lib.VaecfShape(9, I, Z, len(hidden), (ctypes.c_int32 * 3)(*h), act, lik, shadow)

    n_params = sum(int(np.prod(s)) for s in vn.shapes(11, [20], 10).values())
    assert lib.hiprec_vaecf_param_floats(ctypes.byref(shape())) == n_params
    B, I = 1024, 1 << 20
    for shadow in (0, 1):
        need = lib.hiprec_vaecf_workspace_bytes(ctypes.byref(shape(I=I, shadow=shadow)), B, 64 * B)
        print(f"workspace at n_items 2^20, B 1024, shadow {shadow}: {need / 2**20:.1f} MiB vs {4 * B * I / 2**20:.0f} MiB")
        assert 0 < need < 4 * B * I
    for bad in (shape(Z=257), shape(hidden=(513,)), shape(Z=0), shape(act=4), shape(lik=4), shape(I=0)):
        assert lib.hiprec_vaecf_workspace_bytes(ctypes.byref(bad), 8, 8) == 0
        assert lib.hiprec_last_error()
        assert lib.hiprec_vaecf_param_floats(ctypes.byref(bad)) == -1
    assert lib.hiprec_vaecf_workspace_bytes(ctypes.byref(shape()), 1 << 22, 8) == 0
    assert b"2^31" in lib.hiprec_last_error()
