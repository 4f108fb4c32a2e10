"""GPU parity tests of VBCAR (csrc/vbcar.hip): forward + loss + backward, the full step and chained steps vs golden
vectors from the real reference's VBCAREngine (tests/golden/vbcar_*.npz) with the captured noise injected; synthetic
shapes that straddle every kernel constant (tests/vbcar_edges.py) against the fp64 restatement; the epoch loop with its
sampler order, noise draw and logging; predict / ranking_factors / recommend; the bounds check; the ValueError cases; the
checkpoint round trip.

Gradients that come from atomics (the two tables, the split-K weight gradients) are not bit-reproducible and no test asks
for that; the bias gradients of ``fc_*_2_mu`` are fixed-order column sums of ``d_out``, which is written with plain
stores, so they are compared bitwise between two runs."""
import contextlib
import io
import re

import numpy as np
import pytest
import torch

import topk_reference as tk
import vbcar_edges as ve
import vbcar_numpy as vn
from helpers import assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_sgd_exact
from helpers import assert_step_close, assert_tensor_close, float64_oracle, load_golden, oracle_trajectory, to64
from test_oracle_golden_vbcar import CASES, edge_config, exact_grads, golden_config, hyper, meta, vb_band, vb_batch
from test_oracle_golden_vbcar import vb_eps, vb_fea, vb_opt_state, vb_params

pytestmark = pytest.mark.gpu


def engine_for(cfg, w=None):
    import beta_recsys_amd as hp

    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.VBCAREngine(cfg)
    if w is not None:
        load_weights(eng, w)
    return eng


def golden_engine(case, g):
    return engine_for(golden_config(g, device="cuda:0"), vb_params(case, g, 0))


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def load_opt_state(eng, st):
    eng.load_optimizer_state(st["step"], st.get("exp_avg"), st.get("exp_avg_sq", st.get("square_avg")))


def np_grads(grads):
    return {k: v.cpu().numpy() for k, v in grads.items()}


def report(grads, g_ref, g64):
    for k in g64:
        print(f"  grad {k}: err vs exact {np.abs(grads[k].reshape(g64[k].shape) - g64[k]).max():.3e}, reference's own "
              f"{np.abs(g_ref[k] - g64[k]).max():.3e}, scale {np.abs(g64[k]).max():.3e}")


def dot_floor(eu, ei):
    """Scale floor of predict's scores: a score is a dot product of 2D terms of either sign, so its fp32 rounding error is
    relative to the sum of the terms' magnitudes, not to the (cancelled) result (helpers.grad_scale_floor's reasoning)."""
    return float(np.abs(eu * ei).sum(1).max())


def absent_rows_are_zero(grads, batch, what):
    users = set(np.concatenate([batch[0], batch[3].ravel()]).tolist())
    items = set(np.concatenate([batch[1], batch[2], batch[4].ravel(), batch[5].ravel()]).tolist())
    for key, present in (("user_emb.weight", users), ("item_emb.weight", items)):
        absent = [r for r in range(grads[key].shape[0]) if r not in present]
        assert float(np.abs(grads[key][absent]).max(initial=0.0)) == 0.0, f"{what}: a gradient reached an absent {key} row"
    return grads["user_emb.weight"].shape[0] - len(users), grads["item_emb.weight"].shape[0] - len(items)


@pytest.mark.parametrize("case", CASES)
def test_step_matches_reference(hip_device, case):
    """Each step from the reference's own weights and optimizer state, its captured noise injected: the loss and its two
    parts, every gradient (as accurate as the reference against the fp64 evaluation), rows of ids absent from the batch
    exactly zero, the gradient buffer cleared after the sweep, the stepped weights inside the band."""
    g = load_golden(case)
    opt, lr, activator, alpha, scale = hyper(g)
    fea = vb_fea(g)
    eng = golden_engine(case, g)
    for s in range(meta(g)[9]):
        batch, eps = vb_batch(g, s), vb_eps(g, s)
        w0, st0 = vb_params(case, g, s), vb_opt_state(case, g, s)
        load_weights(eng, w0)
        load_opt_state(eng, st0)
        eng.model.next_noise = eps
        loss, grads = eng.backward_only(batch)
        grads = np_grads(grads)
        print(f"{case} step {s}: loss {loss!r} vs {float(g['losses'][s])!r}, kl {eng.model.kl_loss!r} vs "
              f"{float(g['kl_losses'][s])!r}, rec {eng.model.rec_loss!r} vs {float(g['rec_losses'][s])!r}")
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        assert_scalar_close(eng.model.kl_loss, g["kl_losses"][s], what=f"kl_loss step {s}")
        assert_scalar_close(eng.model.rec_loss, g["rec_losses"][s], what=f"rec_loss step {s}")
        g_ref = vb_params(case, g, s + 1, "g")
        g64 = exact_grads(w0, fea, batch, eps, alpha, scale, activator)[3]
        report(grads, g_ref, g64)
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}")
        assert min(absent_rows_are_zero(grads, batch, f"step {s}")) >= 1, "the fixture leaves a user and an item out"
        assert float(eng._g_flat.abs().max()) == 0.0
        assert eng.model.next_noise is None, "injected noise serves one step"
        # the full step
        load_opt_state(eng, st0)
        eng.model.next_noise = np.concatenate(eps)            # the stacked form
        loss = eng.train_single_batch(batch)
        assert isinstance(loss, float)
        assert_scalar_close(loss, g["losses"][s], what=f"loss (step) {s}")
        band = vb_band(w0, st0, g_ref, opt, lr)
        w1, w_ref = get_weights(eng), vb_params(case, g, s + 1)
        for k in w_ref:
            assert_step_close(w0[k], w1[k], w_ref[k], band[k], what=f"weights {k} step {s}")
        assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"


@pytest.mark.parametrize("case", CASES)
def test_trajectory_matches_reference(hip_device, case):
    """Three steps chained from w0.  SGD: every element within 1e-5 of the trajectory's update; Adam / RMSprop: every
    element inside the oracle's perturbed-gradient envelope around the reference's end point."""
    g = load_golden(case)
    opt, lr, activator, alpha, scale = hyper(g)
    fea, steps = vb_fea(g), meta(g)[9]
    eng = golden_engine(case, g)
    w0 = vb_params(case, g, 0)
    batches = [(vb_batch(g, s), vb_eps(g, s)) for s in range(steps)]
    for s, (batch, eps) in enumerate(batches):
        eng.model.next_noise = eps
        loss = eng.train_single_batch(batch)
        print(f"{case} chained step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        if opt == "sgd" or s == 0:
            assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
    ref_end = vb_params(case, g, steps)
    if opt == "sgd":
        assert_sgd_exact(get_weights(eng), ref_end, w0, "final weights")
        return
    _, env, upd = oracle_trajectory(
        w0, batches, lambda w, b: vn.vbcar_grads(w, fea, b[0], b[1], alpha, scale, activator)[3],
        lambda w, gr, st: vn.opt_step(w, gr, st, opt, lr), lambda w: vn.new_opt_state(w, opt))
    assert_on_trajectory(get_weights(eng), ref_end, env, upd, f"{case} trajectory")


@pytest.mark.parametrize("shape", ve.SHAPES, ids=ve.shape_id)
def test_shapes_against_the_restatement(hip_device, shape):
    """Loss, its parts, gradients, the eval-mode encoder and predict at the shapes of vbcar_edges.py against the
    restatement in fp64, as accurate as its fp32 self; the plain-store side of the backward bitwise equal in two runs."""
    U, I, D = shape[:3]
    w, fea, batch, eps = ve.synthetic(shape)
    activator, alpha, scale = ve.hyper(shape)
    eng = engine_for(edge_config(shape, device="cuda:0", fea=fea), w)
    g32 = vn.vbcar_grads(w, fea, batch, eps, alpha, scale, activator)[3]
    loss64, gen64, kld64, g64, _ = exact_grads(w, fea, batch, eps, alpha, scale, activator)
    eng.model.next_noise = eps
    loss, grads = eng.backward_only(batch)
    grads = np_grads(grads)
    print(f"{ve.shape_id(shape)}: loss {loss!r} vs exact {loss64!r}")
    report(grads, g32, g64)
    assert_scalar_close(loss, loss64, what="loss")
    assert_scalar_close(eng.model.rec_loss, gen64, what="rec_loss")
    assert_scalar_close(eng.model.kl_loss, kld64, what="kl_loss")
    assert_grads_as_accurate(grads, g32, g64, what="grad")
    absent_rows_are_zero(grads, batch, ve.shape_id(shape))
    eng.model.next_noise = eps
    again = np_grads(eng.backward_only(batch)[1])
    for k in ("fc_u_2_mu.bias", "fc_i_2_mu.bias"):
        assert np.array_equal(again[k], grads[k]), f"{k}: fixed-order column sums of plain-store d_out moved between runs"
    # eval mode
    users, items = np.arange(U)[::-1].copy(), np.arange(I)
    with float64_oracle(vn):
        eu64, ei64 = vn.encode(to64(w), fea[0], users, "u", activator), vn.encode(to64(w), fea[1], items, "i", activator)
        pu, pi = np.resize(users, 7), np.resize(items, 7)
        p64 = vn.predict(to64(w), fea, pu, pi, activator)
    eu = eng.model.encode(users, "user").cpu().numpy()
    ei = eng.model.encode(items, "item").cpu().numpy()
    assert eu.shape == (U, 2 * D) and ei.shape == (I, 2 * D)
    assert np.array_equal(eu[:, D:], w["user_emb.weight"][users]) and np.array_equal(ei[:, D:], w["item_emb.weight"])
    assert_tensor_close(eu, eu64, what="encode users")
    assert_tensor_close(ei, ei64, what="encode items")
    pred = eng.model.predict(pu, pi)
    assert pred.shape == (7,) and pred.dtype == torch.float32
    assert_tensor_close(pred.cpu().numpy(), p64, what="predict", scale_floor=dot_floor(eu64[::-1][pu], ei64[pi]))


class _Sampler:
    """Stands in for ``engine.data.*_sampler``: hands out the fixture's negatives and records the calls."""

    def __init__(self, rows, log, name):
        self.rows, self.log, self.name = list(rows), log, name

    def sample(self, count, obj_num):
        self.log.append((self.name, count, obj_num))
        return self.rows.pop(0)


def test_epoch_follows_the_reference_loop(hip_device):
    """``train_an_epoch`` on the short-batch fixture's three batches: the negatives come from ``engine.data``'s samplers
    in the reference's order (users, items, items), the noise from ``draw_noise`` under the torch seed (step 0's captured
    RNG state reproduces the fixture's eps, hence its loss), the totals are divided by the config batch size, the line is
    printed and ``add_scalars`` called."""
    import types

    case = "vbcar_sgd_sigmoid_short"
    g = load_golden(case)
    opt, lr, activator, alpha, scale = hyper(g)
    fea, steps, bs = vb_fea(g), meta(g)[9], meta(g)[8]
    eng = golden_engine(case, g)
    log = []
    eng.data = types.SimpleNamespace(
        user_sampler=_Sampler([g["neg_u"][s] for s in range(steps)], log, "user"),
        item_sampler=_Sampler([x for s in range(steps) for x in (g["neg_i_1"][s], g["neg_i_2"][s])], log, "item"))
    loader = [torch.from_numpy(np.stack([g["pos_u"][s], g["pos_i_1"][s], g["pos_i_2"][s]], 1)) for s in range(steps)]
    # the restatement of the same epoch under the same noise stream
    torch.set_rng_state(torch.from_numpy(g["rng_state0"]))
    from beta_recsys_amd.vbcar import draw_noise

    B, n_neg, D = meta(g)[7], meta(g)[6], meta(g)[2]
    w = to64(vb_params(case, g, 0))
    tot = gen_sum = kld_sum = 0.0
    with float64_oracle(vn):
        st = vn.new_opt_state(w, opt)
        for s in range(steps):
            noise = draw_noise(B, n_neg, D, "cpu").numpy()
            eps = np.split(noise, np.cumsum([B, B, B, B * n_neg, B * n_neg])[:5])
            loss, gen, kld = vn.train_step(w, st, fea, vb_batch(g, s), eps, alpha, scale, activator, opt, lr)
            tot, gen_sum, kld_sum = tot + loss, gen_sum + gen, kld_sum + kld
            if s == 0:
                assert_scalar_close(loss, g["losses"][0], what="step 0 under the fixture's RNG state")
    torch.set_rng_state(torch.from_numpy(g["rng_state0"]))
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        eng.train_an_epoch(loader, 4)
    assert log == [(n, n_neg, B) for _ in range(steps) for n in ("user", "item", "item")]
    line = [ln for ln in out.getvalue().splitlines() if ln.startswith("[Training Epoch 4], log_like_loss ")]
    assert len(line) == 1 and line[0].endswith(f" alpha: {alpha} lr: {lr}")
    got = {tag: (v, step) for tag, v, step in eng.writer.scalars[-3:]}
    assert set(got) == {"model/loss/total_loss", "model/loss/rec_loss", "model/loss/kl_loss"}
    assert all(step == 4 for _, step in got.values())
    assert_scalar_close(got["model/loss/total_loss"][0], tot / bs, what="total_loss")
    assert_scalar_close(got["model/loss/kl_loss"][0], kld_sum / bs, what="kl_loss")
    assert_scalar_close(got["model/loss/rec_loss"][0], (tot - kld_sum) / bs, what="rec_loss (total - kl, as the reference)")
    printed = re.match(r"\[Training Epoch 4\], log_like_loss (\S+) kl_loss: (\S+) alpha:", line[0])
    assert_scalar_close(float(printed.group(1)), gen_sum / bs, what="printed log_like_loss")
    assert_scalar_close(float(printed.group(2)), kld_sum / bs, what="printed kl_loss")
    assert_sgd_exact(get_weights(eng), {k: v.astype(np.float32) for k, v in w.items()}, vb_params(case, g, 0), "epoch end")


def test_predict_ranking_factors_and_recommend(hip_device):
    """Against the fp64 restatement's scores; the top-K through tests/topk_reference.py, which compares ids only where
    the reference scores are separated by more than the bound."""
    case = "vbcar_adam_relu"
    g = load_golden(case)
    U, I, D = meta(g)[:3]
    activator = hyper(g)[2]
    w, fea = vb_params(case, g, 0), vb_fea(g)
    eng = golden_engine(case, g)
    users, items = np.repeat(np.arange(U), I), np.tile(np.arange(I), U)
    with float64_oracle(vn):
        eu64 = vn.encode(to64(w), fea[0], np.arange(U), "u", activator)
        ei64 = vn.encode(to64(w), fea[1], np.arange(I), "i", activator)
        p64 = vn.predict(to64(w), fea, users, items, activator)
    s64 = eu64 @ ei64.T
    assert np.allclose(s64.ravel(), p64, rtol=1e-12, atol=1e-12)
    pred = eng.model.predict(users.tolist(), torch.from_numpy(items))
    assert pred.dtype == torch.float32 and pred.shape == (U * I,)
    assert_tensor_close(pred.cpu().numpy(), p64, what="predict", scale_floor=dot_floor(eu64[users], ei64[items]))
    Uf, If, a, bias = eng.model.ranking_factors()
    assert a == 1.0 and bias is None and tuple(Uf.shape) == (U, 2 * D) and tuple(If.shape) == (I, 2 * D)
    assert_tensor_close(Uf.cpu().numpy(), eu64, what="user factors")
    assert_tensor_close(If.cpu().numpy(), ei64, what="item factors")
    k = 5
    q = np.array([3, 0, 8, 3])
    got_i, got_s = eng.recommend(q, k)
    tk.check_against_float64(got_i.cpu().numpy(), got_s.cpu().numpy(), s64[q], None, "recommend")
    seen_u, seen_i = np.array([3, 3, 0, 8]), np.array([int(np.argmax(s64[3])), 1, int(np.argmax(s64[0])), 2])
    got_i, got_s = eng.recommend(q, k, seen=(seen_u, seen_i))
    seen = [np.unique(seen_i[seen_u == u]) for u in q]
    tk.check_against_float64(got_i.cpu().numpy(), got_s.cpu().numpy(), s64[q], seen, "recommend with seen")
    with pytest.raises(ValueError):
        eng.model.predict([0, 1], [0])


def test_out_of_range_ids_raise_and_leave_the_engine_usable(hip_device):
    case = "vbcar_rmsprop_tanh"
    g = load_golden(case)
    U, I = meta(g)[:2]
    eng = golden_engine(case, g)
    good = vb_batch(g, 0)
    before = eng.model.flat.clone()
    for slot, n in enumerate((U, I, I, U, I, I)):              # each of the six arrays, too large and negative
        for value in (n, -1):
            bad = [a.copy() for a in good]
            bad[slot].reshape(-1)[-1] = value
            eng.model.next_noise = vb_eps(g, 0)
            with pytest.raises(IndexError):
                eng.backward_only(tuple(bad))
            assert torch.equal(eng.model.flat, before), "the weights moved"
            assert float(eng._g_flat.abs().max()) == 0.0, "a partial gradient was kept"
    bad = [a.copy() for a in good]
    bad[4][0, 0] = I + 7
    with pytest.raises(IndexError):
        eng.train_single_batch(tuple(bad))
    assert float(eng._g_flat.abs().max()) == 0.0
    with pytest.raises(IndexError):
        eng.model.predict([0, U], [0, 0])
    with pytest.raises(IndexError):
        eng.model.encode([I], "item")
    load_weights(eng, vb_params(case, g, 0))
    eng.load_optimizer_state(0)
    eng.model.next_noise = vb_eps(g, 0)
    loss = eng.train_single_batch(good)
    assert_scalar_close(loss, g["losses"][0], what="loss after the errors")


def test_what_the_reference_cannot_run_is_a_value_error(hip_device):
    case = "vbcar_rmsprop_tanh"
    g = load_golden(case)
    eng = golden_engine(case, g)
    good = vb_batch(g, 0)
    one = tuple(a[:1] for a in good)                            # .squeeze() drops the batch dimension
    fewer_negs = good[:3] + tuple(a[:, :2] for a in good[3:])
    ragged = good[:2] + (good[2][:-1],) + good[3:]
    for bad in (one, fewer_negs, ragged, good[:5]):
        with pytest.raises(ValueError):
            eng.train_single_batch(bad)
    eng.model.next_noise = vb_eps(g, 0)[:5]
    with pytest.raises(ValueError):
        eng.train_single_batch(good)
    cfg = golden_config(g, device="cuda:0")
    cfg["model"]["activator"] = "prelu"
    with pytest.raises(ValueError):
        engine_for(cfg)
    eng.model.next_noise = vb_eps(g, 0)
    assert_scalar_close(eng.train_single_batch(good), g["losses"][0], what="loss after the errors")


def test_checkpoint_round_trip(hip_device, tmp_path):
    """Save, load into a fresh engine (weights and optimizer state): the reference's keys, the same next step."""
    case = "vbcar_adam_relu"
    g = load_golden(case)
    eng = golden_engine(case, g)
    eng.model.next_noise = vb_eps(g, 0)
    eng.train_single_batch(vb_batch(g, 0))
    path = str(tmp_path / "vbcar.pt")
    eng.save_checkpoint(path, optimizer_state=True)
    sd = torch.load(path)
    assert tuple(sd) == vn.KEYS
    other = golden_engine(case, g)
    with contextlib.redirect_stdout(io.StringIO()):
        other.resume_checkpoint(path, optimizer_state=True)
    assert torch.equal(other.model.flat, eng.model.flat)
    for e in (eng, other):
        e.model.next_noise = vb_eps(g, 1)
    a = eng.train_single_batch(vb_batch(g, 1))
    b = other.train_single_batch(vb_batch(g, 1))
    assert_scalar_close(b, a, 1e-6, "loss after the reload")
    assert_tensor_close(other.model.flat.cpu().numpy(), eng.model.flat.cpu().numpy(), 1e-6, "weights after the step")
