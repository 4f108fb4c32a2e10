"""GPU parity tests of BUIR (csrc/buir.hip): every golden fixture step by step and chained, the frozen target, predict /
ranking_factors / recommend, checkpoints, the invalidation of the pooled target and out-of-range ids, against the
reference's vectors (tests/golden/buir_*.npz) and the numpy restatement."""
import contextlib
import io

import numpy as np
import pytest
import torch

import buir_numpy as bx
from helpers import assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_sgd_exact, assert_step_close
from helpers import assert_tensor_close, float64_oracle, load_golden, to64
from test_oracle_golden_buir import CASES, KEYS, ONLINE, TARGET, TRAINABLE, bu_band, bu_batch, bu_graph, bu_meta
from test_oracle_golden_buir import bu_opt_state, bu_params, bu_trajectory, make_engine

pytestmark = pytest.mark.gpu


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def load_opt_state(eng, st):
    eng.load_optimizer_state(st["step"], st.get("exp_avg"), st.get("exp_avg_sq", st.get("square_avg")))


@pytest.mark.parametrize("case", CASES)
def test_steps_match_reference(hip_device, case):
    """Each step from the reference's own weights and optimizer state: the loss at REL, the gradients within REL of scale
    of the reference's fp64 gradients plus twice the reference's own fp32 distance from them, the updated weights inside
    the optimizer band, the target moved by the reference's own ``_update_target`` or not at all.  Then the three steps
    chained from w0: plain SGD every element within REL of the largest update, Adam / RMSprop every element inside the
    legal-trajectory envelope (zero outliers)."""
    g = load_golden(case)
    m = bu_meta(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    eng = make_engine(g, device_str="cuda:0")
    eng.model.train()
    for s in range(m["n_steps"]):
        batch = bu_batch(g, s)
        w0, st0 = bu_params(g, f"w{s}"), bu_opt_state(g, s, opt)
        load_weights(eng, w0)
        load_opt_state(eng, st0)
        loss, grads = eng.backward_only(batch)
        print(f"{case} step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        assert set(grads) == set(TRAINABLE), "gradients for the four trained tensors, none for the target"
        g_ref = bu_params(g, f"g{s + 1}", TRAINABLE)
        assert_grads_as_accurate(grads, g_ref, {k: g[f"g64_{s + 1}/{k}"] for k in TRAINABLE}, what=f"{case} step {s}")
        assert float(eng._g_flat.abs().max()) == 0.0
        load_opt_state(eng, st0)
        loss = eng.train_single_batch(batch)
        assert_scalar_close(loss, g["losses"][s], what=f"loss (step) {s}")
        band = bu_band(w0, st0, g_ref, opt, lr)
        w1 = get_weights(eng)
        for k in TRAINABLE:
            assert_step_close(w0[k], w1[k], g[f"w{s + 1}/{k}"], band[k], what=f"weights {k} step {s}")
        for o, t in zip(ONLINE, TARGET):
            if m["ema"]:
                assert_step_close(w0[t], w1[t], g[f"w{s + 1}/{t}"], (1 - m["momentum"]) * band[o], what=f"target {t} step {s}")
            else:
                assert np.array_equal(w1[t], w0[t]), f"{t} moved with update_target off"
        assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"
    # chained
    w0 = bu_params(g, "w0")
    load_weights(eng, w0)
    load_opt_state(eng, bu_opt_state(g, 0, opt))
    for s in range(m["n_steps"]):
        loss = eng.train_single_batch(bu_batch(g, s))
        print(f"  chained step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
    w_ref, env, upd = bu_trajectory(g)
    ref_end = bu_params(g, f"w{m['n_steps']}")
    if opt == "sgd":
        assert_sgd_exact(get_weights(eng), ref_end, w0, f"{case} chained weights")
    else:
        assert_on_trajectory(get_weights(eng), ref_end, env, upd, f"{case} chained weights")


@pytest.mark.parametrize("case", ["buir_adam", "buir_sgd_hot", "buir_rmsprop_d64"])
def test_target_floats_are_bit_unchanged(hip_device, case):
    """update_target off: three steps leave every float of the target tables -- and of the optimizer moments behind
    them, which the sweep never reaches -- exactly as they were, while everything trained moves."""
    g = load_golden(case)
    eng = make_engine(g, device_str="cuda:0")
    load_weights(eng, bu_params(g, "w0"))
    eng._setup()
    n = eng._sweep_floats()
    before = eng.model.flat.detach().cpu().numpy().copy()
    for s in range(3):
        eng.train_single_batch(bu_batch(g, s))
    after = eng.model.flat.detach().cpu().numpy()
    assert np.array_equal(before[n:], after[n:]) and before[n:].size == sum(g[f"w0/{k}"].size for k in TARGET)
    assert not np.array_equal(before[:n], after[:n])
    for buf in (eng.optimizer.exp_avg, eng.optimizer.exp_avg_sq):
        if buf is not None:
            assert not buf[n:].any().item() and buf[:n].any().item()


def test_predict_factors_and_recommend(hip_device):
    """predict against the reference's scores and the restatement, before and after a step; the dot product of
    ranking_factors' 2 D-wide rows is predict; recommend()'s top-k is a brute-force ranking; a one-element call
    returns one score; ids out of range raise and leave the model usable."""
    import beta_recsys_amd as hp_pkg

    g = load_golden("buir_adam")
    m, graph = bu_meta(g), bu_graph(g)
    eng = make_engine(g, device_str="cuda:0")
    load_weights(eng, bu_params(g, f"w{m['n_steps']}"))
    got = eng.model.predict(g["predict_users"], g["predict_items"])
    assert got.dtype == torch.float32 and tuple(got.shape) == (g["predict_users"].size,)
    assert_tensor_close(got.cpu().numpy(), g["predict_scores"], what="predict vs the reference")
    eng.train_single_batch(bu_batch(g, 0))
    w1 = get_weights(eng)
    users, items = np.repeat(np.arange(m["U"]), m["I"]), np.tile(np.arange(m["I"]), m["U"])
    with float64_oracle(bx):
        ref = bx.buir_predict(to64(w1), graph, m["L"], users, items)
    assert_tensor_close(eng.model.predict(users, items).cpu().numpy(), ref, what="predict after a step")
    U_f, I_f, alpha, bias = eng.model.ranking_factors()
    assert bias is None and alpha == 1.0 and tuple(U_f.shape) == (m["U"], 2 * m["D"]) and tuple(I_f.shape) == (m["I"], 2 * m["D"])
    dense = ref.reshape(m["U"], m["I"])
    assert_tensor_close((U_f.double() @ I_f.double().T).cpu().numpy(), dense, what="ranking_factors' dot product")
    top, _ = hp_pkg.recommend(eng.model, np.arange(m["U"]), 5)
    top = top.cpu().numpy()
    for u in range(m["U"]):
        kth = np.sort(dense[u])[-5]
        assert len(set(top[u])) == 5 and np.all(dense[u][top[u]] >= kth - 1e-5 * np.abs(dense[u]).max()), f"user {u}"
    one = eng.model.predict([3], [7])
    assert tuple(one.shape) == (1,)
    assert abs(float(one[0]) - dense[3, 7]) <= 1e-5 * np.abs(dense).max(), "a one-element predict"
    with pytest.raises(IndexError):
        eng.model.predict([0, m["U"]], [0, 0])
    with pytest.raises(IndexError):
        eng.model.predict([0, 0], [0, -1])
    assert np.isfinite(eng.model.predict([0], [0]).cpu().numpy()).all()


def test_checkpoint_round_trip(hip_device, tmp_path):
    g = load_golden("buir_adam_ema")
    eng = make_engine(g, device_str="cuda:0")
    load_weights(eng, bu_params(g, "w0"))
    eng.train_single_batch(bu_batch(g, 0))
    path = str(tmp_path / "buir.pt")
    eng.save_checkpoint(path)
    saved = get_weights(eng)
    assert list(torch.load(path, map_location="cpu")) == list(KEYS)
    loss_a = eng.backward_only(bu_batch(g, 1))[0]
    other = make_engine(g, device_str="cuda:0")
    assert any(not np.array_equal(v, saved[k]) for k, v in get_weights(other).items())
    with contextlib.redirect_stdout(io.StringIO()):
        other.resume_checkpoint(path)
    for k, v in get_weights(other).items():
        assert np.array_equal(v, saved[k]), k
    # the resumed engine's pooled target was rebuilt from the restored raw tables
    assert_scalar_close(other.backward_only(bu_batch(g, 1))[0], loss_a, what="the step after a resume")
    with float64_oracle(bx):
        P = bx.pooled(bx.tables(to64(saved), TARGET), bx.dense_adj(bu_graph(g)), bu_meta(g)["L"])
    assert_tensor_close(other.pooled_target().cpu().numpy(), P, what="pooled target after a resume")


def test_loading_another_target_invalidates_the_pooled_one(hip_device):
    """load_state_dict with a different target, then one step: the same as a fresh engine given those weights.  An engine
    that kept its old pooled target would differ in the first digit."""
    g = load_golden("buir_adam")
    m = bu_meta(g)
    eng = make_engine(g, device_str="cuda:0")
    load_weights(eng, bu_params(g, "w0"))
    loss_old = eng.backward_only(bu_batch(g, 0))[0]       # the pooled target of w0 is built and in use
    w = bu_params(g, "w0")
    rng = np.random.default_rng(0)
    for t in TARGET:
        w[t] = rng.standard_normal(w[t].shape).astype(np.float32)
    load_weights(eng, w)
    fresh = make_engine(g, device_str="cuda:0")
    load_weights(fresh, w)
    (la, ga), (lb, gb) = eng.backward_only(bu_batch(g, 0)), fresh.backward_only(bu_batch(g, 0))
    assert abs(la - loss_old) > 1e-2, "another target moved nothing: the test shows nothing"
    with float64_oracle(bx):
        l64, g64 = bx.buir_grads(to64(w), bu_graph(g), m["L"], bu_batch(g, 0))
    assert_scalar_close(la, l64, what="loss on the loaded target")
    assert_scalar_close(lb, l64, what="loss of the fresh engine")
    for k in TRAINABLE:
        assert_tensor_close(ga[k].cpu().numpy(), g64[k], what=f"grad {k} on the loaded target")
    # invalidate_target() after writing the raw tables in place does the same
    with torch.no_grad():
        for t in TARGET:
            eng.model.state_dict()[t].copy_(torch.from_numpy(bu_params(g, "w0")[t]))
    eng.invalidate_target()
    assert_scalar_close(eng.backward_only(bu_batch(g, 0))[0], loss_old, what="after invalidate_target")


def test_out_of_range_ids_raise(hip_device):
    """A user or positive id outside its table raises IndexError (nothing is read or written out of range) and the
    engine stays usable; the negatives are never read, so theirs may be anything."""
    g = load_golden("buir_adam")
    m = bu_meta(g)
    eng = make_engine(g, device_str="cuda:0")
    users, pos, neg = (a.copy() for a in bu_batch(g, 0))
    for what, (arr, idx, val) in {"user": (0, 3, m["U"]), "negative user": (0, 0, -1), "pos": (1, 5, m["I"]),
                                  "negative pos": (1, 47, -1)}.items():
        b = [users.copy(), pos.copy(), neg.copy()]
        b[arr][idx] = val
        with pytest.raises(IndexError):
            eng.train_single_batch(tuple(b))
        assert float(eng._g_flat.abs().max()) == 0.0, what
        assert torch.isfinite(eng.model.flat).all(), what
    load_weights(eng, bu_params(g, "w0"))
    eng.load_optimizer_state(0)
    wild = neg.copy()
    wild[:] = 10 ** 9
    assert_scalar_close(eng.train_single_batch((users, pos, wild)), g["losses"][0], what="usable after the errors")


def test_epoch_trains(hip_device, capsys):
    g = load_golden("buir_adam")
    m = bu_meta(g)
    eng = make_engine(g, device_str="cuda:0")
    load_weights(eng, bu_params(g, "w0"))
    batches = [tuple(torch.from_numpy(a) for a in bu_batch(g, s)) for s in range(m["n_steps"])]
    eng.train_an_epoch(batches, 0)
    assert "[Training Epoch 0], Loss" in capsys.readouterr().out
    w = get_weights(eng)
    assert all(np.isfinite(w[k]).all() and np.abs(w[k] - g[f"w0/{k}"]).max() > 0 for k in TRAINABLE)
