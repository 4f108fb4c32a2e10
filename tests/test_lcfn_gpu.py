"""GPU parity tests of LCFN (csrc/lcfn.hip): every golden fixture step by step and chained, predict / ranking_factors /
recommend on the new weights, run-to-run bits of the propagation, out-of-range ids -- against the reference's vectors
(tests/golden/lcfn_*.npz) and the numpy restatement."""
import ctypes

import numpy as np
import pytest
import torch

import lcfn_numpy as lx
from helpers import REL, assert_as_accurate_as_reference, assert_on_trajectory, assert_scalar_close, assert_sgd_exact
from helpers import assert_step_close, assert_tensor_close, float64_oracle, to64
from test_lcfn_host import load_weights, make_engine
from test_oracle_golden_lcfn import CASES, KEYS, lcfn_band, lcfn_bases, lcfn_batch, lcfn_golden, lcfn_hp, lcfn_meta
from test_oracle_golden_lcfn import lcfn_opt_state, lcfn_params, lcfn_trajectory, lcfn_weights

pytestmark = pytest.mark.gpu


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def load_opt_state(eng, st):
    eng.load_optimizer_state(st["step"], st.get("exp_avg"), st.get("exp_avg_sq", st.get("square_avg")))


@pytest.fixture(scope="module")
def trajectories():
    """The restatement's legal-trajectory envelope of every case, computed once."""
    return {case: lcfn_trajectory(lcfn_golden(case), 0 if str(lcfn_golden(case)["optimizer"]) == "sgd" else 8)
            for case in CASES}


@pytest.mark.parametrize("case", CASES)
def test_steps_match_reference(hip_device, case, trajectories):
    """Each step from the reference's own weights and optimizer state: the loss and both parts at REL, the gradients
    within REL of scale of the reference's fp64 gradients plus twice the reference's own fp32 distance from them, the
    updated weights inside the optimizer band, the gradient left cleared.  Then the three steps chained from w0: plain SGD
    every element within REL of the largest update, Adam / RMSprop every element inside the legal-trajectory envelope
    (zero outliers).  Filters and transformers do not move (the reference's behaviour)."""
    g = lcfn_golden(case)
    m = lcfn_meta(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    eng = make_engine(g, device_str="cuda:0")
    eng.model.train()
    load_weights(eng, lcfn_weights(g, "w0"))
    tail0 = eng.model.filter_state()
    for s in range(m["n_steps"]):
        batch = lcfn_batch(g, s)
        w0, st0 = lcfn_params(g, f"w{s}"), lcfn_opt_state(g, s, opt)
        load_weights(eng, w0)
        load_opt_state(eng, st0)
        loss, grads = eng.backward_only(batch)
        parts = eng.last_losses()
        print(f"{case} step {s}: loss {loss!r} vs {float(g['losses'][s])!r}; parts {parts} vs {g['parts'][s]}")
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        for got, ref, name in zip(parts, g["parts"][s], ("bpr", "reg")):
            assert_scalar_close(got, ref, what=f"{name} step {s}")
        g_ref = lcfn_params(g, f"g{s + 1}")
        for k in KEYS:
            got, exact = grads[k].cpu().numpy(), g[f"g64_{s + 1}/{k}"]
            print(f"  grad {k}: err vs fp64 {np.abs(got - exact).max():.3e} (the reference's {np.abs(g_ref[k] - exact).max():.3e}) "
                  f"of scale {np.abs(exact).max():.3e}")
            assert_as_accurate_as_reference(got, g_ref[k], exact, what=f"grad {k} step {s}")
        for k in lx.tail_keys(m["L"]):
            assert float(grads[k].abs().max()) == 0.0, f"{k}: the filters are not trained, their gradient stays zero"
        assert float(eng._g_flat.abs().max()) == 0.0
        load_opt_state(eng, st0)
        loss = eng.train_single_batch(batch)
        assert_scalar_close(loss, g["losses"][s], what=f"loss (step) {s}")
        band = lcfn_band(w0, st0, g_ref, opt, lr)
        w1 = get_weights(eng)
        for k in KEYS:
            assert_step_close(w0[k], w1[k], g[f"w{s + 1}/{k}"], band[k], what=f"weights {k} step {s}")
        assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"
    # chained
    w0 = lcfn_params(g, "w0")
    load_weights(eng, w0)
    load_opt_state(eng, lcfn_opt_state(g, 0, opt))
    for s in range(m["n_steps"]):
        loss = eng.train_single_batch(lcfn_batch(g, s))
        print(f"  chained step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
    w_ref, env, upd = trajectories[case]
    ref_end = lcfn_params(g, f"w{m['n_steps']}")
    if opt == "sgd":
        assert_sgd_exact(get_weights(eng), ref_end, w0, f"{case} chained weights")
    else:
        assert_on_trajectory(get_weights(eng), ref_end, env, upd, f"{case} chained weights")
    for k, v in eng.model.filter_state().items():
        assert torch.equal(v, tail0[k]), f"{k} moved"


@pytest.mark.parametrize("case", ["lcfn_adam", "lcfn_sgd_hot"])
def test_predict_factors_and_recommend_use_the_new_weights(hip_device, case):
    """After a step, predict / ranking_factors / recommend are the restatement on the weights the step LEFT (the
    reference would still read the tables from before it); cached until the weights change again."""
    import beta_recsys_amd as hp_pkg

    g = lcfn_golden(case)
    m, hp, bases = lcfn_meta(g), lcfn_hp(g), lcfn_bases(g)
    eng = make_engine(g, device_str="cuda:0")
    load_weights(eng, lcfn_weights(g, "w0"))
    users, items = np.repeat(np.arange(m["U"]), m["I"]), np.tile(np.arange(m["I"]), m["U"])
    before = eng.model.predict(users, items).cpu().numpy()
    for s in range(m["n_steps"]):
        eng.train_single_batch(lcfn_batch(g, s))
    w1 = {**lcfn_weights(g, "w0"), **get_weights(eng)}
    with float64_oracle(lx):
        ref = lx.lcfn_predict(to64(w1), bases, hp, users, items)
        fu, fi = lx.lcfn_all_embeddings(to64(w1), bases, hp)
        old = lx.lcfn_predict(to64(lcfn_weights(g, "w0")), bases, hp, users, items)
    assert_tensor_close(before, old, what="predict before the steps")
    scores = eng.model.predict(users, items)
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (users.size,)
    assert_tensor_close(scores.cpu().numpy(), ref, what="predict after the steps")
    assert np.abs(ref - old).max() > 10 * REL * np.abs(ref).max(), "the steps moved no score: the test shows nothing"
    U_f, I_f, alpha, bias = eng.model.ranking_factors()
    assert bias is None and alpha == 1.0 and tuple(U_f.shape) == (m["U"], (m["L"] + 1) * m["D"])
    assert_tensor_close(U_f.cpu().numpy(), fu, what="user factors")
    assert_tensor_close(I_f.cpu().numpy(), fi, what="item factors")
    key = eng.model._pool_key
    assert torch.equal(eng.model.predict(users, items), scores) and eng.model._pool_key == key
    top, _ = hp_pkg.recommend(eng.model, np.arange(m["U"]), 5)
    dense = ref.reshape(m["U"], m["I"])
    got = top.cpu().numpy()
    for u in range(m["U"]):
        kth = np.sort(dense[u])[-5]
        assert len(set(got[u])) == 5 and np.all(dense[u][got[u]] >= kth - 1e-5 * np.abs(dense[u]).max()), f"user {u}"
    with pytest.raises(IndexError):
        eng.model.predict([0, m["U"]], [0, 0])
    with pytest.raises(IndexError):
        eng.model.predict([0, 0], [0, -1])
    assert np.isfinite(eng.model.predict([0], [0]).cpu().numpy()).all()     # usable after the error


def test_out_of_range_ids_raise(hip_device):
    """A user, positive or negative id outside its table raises IndexError (nothing is read or written out of range: the
    loss stage and the regulariser scatter skip such triples) and the engine stays usable."""
    g = lcfn_golden("lcfn_adam")
    m = lcfn_meta(g)
    eng = make_engine(g, device_str="cuda:0")
    users, pos, neg = (a.copy() for a in lcfn_batch(g, 0))
    for what, (arr, idx, val) in {"user": (0, 3, m["U"]), "negative user": (0, 0, -1), "pos": (1, 5, m["I"]),
                                  "neg": (2, 7, m["I"]), "negative neg": (2, 0, -1)}.items():
        b = [users.copy(), pos.copy(), neg.copy()]
        b[arr][idx] = val
        with pytest.raises(IndexError):
            eng.train_single_batch(tuple(b))
        assert float(eng._g_flat.abs().max()) == 0.0, what
        assert torch.isfinite(eng.model.flat).all(), what
    load_weights(eng, lcfn_weights(g, "w0"))
    eng.load_optimizer_state(0)
    assert_scalar_close(eng.train_single_batch((users, pos, neg)), g["losses"][0], what="usable after the errors")


@pytest.mark.parametrize("case", ["lcfn_adam", "lcfn_rmsprop_d64"])
def test_two_propagations_give_identical_bits(hip_device, case):
    """hiprec_lcfn_propagate sums its partial slots in slot order and uses no atomics: two runs, and a run into a
    workspace full of garbage, give the same bits."""
    from beta_recsys_amd import _lib

    g = lcfn_golden(case)
    m = lcfn_meta(g)
    eng = make_engine(g, device_str="cuda:0", project_slots=3)       # several tiles per slot at the wide case
    load_weights(eng, lcfn_weights(g, "w0"))
    model = eng.model
    lib = _lib.load()
    n_all = (m["U"] + m["I"]) * (m["L"] + 1) * m["D"]
    runs = []
    for fill in (0.0, 7.0, float("nan")):
        plan = model.plan()
        model._ws["ws"].fill_(fill)
        _lib.check(lib.hiprec_lcfn_propagate(ctypes.byref(plan), _lib.stream_ptr(model.flat.device)))
        runs.append(model._ws["ws"][:n_all].cpu().numpy().copy())
    assert np.isfinite(runs[0]).all() and np.abs(runs[0]).max() > 0
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


def test_epoch_trains_every_batch(hip_device, capsys):
    g = lcfn_golden("lcfn_adam")
    m = lcfn_meta(g)
    eng = make_engine(g, device_str="cuda:0")
    load_weights(eng, lcfn_weights(g, "w0"))
    batches = [tuple(torch.from_numpy(a) for a in lcfn_batch(g, s)) for s in range(m["n_steps"])]
    eng.train_an_epoch(batches, 0)
    assert "[Training Epoch 0], Loss" in capsys.readouterr().out
    w_ref, env, upd = lcfn_trajectory(g, 8)
    assert_on_trajectory(get_weights(eng), lcfn_params(g, f"w{m['n_steps']}"), env, upd, "epoch weights")
