"""GPU parity tests of SimGCL (csrc/simgcl.hip): every golden fixture step by step and chained with the reference's recorded
noise passed in, predict on the raw tables, the device draw against its numpy restatement bit for bit, a drawn step
against the same step fed the materialised noise, and the ``two_views`` switch, against the reference's vectors
(tests/golden/simgcl_*.npz) and the numpy restatement."""
import numpy as np
import pytest
import torch

import simgcl_numpy as sx
from helpers import REL, assert_as_accurate_as_reference, assert_on_trajectory, assert_scalar_close, assert_sgd_exact
from helpers import assert_step_close, assert_tensor_close, float64_oracle, load_golden, oracle_trajectory, to64
from test_oracle_golden_simgcl import CASES, KEYS, make_engine, sim_band, sim_batch, sim_graph, sim_hp, sim_meta
from test_oracle_golden_simgcl import sim_opt_state, sim_params

pytestmark = pytest.mark.gpu


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def load_opt_state(eng, st):
    eng.load_optimizer_state(st["step"], st.get("exp_avg"), st.get("exp_avg_sq", st.get("square_avg")))


def n_uniq(batch):
    return np.unique(batch[0]).size, np.unique(batch[1]).size


def assert_parts_close(got, ref, batch, what, row_floor=False):
    """Every loss part at REL of itself.  ``row_floor`` (the edge cases, which drive a side down to ONE unique row, where
    its InfoNCE part is exactly 0): an InfoNCE part at REL x max(|part|, n_uniq) -- each row's term is a residue of O(1)
    numbers, which helpers.grad_scale_floor is the precedent for."""
    floors = (0, 0) + (n_uniq(batch) if row_floor else (0, 0))
    for name, g_, r_, floor in zip(("bpr", "reg", "cl_user", "cl_item"), got, ref, floors):
        bound = REL * max(abs(r_), floor)
        print(f"  {what} {name}: got {g_!r}, reference {r_!r}, err {abs(g_ - r_):.3e}, bound {bound:.3e}")
        assert abs(g_ - r_) <= bound + 1e-12, f"{what} {name}: got {g_!r}, reference {r_!r}"


@pytest.mark.parametrize("case", CASES)
def test_steps_match_reference(hip_device, case):
    """Each step from the reference's own weights and optimizer state, with its recorded noise: the loss parts at REL,
    the gradients within REL of scale of the reference's fp64 gradients plus twice the reference's own fp32 distance
    from them, the updated weights inside the optimizer band.  Then the three steps chained from w0: plain SGD every
    element within REL of the largest update, Adam / RMSprop every element inside the legal-trajectory envelope (zero
    outliers)."""
    g = load_golden(case)
    m, hp, graph = sim_meta(g), sim_hp(g), sim_graph(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    eng = make_engine(g, device_str="cuda:0")
    eng.model.train()
    for s in range(m["n_steps"]):
        batch, noise = sim_batch(g, s), g["noise"][s]
        w0, st0 = sim_params(g, f"w{s}"), sim_opt_state(g, s, opt)
        load_weights(eng, w0)
        load_opt_state(eng, st0)
        loss, grads = eng.backward_only(batch, noise=noise)
        print(f"{case} step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        assert_parts_close(eng.last_losses(), g["parts"][s], batch, f"step {s}")
        g_ref = sim_params(g, f"g{s + 1}")
        for k in KEYS:
            got, exact = grads[k].cpu().numpy(), g[f"g64_{s + 1}/{k}"]
            print(f"  grad {k}: err vs fp64 {np.abs(got - exact).max():.3e} (the reference's "
                  f"{np.abs(g_ref[k] - exact).max():.3e}) of scale {np.abs(exact).max():.3e}")
            assert_as_accurate_as_reference(got, g_ref[k], exact, what=f"grad {k} step {s}")
        assert float(eng._g_flat.abs().max()) == 0.0
        load_opt_state(eng, st0)
        loss = eng.train_single_batch(batch, noise=noise)
        assert_scalar_close(loss, g["losses"][s], what=f"loss (step) {s}")
        band = sim_band(w0, st0, g_ref, opt, lr)
        w1 = get_weights(eng)
        for k in KEYS:
            assert_step_close(w0[k], w1[k], g[f"w{s + 1}/{k}"], band[k], what=f"weights {k} step {s}")
        assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"
    # chained
    w0 = sim_params(g, "w0")
    load_weights(eng, w0)
    load_opt_state(eng, sim_opt_state(g, 0, opt))
    for s in range(m["n_steps"]):
        loss = eng.train_single_batch(sim_batch(g, s), noise=g["noise"][s])
        print(f"  chained step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")

    def grad_fn(w, s):
        return sx.simgcl_grads(w, graph, hp, sim_batch(g, s), g["noise"][s])[2]

    w_ref, env, upd = oracle_trajectory(w0, list(range(m["n_steps"])), grad_fn,
                                        lambda w, gr, st: sx.opt_step(w, gr, st, opt, lr),
                                        lambda w: sx.new_opt_state(w, opt), trials=0 if opt == "sgd" else 8)
    ref_end = sim_params(g, f"w{m['n_steps']}")
    if opt == "sgd":
        assert_sgd_exact(get_weights(eng), ref_end, w0, f"{case} chained weights")
    else:
        assert_on_trajectory(get_weights(eng), ref_end, env, upd, f"{case} chained weights")


def test_predict_factors_and_recommend_read_the_raw_tables(hip_device):
    """predict is the dot product of the raw table rows (simgcl.py:72-82), before and after a step; ranking_factors hands
    the same tables to the top-K path; ids out of range raise and leave the model usable."""
    import beta_recsys_amd as hp_pkg

    g = load_golden("simgcl_adam")
    m = sim_meta(g)
    eng = make_engine(g, device_str="cuda:0")
    load_weights(eng, sim_params(g, f"w{m['n_steps']}"))
    got = eng.model.predict(g["predict_users"], g["predict_items"])
    assert got.dtype == torch.float32 and tuple(got.shape) == (g["predict_users"].size,)
    assert_tensor_close(got.cpu().numpy(), g["predict_scores"], what="predict vs the reference")
    eng.train_single_batch(sim_batch(g, 0), noise=g["noise"][0])
    w1 = get_weights(eng)
    users, items = np.repeat(np.arange(m["U"]), m["I"]), np.tile(np.arange(m["I"]), m["U"])
    ref = sx.simgcl_predict(to64(w1), users, items)
    assert_tensor_close(eng.model.predict(users, items).cpu().numpy(), ref, what="predict after a step")
    U_f, I_f, alpha, bias = eng.model.ranking_factors()
    assert bias is None and alpha == 1.0
    assert np.array_equal(U_f.cpu().numpy(), w1[KEYS[0]]) and np.array_equal(I_f.cpu().numpy(), w1[KEYS[1]])
    top, _ = hp_pkg.recommend(eng.model, np.arange(m["U"]), 5)
    dense, top = ref.reshape(m["U"], m["I"]), top.cpu().numpy()
    for u in range(m["U"]):
        kth = np.sort(dense[u])[-5]
        assert len(set(top[u])) == 5 and np.all(dense[u][top[u]] >= kth - 1e-5 * np.abs(dense[u]).max()), f"user {u}"
    with pytest.raises(IndexError):
        eng.model.predict([0, m["U"]], [0, 0])
    with pytest.raises(IndexError):
        eng.model.predict([0, 0], [0, -1])
    assert np.isfinite(eng.model.predict([0], [0]).cpu().numpy()).all()


@pytest.mark.parametrize("L,n,D,seed,step", [(1, 7, 1, 0, 0), (3, 50, 40, 1234, 5), (4, 33, 256, 2 ** 63 + 11, 2 ** 31 - 1)])
def test_device_noise_equals_the_restatement_bit_for_bit(hip_device, L, n, D, seed, step):
    from beta_recsys_amd import _lib

    lib = _lib.load()
    out = torch.empty(2, L, n, D, dtype=torch.float32, device="cuda:0")
    _lib.check(lib.hiprec_simgcl_noise(seed, step, L, n, D, _lib.ptr(out), _lib.stream_ptr(out.device)))
    assert np.array_equal(out.cpu().numpy(), sx.device_uniforms(seed, step, L, n, D))


@pytest.mark.parametrize("case", ["simgcl_adam", "simgcl_sgd_hot_l3"])
def test_drawn_step_equals_the_step_fed_its_materialised_noise(hip_device, case):
    """A step with the device draw equals, within REL of scale, the same step fed ``draw_noise`` of that (seed, step):
    the two sources of u share everything after it.  Two steps of one engine draw different noise, and the noise of a
    step is the restatement's."""
    g = load_golden(case)
    m = sim_meta(g)
    eng = make_engine(g, device_str="cuda:0", noise_seed=99)
    load_weights(eng, sim_params(g, "w0"))
    batch = sim_batch(g, 0)
    results = []
    for _ in range(2):
        step = eng.noise_step
        noise = eng.draw_noise(step)
        assert np.array_equal(noise.cpu().numpy(), sx.device_uniforms(99, step, m["L"], m["U"] + m["I"], m["D"]))
        loss_d, grads_d = eng.backward_only(batch)
        parts_d = eng.last_losses()
        assert eng.noise_step == step + 1
        loss_m, grads_m = eng.backward_only(batch, noise=noise)
        assert_scalar_close(loss_d, loss_m, what="drawn vs materialised loss")
        assert_parts_close(parts_d, eng.last_losses(), batch, "drawn vs materialised")
        for k in KEYS:
            assert_tensor_close(grads_d[k].cpu().numpy(), grads_m[k].cpu().numpy(), what=f"drawn vs materialised grad {k}")
        results.append((step, noise.cpu().numpy(), parts_d))
    (s0, n0, p0), (s1, n1, p1) = results
    assert s1 == s0 + 2 and not np.array_equal(n0, n1), "two steps drew the same noise"
    assert_scalar_close(p0[0], p1[0], what="the clean view takes no noise: the same BPR part")
    assert abs(p0[3] - p1[3]) > 10 * REL * abs(p0[3]), "other noise moved no InfoNCE part: the test shows nothing"


def test_two_views_is_the_restatement_with_that_defect(hip_device):
    g = load_golden("simgcl_adam")
    graph, batch, noise = sim_graph(g), sim_batch(g, 0), g["noise"][0]
    w0 = sim_params(g, "w0")
    eng = make_engine(g, device_str="cuda:0", user_view="two_views")
    load_weights(eng, w0)
    loss, grads = eng.backward_only(batch, noise=noise)
    with float64_oracle(sx):
        parts, l64, g64 = sx.simgcl_grads(to64(w0), graph, sim_hp(g), batch, noise, defect="user_view2")
        _, l_ref, _ = sx.simgcl_grads(to64(w0), graph, sim_hp(g), batch, noise)
    assert abs(l64 - l_ref) > 100 * REL * abs(l_ref)
    assert_scalar_close(loss, l64, what="two_views loss")
    assert_parts_close(eng.last_losses(), parts, batch, "two_views")
    for k in KEYS:
        assert_tensor_close(grads[k].cpu().numpy(), g64[k], what=f"two_views grad {k}")


def test_out_of_range_ids_raise(hip_device):
    """A user, positive or negative id outside its table raises IndexError (nothing is stamped, read or written out of
    range) and the engine stays usable."""
    g = load_golden("simgcl_adam")
    m = sim_meta(g)
    eng = make_engine(g, device_str="cuda:0")
    users, pos, neg = (a.copy() for a in sim_batch(g, 0))
    for what, (arr, idx, val) in {"user": (0, 3, m["U"]), "negative user": (0, 0, -1), "pos": (1, 5, m["I"]),
                                  "neg": (2, 7, m["I"]), "negative neg": (2, 0, -1)}.items():
        b = [users.copy(), pos.copy(), neg.copy()]
        b[arr][idx] = val
        with pytest.raises(IndexError):
            eng.train_single_batch(tuple(b), noise=g["noise"][0])
        assert float(eng._g_flat.abs().max()) == 0.0, what
        assert torch.isfinite(eng.model.flat).all(), what
    load_weights(eng, sim_params(g, "w0"))
    eng.load_optimizer_state(0)
    assert_scalar_close(eng.train_single_batch((users, pos, neg), noise=g["noise"][0]), g["losses"][0],
                        what="usable after the errors")
    with pytest.raises(ValueError, match="noise is"):
        eng.train_single_batch((users, pos, neg), noise=g["noise"][0][:1])


def test_epoch_trains(hip_device, capsys):
    g = load_golden("simgcl_adam")
    m = sim_meta(g)
    eng = make_engine(g, device_str="cuda:0")
    load_weights(eng, sim_params(g, "w0"))
    batches = [tuple(torch.from_numpy(a) for a in sim_batch(g, s)) for s in range(m["n_steps"])]
    eng.train_an_epoch(batches, 0)
    assert "[Training Epoch 0], Loss" in capsys.readouterr().out
    w = get_weights(eng)
    assert all(np.isfinite(w[k]).all() and np.abs(w[k] - g[f"w0/{k}"]).max() > 0 for k in KEYS)
    assert eng.noise_step == m["n_steps"]
