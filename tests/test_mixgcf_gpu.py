"""GPU parity tests of MixGCF (csrc/mixgcf.hip): every golden fixture in torch_cpu mode (loss, choice, the gradient
buffer, weights and moments), predict / ranking_factors / recommend, out-of-range ids, checkpoints and the device draw
mode, against the reference's vectors (tests/golden/mix_*.npz) and the numpy restatement."""
import numpy as np
import pytest
import torch

import mixgcf_edges as me
import mixgcf_numpy as mx
from helpers import REL, assert_scalar_close, assert_step_close, assert_tensor_close, float64_oracle, load_golden, to64
from test_mixgcf_host import make_engine
from test_oracle_golden_mixgcf import CASES, KEYS, mix_band, mix_batch, mix_graph, mix_hp, mix_masks, mix_meta
from test_oracle_golden_mixgcf import mix_opt_state, mix_params

pytestmark = pytest.mark.gpu


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def load_opt_state(eng, st):
    eng.load_optimizer_state(st["step"], st.get("exp_avg"), st.get("exp_avg_sq", st.get("square_avg")))


def seed_for_step(g, s):
    """Put the CPU generator where the reference's was before step s (its draws are the fixture's)."""
    m, hp = mix_meta(g), mix_hp(g)
    N, nnz, H = m["U"] + m["I"], g["adj_val"].size, m["L"] + 1
    torch.manual_seed(int(g["torch_seed"]))
    for _ in range(s):
        for _l in range(m["L"]):
            if hp["edge_rate"] is not None:
                torch.rand(nnz)
            if hp["mess_rate"]:
                torch.empty(N, m["D"]).bernoulli_(1 - hp["mess_rate"])
        if hp["ns"] != "rns":
            for _k in range(m["K"]):
                torch.rand(m["B"], 1, H, 1)


@pytest.mark.parametrize("case", CASES)
def test_step_matches_reference(hip_device, case):
    """Each step from the reference's own weights and optimizer state, the draws replayed from the torch seed: loss,
    choice, the gradient buffer after _enqueue_grad, the updated weights and moments."""
    g = load_golden(case)
    m, hp = mix_meta(g), mix_hp(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    eng = make_engine(g, device_str="cuda:0")
    eng.model.train()
    for s in range(m["n_steps"]):
        batch = mix_batch(g, s)
        w0, st0 = mix_params(g, f"w{s}"), mix_opt_state(g, s, opt)
        load_weights(eng, w0)
        load_opt_state(eng, st0)
        seed_for_step(g, s)
        loss, grads = eng.backward_only(batch)
        print(f"{case} step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        assert np.array_equal(eng.last_choice().cpu().numpy(), g["choice"][s]), f"choice step {s}"
        if hp["ns"] != "rns":
            assert np.array_equal(eng.last_seeds().cpu().numpy(), g["seeds"][s])
        order = eng.model.graph()["order"].numpy()
        for l in range(m["L"]):
            if hp["edge_rate"] is not None:
                assert np.array_equal(eng.model.last_edge_keep(l).cpu().numpy(), g["edge_keep"][s][l][order])
            if hp["mess_rate"]:
                assert np.array_equal(eng.model.last_mess_keep(l).cpu().numpy(), g["mess_keep"][s][l])
        g_ref = mix_params(g, f"g{s + 1}")
        for k in KEYS:
            got = grads[k].cpu().numpy()
            print(f"  grad {k}: max err {np.abs(got - g_ref[k]).max():.3e} of scale {np.abs(g_ref[k]).max():.3e}")
            assert_tensor_close(got, g_ref[k], what=f"grad {k} step {s}")
        assert float(eng._g_flat.abs().max()) == 0.0
        # the full step
        load_opt_state(eng, st0)
        seed_for_step(g, s)
        loss = eng.train_single_batch(batch)
        assert_scalar_close(loss, g["losses"][s], what=f"loss (step) {s}")
        band = mix_band(w0, st0, g_ref, opt, lr)
        w1 = get_weights(eng)
        for k in KEYS:
            assert_step_close(w0[k], w1[k], g[f"w{s + 1}/{k}"], band[k], what=f"weights {k} step {s}")
        nxt = mix_opt_state(g, s + 1, opt)
        views = {"exp_avg": eng.optimizer.exp_avg, "exp_avg_sq": eng.optimizer.exp_avg_sq}
        for name, ref_name in (("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq" if opt == "adam" else "square_avg")):
            if views[name] is None:
                continue
            got = {k: v.cpu().numpy() for k, v in eng.model.views(views[name]).items()}
            for k in KEYS:
                assert_tensor_close(got[k], nxt[ref_name][k], REL if name == "exp_avg" else 2 * REL, f"{name} {k} step {s}")
        assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"


@pytest.mark.parametrize("pool", mx.POOLS)
def test_predict_factors_and_recommend(hip_device, pool):
    """predict and ranking_factors against the restatement for every pool; recommend() returns the top-K of a dense
    ranking of predict."""
    import beta_recsys_amd as hp_pkg

    g = load_golden("mix_concat_adam")
    m, graph = mix_meta(g), mix_graph(g)
    hp = dict(mix_hp(g), pool=pool)
    eng = make_engine(g, device_str="cuda:0", pool=pool)
    w = mix_params(g, "w1")
    load_weights(eng, w)
    users, items = np.repeat(np.arange(m["U"]), m["I"]), np.tile(np.arange(m["I"]), m["U"])
    with float64_oracle(mx):
        ref = mx.mix_predict(to64(w), graph, hp, users, items)
        fu, fi = mx.mix_factors(to64(w), graph, hp)
    eng.model.train()                       # predict draws nothing and drops nothing, whatever the mode
    state = torch.get_rng_state()
    scores = eng.model.predict(users, items)
    assert torch.equal(torch.get_rng_state(), state)
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (users.size,)
    assert_tensor_close(scores.cpu().numpy(), ref, what=f"{pool} predict")
    U_f, I_f, alpha, bias = eng.model.ranking_factors()
    assert alpha == 1.0 and bias is None
    assert tuple(U_f.shape) == (m["U"], m["D"] * (m["L"] + 1 if pool == "concat" else 1))
    assert_tensor_close(U_f.cpu().numpy(), fu, what=f"{pool} user factors")
    assert_tensor_close(I_f.cpu().numpy(), fi, what=f"{pool} item factors")
    top, _ = hp_pkg.recommend(eng.model, np.arange(m["U"]), 5)
    dense = scores.cpu().numpy().reshape(m["U"], m["I"]).astype(np.float64)
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
    """A user, positive or candidate id outside its table raises IndexError (the row is skipped whole, nothing is read
    or written out of range) and the engine stays usable."""
    g = load_golden("mix_concat_adam")
    m = mix_meta(g)
    eng = make_engine(g, device_str="cuda:0")
    users, pos, neg = (a.copy() for a in mix_batch(g, 0))
    for what, (arr, idx, val) in {"user": (0, 3, m["U"]), "negative user": (0, 0, -1), "pos": (1, 5, m["I"]),
                                  "candidate": (2, (7, m["K"] * m["n_negs"] - 1), m["I"]),
                                  "negative candidate": (2, (0, 0), -1)}.items():
        b = [users.copy(), pos.copy(), neg.copy()]
        b[arr][idx] = val
        with pytest.raises(IndexError):
            eng.train_single_batch(tuple(b))
        assert float(eng._g_flat.abs().max()) == 0.0, what
        assert torch.isfinite(eng.model.flat).all(), what
    load_weights(eng, mix_params(g, "w0"))
    seed_for_step(g, 0)
    assert_scalar_close(eng.train_single_batch((users, pos, neg)), g["losses"][0], what="usable after the errors")


def test_checkpoint_resume_gives_the_same_next_step(hip_device, tmp_path):
    """Weights and optimizer state through a checkpoint into a fresh engine: its next step is the original engine's
    next step -- the same loss, and weights inside the optimizer band of a gradient that is right to REL (the scatter's
    float atomics land in run order, so two runs of one step differ in the last bits)."""
    g = load_golden("mix_sum_rmsprop")
    opt, lr = str(g["optimizer"]), float(g["lr"])
    eng = make_engine(g, device_str="cuda:0")
    load_weights(eng, mix_params(g, "w0"))
    seed_for_step(g, 0)
    eng.train_single_batch(mix_batch(g, 0))
    path = str(tmp_path / "mixgcf.pt")
    eng.save_checkpoint(path, optimizer_state=True)
    w1 = get_weights(eng)
    seed_for_step(g, 1)
    loss_a = eng.train_single_batch(mix_batch(g, 1))
    w_a = get_weights(eng)
    other = make_engine(g, device_str="cuda:0")
    other.resume_checkpoint(path, optimizer_state=True)
    for k in KEYS:
        assert np.array_equal(get_weights(other)[k], w1[k]), k
    seed_for_step(g, 1)
    loss_b = other.train_single_batch(mix_batch(g, 1))
    w_b = get_weights(other)
    assert_scalar_close(loss_b, loss_a, what="loss after resume")
    band = mix_band(w1, mix_opt_state(g, 1, opt), mix_params(g, "g2"), opt, lr)
    for k in KEYS:
        assert_step_close(w1[k], w_b[k], w_a[k], band[k], what=f"weights {k} after resume")
        assert_tensor_close(other.model.views(other.optimizer.exp_avg_sq)[k].cpu().numpy(),
                            eng.model.views(eng.optimizer.exp_avg_sq)[k].cpu().numpy(), 2 * REL, f"square_avg {k}")


@pytest.mark.parametrize("case", ["mix_mean_sgd_drop", "mix_final_adam_hot", "mix_sum_rmsprop"])
def test_device_draw_mode(hip_device, case):
    """dropout_rng = seed_rng = "device": the masks and seeds the kernel used are read back and the step is held to the
    fp64 restatement under them; the CPU generator is not touched.  Kept shares: a binomial(n, q) count lies within
    5 sigma = 5 sqrt(n q (1 - q)) of n q except once in 1.7e6 draws -- edges survive with q = rate (the reference's
    arithmetic), message elements with q = 1 - p."""
    g = load_golden(case)
    m, hp, graph = mix_meta(g), mix_hp(g), mix_graph(g)
    eng = make_engine(g, device_str="cuda:0", dropout_rng="device", seed_rng="device", dropout_seed=11)
    eng.model.train()
    w0 = mix_params(g, "w0")
    load_weights(eng, w0)
    state = torch.get_rng_state()
    loss, grads = eng.backward_only(mix_batch(g, 0))
    assert torch.equal(torch.get_rng_state(), state)
    seeds = eng.last_seeds().cpu().numpy()
    assert seeds.shape == (m["B"], m["K"], m["L"] + 1) and (seeds >= 0).all() and (seeds < 1).all()
    order = eng.model.graph()["order"].numpy()
    inv = np.empty_like(order)
    inv[order] = np.arange(order.size)
    edge, mess = [], []
    for l in range(m["L"]):
        if hp["edge_rate"] is not None:
            edge.append(eng.model.last_edge_keep(l).cpu().numpy()[inv])     # back to COO order
        if hp["mess_rate"]:
            mess.append(eng.model.last_mess_keep(l).cpu().numpy())
    for arr, q in ((edge, hp["edge_rate"]), (mess, None if not hp["mess_rate"] else 1 - hp["mess_rate"])):
        if arr:
            n = sum(a.size for a in arr)
            kept = sum(int(a.sum()) for a in arr)
            assert abs(kept - n * q) <= 5 * np.sqrt(n * q * (1 - q)), (kept, n, q)
            assert len(arr) == 1 or not np.array_equal(arr[0], arr[1]), "two hops drew the same mask"
    masks = (edge or None, mess or None)
    choice = eng.last_choice().cpu().numpy()
    # the choice by the rule of tests/mixgcf_edges.py (every pick within its fp32 bound of the fp64 maximum), then loss and
    # gradients under that choice
    held = dict(w=w0, graph=graph, hp=hp, batch=mix_batch(g, 0), seeds=seeds, masks=masks, U=m["U"], D=m["D"], L=m["L"])
    off = me.check_choice(held, choice, f"{case} device draws")
    print(f"{case}: {off} of {choice.size} choices differ from the fp64 argmax (inside the bound)")
    me.check_step(held, loss, {k: v.cpu().numpy() for k, v in grads.items()}, choice, f"{case} device draws")
    loss2, _ = eng.backward_only(mix_batch(g, 0))
    assert loss2 != loss or hp["edge_rate"] is None and not hp["mess_rate"], "the next step drew the same numbers"
