"""The MixGCF restatement (tests/mixgcf_numpy.py) against golden vectors captured from the real reference
(tests/golden/mix_*.npz, tools/gen_golden_mixgcf.py): the reference's own loss tensor, autograd's gradients of it and
torch.optim's step on them.  CPU only."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import mixgcf_numpy as mx
from helpers import REL, assert_on_trajectory, assert_scalar_close, assert_sgd_exact, assert_step_close
from helpers import assert_tensor_close, copy_state, float64_oracle, load_golden, oracle_trajectory, to64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["mix_concat_adam", "mix_mean_sgd_drop", "mix_sum_rmsprop", "mix_final_adam_hot", "mix_rns_sgd"]
KEYS = mx.KEYS
MARGIN = 1e-4


def mix_params(g, prefix):
    return {k: g[f"{prefix}/{k}"].astype(np.float32).copy() for k in KEYS}


def mix_meta(g):
    U, I, D, L, B, n_negs, K, n_steps, seed = (int(x) for x in g["meta"])
    return dict(U=U, I=I, D=D, L=L, B=B, n_negs=n_negs, K=K, n_steps=n_steps, seed=seed)


def rate(x):
    return None if np.isnan(float(x)) else float(x)


def mix_hp(g):
    m = mix_meta(g)
    return dict(pool=str(g["pool"]), L=m["L"], n_negs=m["n_negs"], K=m["K"], ns=str(g["ns"]), l2=float(g["l2"]),
                edge_rate=rate(g["edge_rate"]), mess_rate=rate(g["mess_rate"]))


def mix_graph(g):
    m = mix_meta(g)
    return g["adj_row"], g["adj_col"], g["adj_val"], m["U"] + m["I"]


def mix_masks(g, s):
    """(edge, mess) of step s: per hop arrays or None, the edge masks in COO order."""
    e, ms = g["edge_keep"][s], g["mess_keep"][s]
    return (list(e) if e.shape[0] else None, list(ms) if ms.shape[0] else None)


def mix_batch(g, s):
    return g["users"][s], g["pos"][s], g["neg"][s]


def mix_opt_state(g, step, opt):
    st = mx.new_opt_state(mix_params(g, "w0"), opt)
    st["step"] = step
    if step > 0 and opt == "adam":
        st["exp_avg"], st["exp_avg_sq"] = mix_params(g, f"m{step}"), mix_params(g, f"v{step}")
    elif step > 0 and opt == "rmsprop":
        st["square_avg"] = mix_params(g, f"v{step}")
    return st


def mix_band(w_prev, st_prev, g_ref, opt, lr, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel * its scale of g_ref (helpers.optimizer_band)."""
    outs = []
    for sign in (+1.0, -1.0):
        w = {k: v.copy() for k, v in w_prev.items()}
        st = copy_state(st_prev)
        g = {k: (g_ref[k] + np.float32(sign * rel * float(np.abs(g_ref[k]).max()))).astype(np.float32) for k in KEYS}
        mx.opt_step(w, g, st, opt, lr)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in KEYS}


def winner_gaps(g, s):
    """fp64: per (row, k, hop) the winner's lead over every candidate that is another item, minus MARGIN of the row's
    largest |score| (condition (a) holds where that is >= 0), and the fp64 argmax."""
    hp, graph, m = mix_hp(g), mix_graph(g), mix_meta(g)
    with float64_oracle(mx):
        E, _, _ = mx.propagate(to64(mix_params(g, f"w{s}")), graph, hp, mix_masks(g, s))
        cand = mx.candidates(g["neg"][s], hp)
        sc = mx.sampler_scores(E, m["U"], g["users"][s], g["pos"][s], cand, g["seeds"][s].astype(np.float64), hp["pool"])
    first = sc.argmax(axis=2)
    best = np.take_along_axis(sc, first[:, :, None, :], axis=2)
    other = cand[..., None] != np.take_along_axis(cand[..., None], first[:, :, None, :], axis=2)
    gap = np.where(other, best - sc, np.inf).min(axis=2)
    # (lead minus MARGIN of the scale, not their ratio: a user whose last hop lost every edge scores exactly 0 against
    # every candidate in any arithmetic, and the first candidate wins everywhere)
    return gap - MARGIN * np.abs(sc).max(axis=(1, 2, 3))[:, None, None], first


@pytest.mark.parametrize("case", CASES)
def test_every_step_in_isolation(case):
    g = load_golden(case)
    hp, graph, m = mix_hp(g), mix_graph(g), mix_meta(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    for s in range(m["n_steps"]):
        w0, st0 = mix_params(g, f"w{s}"), mix_opt_state(g, s, opt)
        loss, grads, choice = mx.mix_grads(w0, graph, hp, mix_batch(g, s), g["seeds"][s], mix_masks(g, s))
        assert_scalar_close(loss, g["losses"][s], what=f"{case} loss step {s}")
        assert np.array_equal(choice, g["choice"][s]), f"{case} choice step {s}"
        g_ref = mix_params(g, f"g{s + 1}")
        for k in KEYS:
            assert_tensor_close(grads[k], g_ref[k], what=f"{case} grad {k} step {s}")
        band = mix_band(w0, st0, g_ref, opt, lr)
        w1, st1 = {k: v.copy() for k, v in w0.items()}, copy_state(st0)
        mx.opt_step(w1, grads, st1, opt, lr)
        nxt = mix_opt_state(g, s + 1, opt)
        for k in KEYS:
            assert_step_close(w0[k], w1[k], g[f"w{s + 1}/{k}"], band[k], what=f"{case} weights {k} step {s}")
            for name in ("exp_avg", "exp_avg_sq", "square_avg"):
                if name in nxt:
                    assert_tensor_close(st1[name][k], nxt[name][k], REL if name == "exp_avg" else 2 * REL,
                                        f"{case} {name} {k} step {s}")


@pytest.mark.parametrize("case", ["mix_concat_adam", "mix_mean_sgd_drop"])
def test_chained_trajectory(case):
    g = load_golden(case)
    hp, graph, m = mix_hp(g), mix_graph(g), mix_meta(g)
    opt, lr = str(g["optimizer"]), float(g["lr"])
    steps = list(range(m["n_steps"]))

    def grad_fn(w, s):
        return mx.mix_grads(w, graph, hp, mix_batch(g, s), g["seeds"][s], mix_masks(g, s))[1]

    w0 = mix_params(g, "w0")
    w_ref, env, upd = oracle_trajectory(w0, steps, grad_fn, lambda w, gr, st: mx.opt_step(w, gr, st, opt, lr),
                                        lambda w: mx.new_opt_state(w, opt), trials=0 if opt == "sgd" else 8)
    ref_end = mix_params(g, f"w{m['n_steps']}")
    if opt == "sgd":
        assert_sgd_exact(w_ref, ref_end, w0, f"{case} final weights")
    else:
        assert_on_trajectory(w_ref, ref_end, env, upd, f"{case} trajectory")


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_agrees_with_fp32(case):
    g = load_golden(case)
    hp, graph = mix_hp(g), mix_graph(g)
    w0 = mix_params(g, "w0")
    l32, g32, c32 = mx.mix_grads(w0, graph, hp, mix_batch(g, 0), g["seeds"][0], mix_masks(g, 0))
    with float64_oracle(mx):
        l64, g64, c64 = mx.mix_grads(to64(w0), graph, hp, mix_batch(g, 0), g["seeds"][0], mix_masks(g, 0))
    assert g64[KEYS[0]].dtype == np.float64 and np.array_equal(c32, c64)
    assert_scalar_close(l32, l64, what="loss")
    for k in KEYS:
        assert_tensor_close(g32[k], g64[k], what=f"grad {k}")


@pytest.mark.parametrize("case", CASES)
def test_argmax_margins_and_reference_own_rounding_leave_room(case):
    """(a) every (row, k, hop) argmax wins by 1e-4 of the row's largest |score| in fp64 against every other item, so
    the reference's fp32, the restatement and a kernel all pick the same candidate; (b) the reference's own gradients
    lie within REL / 3 of the fp64 restatement's scale (the rule of test_reference_own_rounding_leaves_room)."""
    g = load_golden(case)
    hp, graph, m = mix_hp(g), mix_graph(g), mix_meta(g)
    for s in range(m["n_steps"]):
        if hp["ns"] != "rns":
            gap, first = winner_gaps(g, s)
            assert np.array_equal(first, g["choice"][s])
            assert gap.min() >= 0, f"{case} step {s}: a win misses the margin by {-gap.min():.2e}"
        with float64_oracle(mx):
            _, g64, _ = mx.mix_grads(to64(mix_params(g, f"w{s}")), graph, hp, mix_batch(g, s), g["seeds"][s],
                                     mix_masks(g, s))
        for k in KEYS:
            own = float(np.abs(g[f"g{s + 1}/{k}"] - g64[k]).max() / np.abs(g64[k]).max())
            assert own <= REL / 3, f"{case} step {s} {k}: the reference's own rounding is {own:.2e} of scale"
    if case == "mix_final_adam_hot":
        cand = mx.candidates(g["neg"][0], hp)
        assert any(len(set(r)) < len(r) for r in cand.reshape(-1, cand.shape[-1])), "no row repeats a candidate"
        assert len(set(zip(g["users"].reshape(-1), g["pos"].reshape(-1)))) <= 40


@pytest.mark.parametrize("case", CASES)
def test_rng_order_replay(case):
    """The same torch seed, drawn in the order of one reference step (per hop the edge rand(nnz), then the message
    bernoulli_; then per k the seed rand(B, 1, L + 1, 1)), gives the fixture's masks and seeds."""
    g = load_golden(case)
    hp, m = mix_hp(g), mix_meta(g)
    N, nnz, H = m["U"] + m["I"], g["adj_val"].size, m["L"] + 1
    torch.manual_seed(int(g["torch_seed"]))
    for s in range(m["n_steps"]):
        for l in range(m["L"]):
            if hp["edge_rate"] is not None:
                keep = torch.floor(hp["edge_rate"] + torch.rand(nnz)).type(torch.bool).numpy()
                assert np.array_equal(keep, g["edge_keep"][s][l] != 0), f"edge mask step {s} hop {l}"
            if hp["mess_rate"]:
                keep = torch.empty(N, m["D"]).bernoulli_(1 - hp["mess_rate"]).numpy()
                assert np.array_equal(keep != 0, g["mess_keep"][s][l] != 0), f"message mask step {s} hop {l}"
        if hp["ns"] != "rns":
            for k in range(m["K"]):
                sd = torch.rand(m["B"], 1, H, 1).view(m["B"], H).numpy()
                assert np.array_equal(sd, g["seeds"][s][:, k]), f"seeds step {s} k {k}"
    if hp["edge_rate"] is not None:   # a share `rate` of the edges SURVIVES (the reference's arithmetic, kept)
        share = float(g["edge_keep"].mean())
        assert abs(share - hp["edge_rate"]) < 4 * np.sqrt(0.25 / g["edge_keep"].size)


def test_predict_and_factors():
    for case in CASES:
        g = load_golden(case)
        hp, graph, m = mix_hp(g), mix_graph(g), mix_meta(g)
        w = mix_params(g, f"w{m['n_steps']}")
        sc = mx.mix_predict(w, graph, hp, g["predict_users"], g["predict_items"])
        assert_tensor_close(sc, g["predict_scores"], what=f"{case} predict")
        fu, fi = mx.mix_factors(w, graph, hp)
        assert fu.shape[1] == (m["D"] * (m["L"] + 1) if hp["pool"] == "concat" else m["D"])
        assert_tensor_close((fu[g["predict_users"]] * fi[g["predict_items"]]).sum(-1), g["predict_scores"],
                            what=f"{case} factors")


def test_mixgcf_is_wired_in():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib, compat, mixgcf

    assert compat.MIRRORS["beta_rec.models.mixgcf"] == "mixgcf"
    assert mixgcf.LightGCN is hp.MixGCF and mixgcf.LightGCNEngine is hp.MixGCFEngine and hasattr(mixgcf, "GraphConv")
    assert hp.LightGCN is not hp.MixGCF                     # the package's LightGCN stays lightgcn.py's
    assert ge.EVIDENCE_GROUPS["mixgcf"] == ge._EVIDENCE_COMMON + ["mixgcf.hip", "lightgcn.hip", "spmm.hpp"]
    assert ge.evidence_group("mixgcf_step") == "mixgcf"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hiprec.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("hiprec_mixgcf_plan_bytes", "hiprec_mixgcf_propagate", "hiprec_mixgcf_predict", "hiprec_mixgcf_grad"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name), name
