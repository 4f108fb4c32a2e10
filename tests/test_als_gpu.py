"""GPU: implicit ALS (csrc/als.hip) against the numpy restatement (tests/als_numpy.py).

Every half-sweep of three epochs is checked from the GPU's OWN input tables, read back before the call, so drift never
enters: the same half-sweep is solved in float64 (the truth) and in float32 with numpy's Cholesky (the yardstick).

* forward error: ``helpers.assert_as_accurate_as_reference(got, ref=x32, exact=x64)`` -- 1e-5 of scale plus twice the
  yardstick's own error;
* backward error: ``max rho(got) <= 4 max rho(x32)``, ``rho(x) = |A x - b| / (|A| |x| + |b|)`` in float64.  Both
  eliminations are backward stable with a constant proportional to D eps; the 4 is for the different summation and
  elimination order.  A wrong weight or a missing ``reg`` gives a rho near 1e-3 (tests/test_als_host.py);
* loss: within 1e-5 relative of the dense float64 loss of the read-back tables, and across half-sweeps it never rises
  by more than 2e-5 relative (two evaluations, each within 1e-5).
"""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import als_numpy as an
from helpers import assert_as_accurate_as_reference

pytestmark = pytest.mark.gpu


def make_engine(case, **extra):
    import beta_recsys_amd as hp

    cfg = dict(n_users=case["U"], n_items=case["I"], emb_dim=case["D"], alpha=case["alpha"], reg=case["reg"],
               device_str="cuda:0", **extra)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.ALSEngine({"model": cfg, "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    eng.model.load_state_dict({"user_factors.weight": torch.from_numpy(case["X0"]),
                               "item_factors.weight": torch.from_numpy(case["Y0"])})
    eng.prepare((case["users"], case["items"]))
    return eng


def tables(eng):
    sd = eng.model.state_dict()
    return sd["user_factors.weight"].cpu().numpy().copy(), sd["item_factors.weight"].cpu().numpy().copy()


@pytest.fixture(scope="module", params=list(an.FIXTURES))
def run(request, hip_device):
    """Three epochs on the GPU; per half-sweep the input tables, the result, the two numpy solves of the same input,
    the loss the GPU reports afterwards.  Computed once per fixture and left unchanged."""
    case = an.make_case(request.param)
    eng = make_engine(case)
    steps, losses = [], [(eng.loss(), tables(eng))]
    for _ in range(3):
        for side in ("users", "items"):
            X, Y = tables(eng)
            R, other = (case["R"], Y) if side == "users" else (case["R"].T, X)
            (eng.update_users if side == "users" else eng.update_items)()
            got = tables(eng)[0 if side == "users" else 1]
            x64 = an.half_sweep(R, other, case["alpha"], case["reg"], np.float64)
            x32 = an.half_sweep(R, other, case["alpha"], case["reg"], np.float32)
            rho = an.row_residuals(R, other, case["alpha"], case["reg"], got)
            rho32 = an.row_residuals(R, other, case["alpha"], case["reg"], x32)
            steps.append(dict(side=side, got=got, x64=x64, x32=x32, rho=rho, rho32=rho32,
                              untouched=tables(eng)[1 if side == "users" else 0], other=other))
            losses.append((eng.loss(), tables(eng)))
    return case, steps, losses


@pytest.mark.parametrize("n,D", [(9, 1), (70, 17), (257, 64), (230, 100), (300, 128), (64 * 128 + 37, 20)])
def test_gram_is_within_1e5_of_scale(hip_device, n, D):
    """The last shape has more 64-row tiles than slots, so the blocks walk their block-stride loop."""
    import beta_recsys_amd as hp

    rng = np.random.default_rng(n + D)
    F = (0.1 * rng.standard_normal((n, D))).astype(np.float32)
    model = hp.ALS(dict(n_users=n, n_items=n, emb_dim=D, reg=0.25, device_str="cuda:0"))
    G, G_reg = (t.cpu().numpy() for t in model.gram(torch.from_numpy(F).cuda()))
    exact = F.astype(np.float64).T @ F.astype(np.float64)
    err = np.abs(G - exact).max() / np.abs(exact).max()
    print(f"gram n={n} D={D}: max err / scale {err:.2e}")
    assert err <= 1e-5
    assert np.array_equal(G, G.T)
    assert np.array_equal(G_reg, G + np.float32(0.25) * np.eye(D, dtype=np.float32))


def test_half_sweeps_are_as_accurate_as_the_fp32_yardstick(run):
    case, steps, _ = run
    for k, s in enumerate(steps):
        what = f"{case['name']} half-sweep {k} ({s['side']})"
        print(f"{what}: forward gpu {an.forward_error(s['got'], s['x64']):.2e} yardstick "
              f"{an.forward_error(s['x32'], s['x64']):.2e}; rho gpu {s['rho'].max():.2e} yardstick {s['rho32'].max():.2e}")
    for k, s in enumerate(steps):
        what = f"{case['name']} half-sweep {k} ({s['side']})"
        assert np.isfinite(s["got"]).all(), what
        assert_as_accurate_as_reference(s["got"], ref=s["x32"], exact=s["x64"], what=what)
        assert s["rho"].max() <= 4 * s["rho32"].max(), (what, s["rho"].max(), s["rho32"].max())


def test_empty_rows_are_exact_zeros_and_the_other_table_is_untouched(run):
    case, steps, _ = run
    for s in steps:
        empty = an.EMPTY_USER if s["side"] == "users" else an.EMPTY_ITEM
        assert not s["got"][empty].any() and not np.signbit(s["got"][empty]).any()
        assert np.array_equal(s["untouched"], s["other"])
        assert np.abs(s["got"]).sum(axis=1).astype(bool).sum() == s["got"].shape[0] - 1


def test_loss_matches_the_dense_fp64_loss_and_never_rises(run):
    case, _, losses = run
    values = []
    for k, (got, (X, Y)) in enumerate(losses):
        want = an.dense_loss(case["R"], X, Y, case["alpha"], case["reg"])
        print(f"{case['name']} loss after {k} half-sweeps: gpu {got:.9g} dense fp64 {want:.9g} rel {abs(got - want) / want:.1e}")
        values.append((got, want))
    for got, want in values:
        assert abs(got - want) <= 1e-5 * abs(want), (case["name"], got, want)
    for (before, _), (after, _) in zip(values, values[1:]):
        assert after <= before * (1 + 2e-5), (case["name"], before, after)
    assert values[-1][0] < 0.5 * values[0][0]


@pytest.mark.parametrize("name", list(an.FIXTURES))
def test_runs_and_grids_give_the_same_bits(hip_device, name):
    """Two runs from the same tables are bit-identical, and ``als_blocks`` of 1 and 3 -- every row through one block's
    block-stride loop, or through three -- give the bits of the default grid."""
    case = an.make_case(name)
    results = []
    for extra in ({}, {}, {"als_blocks": 1}, {"als_blocks": 3}):
        eng = make_engine(case, **extra)
        eng.update_users()
        eng.update_items()
        results.append(eng.model.flat.cpu().numpy().copy())
    for other in results[1:]:
        assert np.array_equal(results[0].view(np.uint32), other.view(np.uint32))


@pytest.mark.parametrize("name", ["d17", "d64", "d128"])
def test_fold_in_returns_the_rows_update_users_wrote(hip_device, name):
    case = an.make_case(name)
    eng = make_engine(case)
    eng.update_users()
    flat = eng.model.flat.clone()
    X = eng.model.state_dict()["user_factors.weight"]
    ptr, idx, val = (t.cpu().numpy() for t in eng._b)
    picked = [an.HEAVY_USER, an.EMPTY_USER, 0, case["U"] - 1, 7]
    f_ptr = np.concatenate([[0], np.cumsum([ptr[u + 1] - ptr[u] for u in picked])])
    f_idx = np.concatenate([idx[ptr[u]:ptr[u + 1]] for u in picked])
    f_val = np.concatenate([val[ptr[u]:ptr[u + 1]] for u in picked])
    rows = eng.model.fold_in(f_ptr, f_idx, f_val)
    assert tuple(rows.shape) == (len(picked), case["D"]) and rows.dtype == torch.float32
    assert torch.equal(rows.view(torch.int32), X[picked].view(torch.int32))
    assert not rows[1].any()                                              # the empty list folds in to zeros
    assert torch.equal(eng.model.flat.view(torch.int32), flat.view(torch.int32))          # no table was touched
    # values=None reads every entry as one interaction
    ones = eng.model.fold_in(f_ptr, f_idx)
    assert torch.equal(ones, eng.model.fold_in(f_ptr, f_idx, np.ones_like(f_val)))
    assert not torch.equal(ones, rows)
    want = an.half_sweep((case["R"][picked] > 0).astype(np.float64), case["Y0"], case["alpha"], case["reg"], np.float64)
    assert an.forward_error(ones.cpu().numpy(), want) <= 1e-3
    assert tuple(eng.model.fold_in([0], []).shape) == (0, case["D"])
    assert not eng.model.fold_in([0, 0, 0], []).any()
    for bad in ([case["I"]], [-1]):
        with pytest.raises(IndexError):
            eng.model.fold_in([0, 1], bad)
    with pytest.raises(ValueError):
        eng.model.fold_in([0, 2], [1])
    assert torch.equal(eng.model.flat.view(torch.int32), flat.view(torch.int32))


def test_predict_recommend_evaluate_and_checkpoint(hip_device, tmp_path):
    import beta_recsys_amd as hp
    from beta_recsys_amd.recommend import topk_factors

    case = an.make_case("d17")
    eng = make_engine(case)
    with contextlib.redirect_stdout(io.StringIO()) as out:
        total = eng.train_an_epoch(None, 4)
    assert out.getvalue() == f"[Training Epoch 4], Loss {total}\n"
    assert ("model/loss", total, 4) in eng.writer.scalars and ("model/regularizer", eng.last_regularizer, 4) in eng.writer.scalars
    X, Y = tables(eng)
    assert 0 < eng.last_regularizer < total
    assert eng.last_regularizer == pytest.approx(case["reg"] * ((X.astype(np.float64) ** 2).sum()
                                                              + (Y.astype(np.float64) ** 2).sum()), rel=1e-5)
    rng = np.random.default_rng(3)
    users, items = rng.integers(0, case["U"], 300), rng.integers(0, case["I"], 300)
    scores = eng.model.predict(users, items).cpu().numpy()
    want = (X[users].astype(np.float64) * Y[items].astype(np.float64)).sum(axis=1)
    assert scores.dtype == np.float32 and np.abs(scores - want).max() <= 1e-5 * np.abs(want).max()
    with pytest.raises(IndexError):
        eng.model.predict([case["U"]], [0])
    # recommend() is topk_factors on the tables
    query = np.arange(case["U"])
    rec_items, rec_scores = eng.recommend(query, 10, seen=eng.seen_csr())
    Xd, Yd, scale, bias = eng.model.ranking_factors()
    ref_items, ref_scores = topk_factors(Xd, Yd, scale, bias, torch.from_numpy(query).cuda(), 10, seen=eng.seen_csr())
    assert torch.equal(rec_items, ref_items) and torch.equal(rec_scores, ref_scores)
    seen = case["R"] > 0
    assert not seen[np.repeat(query, 10), rec_items.cpu().numpy().ravel().clip(0)].any()
    metrics = hp.evaluate_full(eng, {"col_user": case["users"][:50], "col_item": case["items"][:50]}, k_li=(5, 10))
    assert set(metrics) >= {"ndcg@5", "ndcg@10"} and all(0.0 <= v <= 1.0 for v in metrics.values())
    # checkpoint round trip
    path = str(tmp_path / "als.pt")
    eng.save_checkpoint(path)
    other = make_engine(case)
    assert not torch.equal(other.model.flat, eng.model.flat)
    with contextlib.redirect_stdout(io.StringIO()):
        other.resume_checkpoint(path)
    assert torch.equal(other.model.flat.view(torch.int32), eng.model.flat.view(torch.int32))
    assert other.loss() == eng.loss()
    with pytest.raises(NotImplementedError):
        eng.train_single_batch((users, items))
    unprepared = hp.ALSEngine.__new__(hp.ALSEngine)
    unprepared.__dict__.update(eng.__dict__, _b=None)
    with pytest.raises(RuntimeError, match="prepare"):
        unprepared.update_users()


def test_a_nan_row_raises_and_leaves_the_dependent_rows_unchanged(hip_device):
    """A numeric flag, not a fault: every pivot that meets the NaN fails its comparison, the row is left as it was and
    the device counter says how many."""
    case = an.make_case("d17")
    eng = make_engine(case)
    eng.update_users()
    eng.update_items()
    X0, Y0 = tables(eng)
    sd = eng.model.state_dict()
    sd["item_factors.weight"][9, 2] = float("nan")       # G = Y^T Y is NaN throughout: every user row depends on it
    with pytest.raises(FloatingPointError, match=f"{case['U'] - 1} of {case['U']}"):
        eng.update_users()
    X1, Y1 = tables(eng)
    assert np.array_equal(X1.view(np.uint32), X0.view(np.uint32))
    assert np.isnan(Y1[9, 2]) and np.isnan(Y1).sum() == 1
    sd["item_factors.weight"][9, 2] = float(Y0[9, 2])
    eng.update_users()                                                     # the engine stays usable
    assert np.isfinite(tables(eng)[0]).all()
