"""Host-side checks of implicit ALS that need no GPU: the symbols are declared, exported and bound; the workspace and the
argument validation of every entry point; the config errors; a CPU model refuses to compute; the evidence group; and
the numpy restatement (tests/als_numpy.py) against itself -- the D = 1 closed form, sparse loss = dense loss, a loss
that never rises, fixtures that carry the bound the GPU tests lean on, and three named defects that land outside it."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest

import als_numpy as an

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hiprec_als_workspace_bytes", "hiprec_als_gram", "hiprec_als_solve_rows", "hiprec_als_loss")
NONE = (1 << 64) - 1           # hiprec_als_workspace_bytes for a bad shape
CFG = dict(n_users=10, n_items=20, emb_dim=8, device_str="cpu")


def test_symbols_are_declared_exported_and_bound():
    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib, als

    header = open(os.path.join(ROOT, "include", "hiprec.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in header, f"{name} is not declared in include/hiprec.h"
        assert name in _lib.SIGNATURES, f"_lib.py has no prototype for {name}"
        assert hasattr(lib, name), f"libhiprec.so does not export {name}"
    assert f"#define HIPREC_ALS_MAX_DIM {als.MAX_DIM}" in header
    assert f"#define HIPREC_ALS_MAX_BLOCKS {als.MAX_BLOCKS}" in header
    assert lib.hiprec_version() == 100
    assert hp.ALS is als.ALS and hp.ALSEngine is als.ALSEngine
    assert issubclass(hp.ALS, hp.flat_engine._FlatModel) and issubclass(hp.ALSEngine, hp.ModelEngine)
    for method in ("predict", "ranking_factors", "fold_in"):
        assert callable(getattr(hp.ALS, method)), method
    for method in ("prepare", "update_users", "update_items", "loss", "train_an_epoch", "train_single_batch",
                   "recommend", "save_checkpoint", "resume_checkpoint"):
        assert callable(getattr(hp.ALSEngine, method)), method


def test_evidence_group_exists():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    assert ge.EVIDENCE_GROUPS["als"] == ["common.hpp", "util.hip", "als.hip"]
    assert ge.evidence_group("als_sweep") == "als" and ge.evidence_group("adam") == "mf"
    assert os.path.exists(os.path.join(ge.CSRC, "als.hip"))


def test_workspace_bytes_follow_the_shape():
    from beta_recsys_amd import _lib

    ws = _lib.load().hiprec_als_workspace_bytes
    # Gram slots: one per 64 rows of the longer side, at most 128, each [pad16(D)]^2 floats; then 16 B per user
    assert ws(10, 20, 8) == 1 * 16 * 16 * 4 + 16 * 10
    assert ws(10, 65, 17) == 2 * 32 * 32 * 4 + 16 * 10
    assert ws(200, 65, 16) == 4 * 16 * 16 * 4 + 16 * 200
    assert ws(6040, 3706, 64) == 95 * 64 * 64 * 4 + 16 * 6040
    assert ws(100000, 3706, 128) == 128 * 128 * 128 * 4 + 16 * 100000
    assert ws(1, 1, 1) == 16 * 16 * 4 + 16
    for bad in ((0, 5, 8), (5, 0, 8), (-1, 5, 8), (5, 5, 0), (5, 5, 129), (5, 5, -3), (1 << 31, 5, 8), (5, 1 << 31, 8)):
        assert ws(*bad) == NONE, bad


def test_entry_points_validate_before_touching_the_gpu():
    """(the non-NULL pointers are never dereferenced: validation fails first)"""
    from beta_recsys_amd import _lib

    lib = _lib.load()
    P = 64

    def gram(F=P, n=10, dim=8, reg=0.1, G=P, Gr=P, work=P, work_bytes=1 << 20):
        return lib.hiprec_als_gram(F, n, dim, reg, G, Gr, work, work_bytes, None)

    for bad in (dict(n=0), dict(n=-4), dict(n=1 << 31), dict(dim=0), dict(dim=129)):
        assert gram(**bad) == -1 and b"bad shape" in lib.hiprec_last_error(), bad
    assert gram(reg=float("nan")) == -1 and b"reg" in lib.hiprec_last_error()
    for null in ("F", "G", "Gr"):
        assert gram(**{null: None}) == -1 and b"NULL" in lib.hiprec_last_error(), null
    assert gram(work=None) == -1 and b"workspace" in lib.hiprec_last_error()
    assert gram(work_bytes=16 * 16 * 4 - 1) == -1 and b"workspace" in lib.hiprec_last_error()

    def solve(ptr=P, idx=P, val=P, order=None, n_rows=10, other=P, n_other=20, dim=8, Gr=P, alpha=40.0, out=P, blocks=0,
              failed=P, stats=P):
        return lib.hiprec_als_solve_rows(ptr, idx, val, order, n_rows, other, n_other, dim, Gr, alpha, out, blocks,
                                         failed, stats, None)

    for bad in (dict(n_rows=-1), dict(n_rows=1 << 31), dict(n_other=0), dict(n_other=1 << 31), dict(dim=0), dict(dim=129)):
        assert solve(**bad) == -1 and b"bad shape" in lib.hiprec_last_error(), bad
    for bad_alpha in (-1.0, float("nan"), float("inf")):
        assert solve(alpha=bad_alpha) == -1 and b"alpha" in lib.hiprec_last_error()
    for bad_blocks in (-1, 1025):
        assert solve(blocks=bad_blocks) == -1 and b"blocks=" in lib.hiprec_last_error()
    assert solve(failed=None) == -1 and b"failed" in lib.hiprec_last_error()
    assert solve(stats=None) == -1 and b"stats" in lib.hiprec_last_error()
    for null in ("ptr", "idx", "val", "other", "Gr", "out"):
        assert solve(**{null: None}) == -1 and b"NULL" in lib.hiprec_last_error(), null
    assert solve(n_rows=0) == 0                                  # nothing to do: no launch

    def loss(ptr=P, idx=P, val=P, n_users=10, X=P, Y=P, n_items=20, dim=8, G=P, alpha=40.0, reg=0.1, work=P,
             work_bytes=1 << 20, out=P, stats=P):
        return lib.hiprec_als_loss(ptr, idx, val, n_users, X, Y, n_items, dim, G, alpha, reg, work, work_bytes, out, stats,
                                   None)

    for bad in (dict(n_users=0), dict(n_items=0), dict(n_users=1 << 31), dict(dim=0), dict(dim=129)):
        assert loss(**bad) == -1 and b"bad shape" in lib.hiprec_last_error(), bad
    assert loss(alpha=-2.0) == -1 and loss(reg=float("inf")) == -1
    assert loss(stats=None) == -1 and b"stats" in lib.hiprec_last_error()
    for null in ("ptr", "idx", "val", "X", "Y", "G", "out"):
        assert loss(**{null: None}) == -1 and b"NULL" in lib.hiprec_last_error(), null
    assert loss(work=None) == -1 and b"workspace" in lib.hiprec_last_error()
    assert loss(work_bytes=16 * 16 * 4 + 16 * 10 - 1) == -1 and b"workspace" in lib.hiprec_last_error()


def test_config_errors_and_the_cpu_refusal():
    import torch

    import beta_recsys_amd as hp

    for bad, match in ((dict(emb_dim=0), "emb_dim"), (dict(emb_dim=129), "emb_dim"), (dict(alpha=-1.0), "alpha"),
                       (dict(alpha=float("nan")), "alpha"), (dict(reg=0.0), "reg"), (dict(reg=-0.1), "reg"),
                       (dict(stddev=-1.0), "stddev"), (dict(als_blocks=-1), "als_blocks"),
                       (dict(als_blocks=1025), "als_blocks"), (dict(n_users=0), "n_users"), (dict(n_items=0), "n_users")):
        with pytest.raises(ValueError, match=match):
            hp.ALS(dict(CFG, **bad))
    torch.manual_seed(0)
    model = hp.ALS(dict(CFG, emb_dim=128, alpha=0.0))
    assert (model.alpha, model.reg, model.stddev, model.als_blocks) == (0.0, 0.1, 0.01, 0)
    assert hp.ALS(CFG).alpha == 40.0
    sd = model.state_dict()
    assert list(sd) == ["user_factors.weight", "item_factors.weight"]
    assert tuple(sd["user_factors.weight"].shape) == (10, 128) and tuple(sd["item_factors.weight"].shape) == (20, 128)
    assert 0.005 < float(sd["item_factors.weight"].std()) < 0.02
    other = hp.ALS(dict(CFG, emb_dim=128))
    other.load_state_dict(sd)
    assert torch.equal(other.flat, model.flat)
    X, Y, scale, bias = model.ranking_factors()
    assert X.data_ptr() == model.flat.data_ptr() and tuple(Y.shape) == (20, 128) and scale == 1.0 and bias is None
    # no CPU fallback anywhere
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.predict([0], [1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.fold_in([0, 1], [2])
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.ALSEngine({"model": CFG, "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    assert isinstance(eng.model, hp.ALS) and not hasattr(eng, "optimizer")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.prepare((np.array([0, 1]), np.array([2, 3])))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.train_an_epoch(None, 0)
    with pytest.raises(NotImplementedError, match="no batch step"):
        eng.train_single_batch(None)
    eng._dp_world = 2
    with pytest.raises(NotImplementedError, match="data-parallel"):
        eng.update_users()


# ---- the restatement against itself ------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=list(an.FIXTURES))
def trajectory(request):
    """Three epochs from the case's start tables, the way the GPU test walks them: every half-sweep is solved in float64
    and in float32 from the same float32 input tables, and the float32 result is the next input."""
    case = an.make_case(request.param)
    X, Y = case["X0"], case["Y0"]
    steps = []
    for _ in range(3):
        for side in ("users", "items"):
            R, other = (case["R"], Y) if side == "users" else (case["R"].T, X)
            x64 = an.half_sweep(R, other, case["alpha"], case["reg"], np.float64)
            x32 = an.half_sweep(R, other, case["alpha"], case["reg"], np.float32)
            if side == "users":
                X = x32
            else:
                Y = x32
            steps.append(dict(side=side, R=R, other=other, x64=x64, x32=x32, X=X, Y=Y))
    return case, steps


def test_fixtures_reach_what_they_are_named_for():
    for name, (U, I, D, alpha, reg, _, heavy) in an.FIXTURES.items():
        case = an.make_case(name)
        R = case["R"]
        assert R.shape == (U, I) and case["X0"].shape == (U, D) and case["Y0"].dtype == np.float32
        assert U >= 2 * D and I >= 2 * D, "both Gram matrices must have full rank for the fp32 yardstick to mean anything"
        assert R[an.EMPTY_USER].sum() == 0 and R[:, an.EMPTY_ITEM].sum() == 0 and R.max() == 3
        assert (R.sum(axis=1) > 0).sum() == U - 1 and (R.sum(axis=0) > 0).sum() == I - 1   # exactly one empty each
        counts = np.zeros_like(R)
        np.add.at(counts, (case["users"], case["items"]), 1)
        assert np.array_equal(counts, R) and case["users"].size == int(R.sum()) > int((R > 0).sum())
        if heavy == "all":
            assert (R[an.HEAVY_USER] > 0).sum() == I - 1 == 256        # four full chunks of 64
        elif heavy is not None:
            assert (R[an.HEAVY_USER] > 0).sum() == heavy == 290        # four chunks and a part of a fifth
    assert an.FIXTURES["d100_alpha1"][3:5] == (1.0, 0.01) and an.FIXTURES["d64"][1] == 257


def test_d1_closed_form():
    case = an.make_case("d1")
    R, Y, alpha, reg = case["R"], case["Y0"].astype(np.float64), case["alpha"], case["reg"]
    X = an.half_sweep(R, Y, alpha, reg)
    y = Y[:, 0]
    for u in range(case["U"]):
        want = ((1 + alpha * R[u]) * (R[u] > 0) * y).sum() / ((y * y).sum() + (alpha * R[u] * y * y).sum() + reg)
        assert X[u, 0] == pytest.approx(want, rel=1e-13, abs=1e-300)
    assert X[an.EMPTY_USER, 0] == 0.0


def test_sparse_loss_equals_dense_loss_and_never_rises_in_fp64():
    for name in an.FIXTURES:
        case = an.make_case(name)
        R, alpha, reg = case["R"], case["alpha"], case["reg"]
        X, Y = case["X0"].astype(np.float64), case["Y0"].astype(np.float64)
        last = an.dense_loss(R, X, Y, alpha, reg)
        assert an.sparse_loss(R, X, Y, alpha, reg) == pytest.approx(last, rel=1e-9)
        for _ in range(3):
            for side, _, _, new in an.both_half_sweeps(case, X, Y, np.float64):
                X, Y = (new, Y) if side == "users" else (X, new)
            now = an.dense_loss(R, X, Y, alpha, reg)
            assert an.sparse_loss(R, X, Y, alpha, reg) == pytest.approx(now, rel=1e-9), name
            assert now <= last, (name, now, last)
            last = now


def test_loss_falls_after_each_half_sweep_in_fp64():
    case = an.make_case("d17")
    R, alpha, reg = case["R"], case["alpha"], case["reg"]
    X, Y = case["X0"].astype(np.float64), case["Y0"].astype(np.float64)
    last = an.dense_loss(R, X, Y, alpha, reg)
    for _ in range(3):
        X = an.half_sweep(R, Y, alpha, reg)
        mid = an.dense_loss(R, X, Y, alpha, reg)
        Y = an.half_sweep(R.T, X, alpha, reg)
        now = an.dense_loss(R, X, Y, alpha, reg)
        assert now <= mid <= last
        last = now


def test_fixtures_carry_the_bound(trajectory):
    """A condition on the fixtures, not a measurement: the fp32 yardstick's own forward error stays within 1e-4 at every
    half-sweep of three epochs (measured 6.5e-8 .. 4.3e-5; its backward error rho 3.4e-8 .. 1.3e-7).  It needs both
    sides to have at least 2 D rows: a rank-deficient Gram matrix puts the yardstick itself 10 .. 40 % off."""
    case, steps = trajectory
    assert len(steps) == 6
    for k, s in enumerate(steps):
        e32 = an.forward_error(s["x32"], s["x64"])
        rho = an.row_residuals(s["R"], s["other"], case["alpha"], case["reg"], s["x32"]).max()
        print(f"{case['name']} half-sweep {k} ({s['side']}): e32 {e32:.2e} rho32 {rho:.2e}")
        assert e32 <= an.E32_BOUND, (case["name"], k, e32)
        assert rho <= 1e-6, (case["name"], k, rho)
        empty = an.EMPTY_USER if s["side"] == "users" else an.EMPTY_ITEM
        assert not s["x64"][empty].any() and not s["x32"][empty].any()


@pytest.mark.parametrize("defect", an.DEFECTS)
def test_each_defect_lands_outside_the_bound(defect):
    """The first user half-sweep from the start tables, on every fixture: at least 10 x the bound away from the truth
    (measured 1.2e-2 .. 1.5), and its residual against the true normal equation is visible too."""
    for name in an.FIXTURES:
        case = an.make_case(name)
        R, Y, alpha, reg = case["R"], case["Y0"], case["alpha"], case["reg"]
        x64 = an.half_sweep(R, Y, alpha, reg, np.float64)
        wrong = an.half_sweep(R, Y, alpha, reg, np.float64, defect)
        err = an.forward_error(wrong, x64)
        assert err >= 10 * an.E32_BOUND, (name, defect, err)
        assert an.row_residuals(R, Y, alpha, reg, wrong).max() >= 1e-5, (name, defect)
    with pytest.raises(AssertionError):
        an.half_sweep(R, Y, alpha, reg, np.float64, "no such defect")
