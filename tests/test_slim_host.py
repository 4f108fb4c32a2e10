"""Host-side checks of SLIM that need no GPU: the symbols are declared, exported and bound; the workspace and the argument
validation of both entry points; the config errors; a CPU model refuses to compute; the evidence group; and the numpy
restatement (tests/slim_numpy.py) against itself -- the n = 1 and n = 2 closed forms, W64 at its KKT point, the screening
rule bit for bit, fixtures that reach the seams they are named for, seven named defects that land outside the bound, and
the support test's cap."""
import contextlib
import io
import os
import re
import sys

import numpy as np
import pytest

import slim_numpy as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hiprec_slim_workspace_bytes", "hiprec_slim_fit")
NONE = (1 << 64) - 1           # hiprec_slim_workspace_bytes for a bad shape
CFG = dict(n_users=10, n_items=20, device_str="cpu")

# a defect that cannot show on a fixture by construction: without l1 there is none to drop; and where l1 = 1000 exceeds
# every count (three times over, so the multiplicities too) W = 0 whatever the denominator, the order, the diagonal or
# the multiplicity, and q never moves.  Dropping the clamp shows there as well: the unclamped step is negative.
VACUOUS = {
    "no_l1": ("l1_zero",),
    "no_l2_in_denominator": ("all_zero",),
    "stale_q": ("all_zero",),
    "diagonal_free": ("all_zero",),
    "descending_one_sweep": ("all_zero",),
    "counts_not_binary": ("all_zero",),
    "no_clamp": (),
}


def header_constants():
    header = open(os.path.join(ROOT, "include", "hiprec.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (HIPREC_(?:SLIM|EASE)_\w+) (\d+)", header)}


def test_symbols_are_declared_exported_and_bound():
    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib, ease, knn, slim

    header = open(os.path.join(ROOT, "include", "hiprec.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in header, f"{name} is not declared in include/hiprec.h"
        assert name in _lib.SIGNATURES, f"_lib.py has no prototype for {name}"
        assert hasattr(lib, name), f"libhiprec.so does not export {name}"
    k = header_constants()
    assert k["HIPREC_SLIM_CHUNK"] == slim.CHUNK == sn.CHUNK == 64
    assert k["HIPREC_SLIM_LDS_CAP"] == slim.LDS_CAP and 2 * 4 * slim.LDS_CAP <= 64 << 10
    assert k["HIPREC_SLIM_MAX_SWEEPS"] == slim.MAX_SWEEPS
    assert k["HIPREC_EASE_MAX_ITEMS"] == slim.MAX_ITEMS and k["HIPREC_EASE_MAX_USERS"] == slim.MAX_USERS
    assert "#define HIPREC_STATUS_NOT_FINITE 512u" in header and _lib.STATUS_NOT_FINITE == 512
    assert hp.SLIM is slim.SLIM and hp.SLIMEngine is slim.SLIMEngine
    assert issubclass(hp.SLIM, knn._KNNBase) and issubclass(hp.SLIMEngine, knn._KNNEngine)
    # the shared base: EASE and SLIM score, rank and checkpoint through the same code
    for method in ("recommend_for", "_score_call", "state_dict", "load_state_dict"):
        assert getattr(hp.SLIM, method) is getattr(hp.EASE, method) is getattr(ease._ItemWeightsBase, method), method
    for method in ("prepare_model", "gram", "fit_from_gram", "predict", "topk_items", "recommend", "seen_csr"):
        assert callable(getattr(hp.SLIM, method)), method
    for method in ("train_an_epoch", "train_single_batch", "recommend", "save_checkpoint", "resume_checkpoint"):
        assert callable(getattr(hp.SLIMEngine, method)), method


def test_evidence_group_exists():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge

    assert ge.EVIDENCE_GROUPS["slim"] == ["common.hpp", "util.hip", "knn.hip", "ease.hip", "slim.hip"]
    assert ge.evidence_group("slim") == "slim" and ge.evidence_group("slim_fit") == "slim"
    assert ge.evidence_group("ease") == "ease" and ge.evidence_group("adam") == "mf"
    assert os.path.exists(os.path.join(ge.CSRC, "slim.hip"))


def test_workspace_bytes_follow_the_shape():
    from beta_recsys_amd import _lib

    ws = _lib.load().hiprec_slim_workspace_bytes
    cap = header_constants()["HIPREC_SLIM_LDS_CAP"]
    # the diagonal (n floats, rounded up to four); above lds_cap min(n, 1024) slices of 2 n floats behind it
    assert ws(1, 0) == 16 and ws(4, 0) == 16 and ws(5, 0) == 32 and ws(3706, 0) == 3708 * 4
    assert ws(cap, 0) == cap * 4 and ws(cap, cap + 5) == cap * 4
    assert ws(261, 256) == (264 + 261 * 2 * 261) * 4 and ws(261, 261) == 264 * 4
    assert ws(20, 1) == (20 + 20 * 2 * 20) * 4
    assert ws(cap + 1, 0) == ((cap + 4) + 1024 * 2 * (cap + 1)) * 4
    for bad in ((0, 0), (-1, 0), (5, -1), (header_constants()["HIPREC_EASE_MAX_ITEMS"] + 1, 0)):
        assert ws(*bad) == NONE, bad


def test_entry_point_validates_before_touching_the_gpu():
    """(the non-NULL pointers are never dereferenced: validation fails first)"""
    from beta_recsys_amd import _lib

    lib = _lib.load()
    P = 64

    def fit(A=P, n=20, l1=1.0, positive=1, tol=1e-5, max_sweeps=10, W=2 * P, sweeps=P, lds_cap=0, work=P,
            work_bytes=1 << 20, stats=P):
        return lib.hiprec_slim_fit(A, n, l1, positive, tol, max_sweeps, W, sweeps, lds_cap, work, work_bytes, stats, None)

    for bad in (dict(n=0), dict(n=-1), dict(n=(1 << 20) + 1), dict(lds_cap=-1)):
        assert fit(**bad) == -1 and b"bad sizes" in lib.hiprec_last_error(), bad
    for bad_l1 in (-1.0, float("nan"), float("inf")):
        assert fit(l1=bad_l1) == -1 and b"l1" in lib.hiprec_last_error(), bad_l1
    for bad_tol in (-1e-9, float("nan"), float("inf")):
        assert fit(tol=bad_tol) == -1 and b"tol" in lib.hiprec_last_error(), bad_tol
    for bad_sweeps in (0, -3, 1000001):
        assert fit(max_sweeps=bad_sweeps) == -1 and b"max_sweeps" in lib.hiprec_last_error(), bad_sweeps
    for bad_mode in (2, -1):
        assert fit(positive=bad_mode) == -1 and b"positive_only" in lib.hiprec_last_error(), bad_mode
    assert fit(stats=None) == -1 and b"stats" in lib.hiprec_last_error()
    for null in ("A", "W", "sweeps"):
        assert fit(**{null: None}) == -1 and b"NULL" in lib.hiprec_last_error(), null
    assert fit(W=P) == -1 and b"must not be A" in lib.hiprec_last_error()
    assert fit(work=None) == -1 and b"workspace" in lib.hiprec_last_error()
    assert fit(work_bytes=20 * 4 - 1) == -1 and b"workspace" in lib.hiprec_last_error()
    assert fit(lds_cap=19, work_bytes=(20 + 20 * 2 * 20) * 4 - 1) == -1 and b"workspace" in lib.hiprec_last_error()


def test_config_errors_and_the_cpu_refusal():
    import torch

    import beta_recsys_amd as hp

    nan, inf = float("nan"), float("inf")
    for bad, match in ((dict(l2_reg=0.0), "l2_reg"), (dict(l2_reg=-1.0), "l2_reg"), (dict(l2_reg=nan), "l2_reg"),
                       (dict(l2_reg=inf), "l2_reg"), (dict(l1_reg=-0.5), "l1_reg"), (dict(l1_reg=nan), "l1_reg"),
                       (dict(l1_reg=inf), "l1_reg"), (dict(tol=-1e-9), "tol"), (dict(tol=nan), "tol"),
                       (dict(tol=inf), "tol"), (dict(max_sweeps=0), "max_sweeps"), (dict(max_sweeps=-2), "max_sweeps"),
                       (dict(max_sweeps=1000001), "max_sweeps"), (dict(n_users=0), "n_users"),
                       (dict(n_items=0), "n_users"), (dict(n_users=1 << 24), "n_users"),
                       (dict(max_sim_bytes=2 * 20 * 20 * 4 - 1), "max_sim_bytes")):
        with pytest.raises(ValueError, match=match):
            hp.SLIM(dict(CFG, **bad))
    model = hp.SLIM(dict(CFG, max_sim_bytes=2 * 20 * 20 * 4))
    assert (model.l1_reg, model.l2_reg, model.positive_only, model.tol, model.max_sweeps) == (1.0, 1.0, True, 1e-5, 100)
    assert model.item_weights is None and model.sweeps is None and model.n_unconverged is None and model.nnz is None
    assert hp.SLIM(dict(CFG, l1_reg=0, positive_only=False)).positive_only is False
    assert hp.SLIM(CFG).max_sim_bytes == 4 << 30
    assert model.state_dict() == {} and model.forward(None) == 0.0
    # no CPU fallback anywhere, and nothing before prepare_model
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.prepare_model((np.array([0, 1]), np.array([2, 3])))
    assert model.item_weights is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.fit_from_gram(torch.eye(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.load_state_dict({"item_weights": torch.zeros(20, 20)})
    for call in (lambda: model.predict([0], [1]), lambda: model.recommend([0], 3), lambda: model.seen_csr(),
                 lambda: model.gram(), lambda: model.recommend_for([0, 1], [2], 3)):
        with pytest.raises(RuntimeError, match="prepare_model"):
            call()
    with contextlib.redirect_stdout(io.StringIO()) as out:
        eng = hp.SLIMEngine({"model": CFG})
        assert eng.train_single_batch(None) == 0
        eng.train_an_epoch(None, 7)
    assert isinstance(eng.model, hp.SLIM) and not hasattr(eng, "optimizer")
    assert out.getvalue() == "[Training Epoch 7] skipped\n"


# ---- the restatement against itself ------------------------------------------------------------------------------------

def test_n1_gives_zero_and_n2_matches_the_closed_form():
    for X in (np.zeros((5, 1)), np.ones((5, 1))):
        A, _ = sn.gram(X, 3.0)
        out = sn.coordinate_descent(A, 1.0, True, 0.0, 10)
        assert np.array_equal(out["W"], [[0.0]]) and out["sweeps"].tolist() == [1] and out["converged"].all()
    assert np.array_equal(sn.make_case("n1")["W64"], [[0.0]]) and np.array_equal(sn.make_case("n1")["W32"], [[0.0]])
    X = (sn.PAIR > 0).astype(np.float64)
    a, b, c = X[:, 0].sum(), (X[:, 0] * X[:, 1]).sum(), X[:, 1].sum()
    assert b >= 2 and a > b and c > b
    for l1, l2, positive in ((0.5, 1.0, True), (1.0, 2.5, True), (0.5, 1.0, False), (b + 1.0, 1.0, True)):
        A, G = sn.gram(X, l2)
        W = sn.exact_weights(A, G, l1, positive)
        # with w_j = 0 each column has one free coordinate: w = max(0, b - l1) / (A_kk)
        assert W[0, 0] == 0.0 and W[1, 1] == 0.0
        assert W[0, 1] == pytest.approx(max(0.0, b - l1) / (a + l2), rel=1e-14, abs=0.0)
        assert W[1, 0] == pytest.approx(max(0.0, b - l1) / (c + l2), rel=1e-14, abs=0.0)
    case = sn.make_case("n2")
    assert case["W64"][0, 1] > 0 and case["W64"][1, 0] > 0 and case["empty_item"] is None


def test_w64_sits_at_its_kkt_point_and_the_yardstick_near_it():
    """Measured: W64's violation 0 .. 8.2e-13; the yardstick's 0 .. 2.5e-4, between 0.05 and 0.11 of the derived term
    ``tol * max_k sum_l |A_kl|`` of the GPU test's backward bound; the yardstick's forward error 0 .. 1.7e-5 of scale."""
    for name in sn.FIXTURES:
        case = sn.make_case(name)
        k64 = sn.kkt_violation(case["A64"], case["G64"], case["W64"], case["l1"], case["positive"])
        k32 = sn.kkt_violation(case["A64"], case["G64"], case["W32"], case["l1"], case["positive"])
        derived = case["tol"] * np.abs(case["A64"]).sum(axis=1).max()
        print(f"{name}: kkt W64 {k64:.2e} W32 {k32:.2e} derived {derived:.2e} ratio {k32 / derived:.3f} "
              f"forward W32 {sn.forward_error(case['W32'], case['W64']):.2e}")
        assert k64 <= sn.KKT64, name
        assert k32 <= derived, name
        assert case["converged32"].all(), name
        assert np.isfinite(case["W64"]).all() and not np.diag(case["W64"]).any() and not np.diag(case["W32"]).any()


def test_the_screening_rule_never_changes_a_bit():
    """Positive mode: a coordinate with G_kj <= l1 never leaves zero, so skipping it changes nothing.  (Signed mode has
    no such rule: the argument is the rule's own switch there and does nothing.)"""
    for name in sn.FIXTURES:
        case = sn.make_case(name)
        out = sn.coordinate_descent(case["A32"], case["l1"], case["positive"], case["tol"], case["max_sweeps"],
                                    np.float32, screen=True)
        assert out["W"].tobytes() == case["W32"].tobytes(), name
        assert np.array_equal(out["sweeps"], case["sweeps32"]), name
        if case["positive"]:
            G = case["A32"] - np.float32(case["l2"]) * np.eye(case["I"], dtype=np.float32)
            assert not case["W32"][G <= case["l1"]].any(), name


def test_fixtures_reach_what_they_are_named_for():
    k = header_constants()
    chunk, cap = k["HIPREC_SLIM_CHUNK"], k["HIPREC_SLIM_LDS_CAP"]
    size = {name: sn.make_case(name)["I"] for name in sn.FIXTURES}
    assert size["n1"] == 1 and size["n2"] == 2
    assert (size["chunk_minus"], size["chunk"], size["chunk_plus"]) == (chunk - 1, chunk, chunk + 1)
    assert size["block_plus"] > sn.BLOCK and size["block_plus"] % sn.BLOCK != 0 and size["block_plus"] % chunk != 0
    n, cap_ws = size["ws_path"], sn.FIXTURES["ws_path"][6]
    assert 255 <= n <= 265 and 0 < cap_ws < n <= cap
    assert all(f[6] == 0 for name, f in sn.FIXTURES.items() if name != "ws_path")
    params = {(f[1], f[2], f[3]) for f in sn.FIXTURES.values()}
    assert {(1.0, 1.0, True), (0.5, 10.0, True), (0.0, 5.0, True), (1.0, 1.0, False)} <= params
    assert all(f[4] == 1e-6 for f in sn.FIXTURES.values())
    assert not sn.make_case("all_zero")["W64"].any() and sn.make_case("all_zero")["sweeps32"].max() == 1
    assert (sn.make_case("signed")["W64"] < 0).sum() >= 50
    for name in sn.FIXTURES:
        case = sn.make_case(name)
        R, U, I = case["R"], case["U"], case["I"]
        assert U <= 600 and case["users"].size == int(R.sum())
        got = np.zeros_like(R)
        np.add.at(got, (case["users"], case["items"]), 1)
        assert np.array_equal(got, R)
        assert not R[sn.EMPTY_USER].any() and (I == 1 or (R.sum(axis=1) == 0).sum() == 1)    # (n1: nobody has anything)
        if I > 2:
            e = case["empty_item"]
            assert not R[:, e].any() and (R.sum(axis=0) > 0).sum() == I - 1
            assert not case["W64"][e].any() and not case["W64"][:, e].any()
            assert not case["W32"][e].any() and not case["W32"][:, e].any()
        if I > 1:
            assert R.max() == 3, "multiplicities must be there for the binarisation to show"
        if I >= 15:
            pop = (R > 0).sum(axis=0)
            assert pop[:3].sum() > 2 * pop[-3:].sum(), "popularity-skewed columns"
            if name != "all_zero":
                assert case["sweeps32"].max() >= 8, "the fixed-sweeps test needs a fixture that takes more than 3"
        if case["positive"]:
            assert (case["W64"] >= 0).all() and (case["W32"] >= 0).all() and not np.signbit(case["W32"]).any()


@pytest.mark.parametrize("defect", sn.DEFECTS)
def test_each_defect_lands_outside_the_bound(defect):
    """At least 10 x the GPU test's forward bound away from the truth on every fixture of 15 items and more on which the
    defect can show at all (VACUOUS lists the others and why)."""
    checked = 0
    for name in sn.FIXTURES:
        case = sn.make_case(name)
        if case["I"] < 15 or name in VACUOUS[defect]:
            continue
        wrong = sn.defect_weights(case, defect)
        err = sn.forward_error(np.nan_to_num(wrong, nan=np.inf), case["W64"])
        ratio = err / sn.bound(case)
        print(f"{defect} on {name}: {err:.2e} of scale, {ratio:.1f} x the bound")
        assert ratio >= 10.0, (name, defect, err, sn.bound(case))
        checked += 1
    assert checked >= 8
    with pytest.raises(AssertionError):
        sn.coordinate_descent(case["A64"], 1.0, True, 0.0, 1, defect="no such defect")


def test_the_support_tests_cap_holds_for_the_restatement():
    """Indecisive entries are at most 5 % of the off-diagonal ones on every l1 >= 0.5 fixture (measured: none), and the
    yardstick gets no decisive entry wrong."""
    assert set(sn.SUPPORT) == {n for n, f in sn.FIXTURES.items() if f[1] >= 0.5} and "l1_zero" not in sn.SUPPORT
    for name in sn.SUPPORT:
        case = sn.make_case(name)
        dec, pos, zero = sn.decisive(case)
        off = case["I"] * (case["I"] - 1)
        share = (off - int(pos.sum()) - int(zero.sum())) / max(off, 1)
        print(f"{name}: dec {dec:.2e} decisive positive {int(pos.sum())} zero {int(zero.sum())} indecisive {share:.4f}")
        assert share <= 0.05, name
        assert (case["W32"][pos] != 0).all() and (np.sign(case["W32"][pos]) == np.sign(case["W64"][pos])).all()
        assert not case["W32"][zero].any() and not np.signbit(case["W32"][zero]).any()
