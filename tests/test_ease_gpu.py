"""EASE on the GPU (csrc/ease.hip) against the fp64 restatement tests/ease_numpy.py, on every fixture of that module.

* Gram: off the diagonal ``G`` is the integer co-occurrence matrix bit for bit, on it ``float32(count) + float32(reg)``
  (so ``G - reg I`` is the count matrix exactly for the integral ``reg`` of every fixture but the stiff one); symmetric;
  the LDS and the workspace accumulator give the same bits.
* Weights: the project's bounds as tests/test_als_gpu.py applies them -- forward error within 1e-5 of ``B``'s scale plus
  twice the fp32 yardstick's own error (``helpers.assert_as_accurate_as_reference``), backward error ``max |G P - I|``
  (fp64, on the GPU's own ``P``) at most 4 x the yardstick's.  Both are Cholesky factorisations followed by
  ``L^-1`` and ``L^-T L^-1``; the 4 is for the different summation and elimination order.
* Bits: two runs give identical bits (the grid is not configurable: every tile has one owner).
* Scores: ``predict`` within 1e-5 of scale of the fp64 ``X B`` of the GPU's own ``B``; ``recommend`` against an fp64
  ranking of that ``B`` wherever the ranking's gaps exceed the fp32 sum's error bound, ties to the lower id.
* Failure: a NaN or a negative pivot in a caller's matrix raises FloatingPointError (a status word, never a fault).
"""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import ease_numpy as en
from helpers import assert_as_accurate_as_reference

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24
SCORED = ("n2", "n17", "panel_plus", "ws_path")       # the fixtures whose scores are checked


def new_model(name, **extra):
    import beta_recsys_amd as hp

    case = en.make_case(name)
    cfg = dict(n_users=case["U"], n_items=case["I"], reg=case["reg"], device_str="cuda:0", lds_cap=case["lds_cap"],
               keep_inverse=True)
    cfg.update(extra)
    model = hp.EASE(cfg)
    model.prepare_model((case["users"], case["items"]))
    return model


@functools.lru_cache(maxsize=None)
def trained(name):
    """One prepared model per fixture, shared and never modified."""
    return new_model(name)


@functools.lru_cache(maxsize=None)
def gpu_weights(name):
    B = trained(name).item_weights.cpu().numpy()
    B.setflags(write=False)
    return B


@pytest.mark.parametrize("name", list(en.FIXTURES))
def test_gram_is_the_integer_cooccurrence_matrix(name, hip_device):
    case = en.make_case(name)
    model = trained(name)
    G = model.gram().cpu().numpy()
    Xi = (case["R"] > 0).astype(np.int64)
    counts = Xi.T @ Xi
    want = counts.astype(np.float32)
    want[np.diag_indices_from(want)] += np.float32(case["reg"])
    assert G.dtype == np.float32 and G.tobytes() == want.tobytes(), f"G differs in {(G != want).sum()} entries"
    assert np.array_equal(G, G.T)
    if float(case["reg"]).is_integer():
        assert np.array_equal(G - np.float32(case["reg"]) * np.eye(case["I"], dtype=np.float32), counts)
    assert np.array_equal(G, case["G32"])
    # the other accumulator form: forced into the workspace (lds_cap = 1), or back into LDS (0) for the ws fixture
    other = new_model(name, lds_cap=0 if case["lds_cap"] else 1)
    assert other.gram().cpu().numpy().tobytes() == G.tobytes()
    assert other.item_weights.cpu().numpy().tobytes() == gpu_weights(name).tobytes()


@pytest.mark.parametrize("name", list(en.FIXTURES))
def test_weights_are_as_accurate_as_the_fp32_yardstick(name, hip_device):
    """Measured on an MI355X: see DESIGN.md (EASE) for the ranges of both errors."""
    case = en.make_case(name)
    model = trained(name)
    B, P = gpu_weights(name), model.inverse.cpu().numpy()
    e = case["empty_item"]
    assert B.shape == (case["I"], case["I"]) and B.dtype == np.float32 and np.isfinite(B).all()
    assert not np.diag(B).any() and not np.signbit(np.diag(B)).any(), "the diagonal is exact +0"
    assert not B[e].any() and not B[:, e].any(), "an untouched item weighs nothing and receives nothing"
    assert np.array_equal(P, P.T), "the kept inverse is mirrored"
    fwd, fwd32 = en.forward_error(B, case["B64"]), en.forward_error(case["B32"], case["B64"])
    res, res32 = en.residual(case["G32"], P), en.residual(case["G32"], case["P32"])
    print(f"{name}: forward gpu {fwd:.3e} yardstick {fwd32:.3e}; backward gpu {res:.3e} yardstick {res32:.3e} "
          f"(ratio {res / res32:.2f})")
    assert_as_accurate_as_reference(got=B, ref=case["B32"], exact=case["B64"], what=f"{name} B")
    assert res <= 4 * res32, (name, res, res32)


@pytest.mark.parametrize("name", ("n17", "panel_plus", "two_panels_ragged", "ws_path", "stiff"))
def test_two_runs_give_identical_bits(name, hip_device):
    again = new_model(name)
    assert again.item_weights.cpu().numpy().tobytes() == gpu_weights(name).tobytes()
    assert torch.equal(again.inverse, trained(name).inverse)
    again.prepare_model((en.make_case(name)["users"], en.make_case(name)["items"]))       # and on the same object
    assert again.item_weights.cpu().numpy().tobytes() == gpu_weights(name).tobytes()


@pytest.mark.parametrize("name", SCORED)
def test_predict_matches_the_fp64_product(name, hip_device):
    case = en.make_case(name)
    model = trained(name)
    S = en.scores(case["R"], gpu_weights(name))
    rng = np.random.default_rng(11)
    users, items = rng.integers(0, case["U"], 300), rng.integers(0, case["I"], 300)
    users[:2] = en.EMPTY_USER
    got = model.predict(users, items).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (300,)
    scale = np.abs(S).max()
    assert np.abs(got.astype(np.float64) - S[users, items]).max() <= 1e-5 * scale + 1e-30
    assert not got[:2].any()
    with pytest.raises(IndexError):
        model.predict([0, case["U"]], [0, 0])
    with pytest.raises(IndexError):
        model.predict([0], [case["I"]])


def _check_ranking(got_items, got_scores, S, tol, seen, k):
    """Row by row: nothing seen, scores as the fp64 row says, best first with ties to the lower id, nothing better left
    out, and the fp64 ranking's own items wherever its gaps are clear of the fp32 sum's error."""
    n_clear = 0
    for u in range(S.shape[0]):
        row, t = S[u].copy(), tol[u]
        row[seen[u]] = -np.inf
        n_cand = int(np.isfinite(row).sum())
        items, sc = got_items[u], got_scores[u]
        m = min(k, n_cand)
        assert (items[m:] == -1).all() and np.isneginf(sc[m:]).all()
        assert len(set(items[:m].tolist())) == m and np.isfinite(row[items[:m]]).all(), "a seen item came back"
        assert (np.abs(sc[:m].astype(np.float64) - row[items[:m]]) <= t[items[:m]] + 1e-30).all()
        for a in range(m - 1):
            assert sc[a] > sc[a + 1] or (sc[a] == sc[a + 1] and items[a] < items[a + 1]), (u, a)
        left = np.ones(S.shape[1], dtype=bool)
        left[items[:m]] = False
        left &= np.isfinite(row)
        if m and left.any():
            assert (row[left] - t[left] <= float(sc[m - 1]) + t[items[m - 1]]).all(), "a better item was left out"
        order = np.lexsort((np.arange(S.shape[1]), -row))          # fp64 ranking, ties to the lower id
        top = order[:min(m + 1, n_cand)]
        gaps = row[top[:-1]] - row[top[1:]]
        clear = gaps > t[top[:-1]] + t[top[1:]]
        for a in range(m):                                         # a place whose neighbours are both clear of it
            if (a == 0 or clear[a - 1]) and (a >= len(gaps) or clear[a]):
                assert items[a] == top[a], (u, a)
                n_clear += 1
    return n_clear


@pytest.mark.parametrize("name", SCORED)
def test_recommend_never_returns_a_seen_item_and_follows_the_fp64_ranking(name, hip_device):
    case = en.make_case(name)
    model = trained(name)
    B = gpu_weights(name).astype(np.float64)
    X = case["R"] > 0
    S = X @ B
    # |fl(sum of m terms) - sum| <= (m - 1) eps sum |terms| to first order; m eps is the safe side
    tol = X.sum(axis=1, keepdims=True) * EPS32 * (X.astype(np.float64) @ np.abs(B)) * 1.01
    k = min(10, case["I"])
    items, scores = model.recommend(np.arange(case["U"]), k, seen=model.seen_csr())
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    assert items.shape == (case["U"], k) and items.dtype == np.int64 and scores.dtype == np.float32
    n_clear = _check_ranking(items, scores, S, tol, [np.nonzero(X[u])[0] for u in range(case["U"])], k)
    if case["I"] >= 15:
        assert n_clear >= case["U"], "the comparison with the fp64 ranking must bite somewhere"
    # the empty user: every score is +0, so the lowest ids in order
    assert items[en.EMPTY_USER].tolist() == list(range(k)) and not scores[en.EMPTY_USER].any()
    # and without a seen mask the user's own items may come back
    free_items, _ = model.recommend(np.arange(case["U"]), k)
    _check_ranking(free_items.cpu().numpy(), _.cpu().numpy(), S, tol, [np.zeros(0, dtype=np.int64)] * case["U"], k)


@pytest.mark.parametrize("name", SCORED)
def test_recommend_for_on_the_frames_own_lists_is_recommend(name, hip_device):
    """Bit for bit on every user with a list.  The user with nothing differs by design: ``recommend`` ranks a row of
    zeros (ItemKNN's kernel), ``recommend_for`` says there is nothing to score from."""
    case = en.make_case(name)
    model = trained(name)
    X = case["R"] > 0
    k = min(7, case["I"])
    want_items, want_scores = model.recommend(np.arange(case["U"]), k, seen=model.seen_csr())
    rng = np.random.default_rng(5)
    lists = [rng.permutation(np.repeat(np.nonzero(X[u])[0], 2)) for u in range(case["U"])]     # shuffled, listed twice
    ptr = np.concatenate([[0], np.cumsum([len(a) for a in lists])])
    idx = np.concatenate(lists).astype(np.int64)
    got_items, got_scores = model.recommend_for(ptr, idx, k)
    has = X.any(axis=1)
    assert torch.equal(got_items.cpu()[has], want_items.cpu()[has])
    assert got_scores.cpu().numpy()[has].tobytes() == want_scores.cpu().numpy()[has].tobytes()
    assert (got_items.cpu().numpy()[~has] == -1).all() and np.isneginf(got_scores.cpu().numpy()[~has]).all()
    assert (~has).sum() == 1
    free_items, free_scores = model.recommend_for(ptr, idx, k, exclude=False)
    base_items, base_scores = model.recommend(np.arange(case["U"]), k)
    assert torch.equal(free_items.cpu()[has], base_items.cpu()[has])
    assert torch.equal(free_scores.cpu()[has], base_scores.cpu()[has])


def test_recommend_for_edge_cases(hip_device):
    model = trained("n17")
    I = 17
    items, scores = model.recommend_for([0, 0, 0], [], 4)                      # two users, nothing listed
    assert items.shape == (2, 4) and (items.cpu().numpy() == -1).all() and np.isneginf(scores.cpu().numpy()).all()
    items, scores = model.recommend_for([0], [], 4)                            # no users
    assert items.shape == (0, 4) and scores.shape == (0, 4)
    items, scores = model.recommend_for([0, 0, 2, 2], [0, 5], 3)               # a list between two empty ones
    items = items.cpu().numpy()
    assert (items[0] == -1).all() and (items[2] == -1).all() and (items[1] >= 0).all()
    assert 0 not in items[1] and 5 not in items[1]
    everything, _ = model.recommend_for([0, I], np.arange(I), 5)               # everything listed: nothing is left
    assert (everything.cpu().numpy() == -1).all()
    for bad in ([I], [-1], [0, I]):
        with pytest.raises(IndexError):
            model.recommend_for([0, len(bad)], bad, 3)
    for bad_ptr in ([1, 2], [0, 3], [0, 2, 1, 2]):
        with pytest.raises(ValueError):
            model.recommend_for(bad_ptr, [0, 1], 3)
    with pytest.raises(ValueError):
        model.recommend_for([0, 1], [0], 129)
    after, _ = model.recommend_for([0, 2], [0, 5], 3)                          # a raised call leaves nothing behind
    assert np.array_equal(after.cpu().numpy()[0], items[1])


def test_evaluate_full_returns_metrics_in_range(hip_device):
    import beta_recsys_amd as hp

    case = en.make_case("panel_plus")
    model = trained("panel_plus")
    rng = np.random.default_rng(3)
    test_users = np.setdiff1d(np.arange(case["U"]), [en.EMPTY_USER])
    test_items = rng.integers(0, case["I"], test_users.size)
    metrics = hp.evaluate_full(model, {"col_user": test_users, "col_item": test_items},
                               {"col_user": case["users"], "col_item": case["items"]}, k_li=(5, 10))
    assert metrics and all(0.0 <= float(v) <= 1.0 for v in metrics.values()), metrics
    assert any(key.endswith("@10") for key in metrics)


def test_a_matrix_that_is_not_positive_definite_raises_and_leaves_the_model_usable(hip_device):
    import beta_recsys_amd as hp

    case = en.make_case("panel_plus")
    n = case["I"]
    model = hp.EASE(dict(n_users=case["U"], n_items=n, reg=case["reg"], device_str="cuda:0", keep_inverse=True))
    G = torch.from_numpy(case["G32"].copy())
    # the hook itself inverts: a good matrix first
    B, P = model.weights_from_gram(G)
    assert B.cpu().numpy().tobytes() == gpu_weights("panel_plus").tobytes()
    assert en.residual(case["G32"], P.cpu().numpy()) <= 4 * en.residual(case["G32"], case["P32"])
    for where in ((0, 0), (40, 7), (n - 1, n - 1), (n - 1, 2)):                # first panel, across, the ragged panel
        bad = G.clone()
        bad[where] = bad[where[::-1]] = float("nan")
        with pytest.raises(FloatingPointError, match="pivot"):
            model.weights_from_gram(bad)
    for j in (3, n - 1):                                                       # a negative pivot in either panel
        bad = G.clone()
        bad[j, j] = -1.0
        with pytest.raises(FloatingPointError, match="pivot"):
            model.weights_from_gram(bad)
    zero = G.clone()
    zero[case["empty_item"], case["empty_item"]] = 0.0                         # a zero pivot is not positive either
    with pytest.raises(FloatingPointError):
        model.weights_from_gram(zero)
    assert model.item_weights is None and model.inverse is None
    with pytest.raises(RuntimeError, match="prepare_model"):
        model.predict([0], [0])
    # a following prepare_model on good data works, to the bits of a fresh model
    model.prepare_model((case["users"], case["items"]))
    assert model.item_weights.cpu().numpy().tobytes() == gpu_weights("panel_plus").tobytes()
    # ... and prepare_model itself reports a failed pivot the same way (its Gram stage handed a planted matrix)
    real_gram = model.gram

    def planted(workspace=None):
        bad = real_gram(workspace)
        bad[20, 20] = float("nan")
        return bad

    model.gram = planted
    with pytest.raises(FloatingPointError, match="pivot"):
        model.prepare_model((case["users"], case["items"]))
    assert model.item_weights is None and model.inverse is None
    del model.gram
    model.prepare_model((case["users"], case["items"]))
    assert model.item_weights.cpu().numpy().tobytes() == gpu_weights("panel_plus").tobytes()


def test_engine_and_checkpoint_round_trip(hip_device, tmp_path):
    import beta_recsys_amd as hp

    case = en.make_case("n17")
    cfg = {"model": dict(n_users=case["U"], n_items=case["I"], reg=case["reg"], device_str="cuda:0")}
    with contextlib.redirect_stdout(io.StringIO()) as out:
        eng = hp.EASEEngine(cfg)
        assert eng.train_single_batch(None) == 0
        eng.train_an_epoch(None, 3)
    assert out.getvalue() == "[Training Epoch 3] skipped\n"
    eng.model.prepare_model((case["users"], case["items"]))
    assert eng.model.item_weights.cpu().numpy().tobytes() == gpu_weights("n17").tobytes()
    path = str(tmp_path / "ease.pt")
    eng.save_checkpoint(path)
    assert list(torch.load(path, map_location="cpu")) == ["item_weights"]
    with contextlib.redirect_stdout(io.StringIO()):
        other = hp.EASEEngine(cfg)
        other.resume_checkpoint(path)
    assert other.model.item_weights.cpu().numpy().tobytes() == gpu_weights("n17").tobytes()
    # the restored weights score lists without the frame ...
    ptr, idx = [0, 3], [0, 2, 5]
    a, b = other.model.recommend_for(ptr, idx, 5), eng.model.recommend_for(ptr, idx, 5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(RuntimeError, match="prepare_model"):
        other.model.recommend([0], 3)                       # ... the frame's users need the frame
    k = eng.recommend([0, 2], 4, seen=eng.model.seen_csr())
    assert k[0].shape == (2, 4)
