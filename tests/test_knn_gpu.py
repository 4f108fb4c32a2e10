"""ItemKNN / UserKNN on the GPU (csrc/knn.hip) against the numpy restatement (tests/knn_numpy.py) on every user, and
against the vectors captured from the reference (tests/golden/knn_*.npz) on the users whose neighbours the reference
determines (``untied``).

Every case runs at both accumulator forms: ``lds_cap = 0`` (chosen by the library: LDS at these sizes) and
``lds_cap = 1`` (its minimum: the block's slice of the workspace, cleared through the touched list).

Exact: ``item_sim_matrix``, ItemKNN ``predict``, ``neighbours()`` ids and sim bits, UserKNN's ``-inf`` pattern, ItemKNN's
recommended ids and scores.  Toleranced: UserKNN ``predict`` within ``k * 2^-52 * score`` (at most k non-negative doubles
summed, possibly in another order); UserKNN's recommended scores within one float32 ulp of the rounded restatement
score (the float64 discrepancy is far below half a float32 ulp, so a rounding moves by at most one), and no left-out
item's rounded score exceeds the last returned one by more than that ulp."""
import functools
import os

import numpy as np
import pytest
import torch

import knn_numpy as kn

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDENS = ("knn_k3", "knn_k5", "knn_k8", "knn_kbig")
FORMS = (0, 1)          # lds_cap: library's choice (LDS here), forced workspace


def _frame(rng, U, I, density, big_rows=(), empty_user=None, empty_item=None, max_mult=1):
    m = rng.random((U, I)) < density
    for u, n in big_rows:
        m[u, :n] = True
    if empty_user is not None:
        m[empty_user] = False
    if empty_item is not None:
        m[:, empty_item] = False
    u, i = np.nonzero(m)
    reps = rng.integers(1, max_mult + 1, len(u))
    u, i = np.repeat(u, reps), np.repeat(i, reps)
    perm = rng.permutation(len(u))
    return u[perm].astype(np.int64), i[perm].astype(np.int64)


# name -> (n_users, n_items, neighbourhood_size, frame): each the smallest shape that reaches the code it is named for
def _edge_frame(name):
    rng = np.random.default_rng({"tile_edge": 1, "big_rows": 2, "k1": 3, "clamp5": 4, "many_items": 5}[name])
    if name == "tile_edge":       # a catalogue one wider than the 256-column tile of the block; the last column is in use
        u, i = _frame(rng, 9, 257, 0.1, empty_user=6, empty_item=253)
        return 9, 257, 3, np.concatenate([u, [0, 3]]), np.concatenate([i, [256, 256]])
    if name == "big_rows":        # k = 128 of 130 users; users 0 and 1 (a query user and a neighbour) own 260 > 256 items;
        return (130, 300, 128) + _frame(rng, 130, 300, 0.04, big_rows=((0, 260), (1, 260)), empty_user=5,
                                        empty_item=299, max_mult=3)           # multiplicities up to 3
    if name == "k1":
        return (20, 15, 1) + _frame(rng, 20, 15, 0.2, empty_user=2, max_mult=2)
    if name == "clamp5":          # neighbourhood_size 8 clamped to 5 users
        return (5, 7, 8) + _frame(rng, 5, 7, 0.4)
    if name == "many_items":      # more rows of S than the launch has blocks (1024): a block owns several rows in turn
        return (7, 1030, 3) + _frame(rng, 7, 1030, 0.03, max_mult=2)
    raise KeyError(name)


EDGES = ("tile_edge", "big_rows", "k1", "clamp5", "many_items")


@functools.lru_cache(maxsize=None)
def case(name):
    """(U, I, k, users, items, B, S, item_rows, nb_ids, nb_sims, user_rows, golden | None): the reference values, computed
    once and shared (never modified: the arrays are read-only)."""
    golden = None
    if name in GOLDENS:
        golden = np.load(os.path.join(GOLDEN, name + ".npz"))
        U, I, k = (int(x) for x in golden["meta"][:3])
        users, items = golden["users"], golden["items"]
    else:
        U, I, k, users, items = _edge_frame(name)
    B = kn.dense_matrix(users, items, U, I)
    S = kn.item_similarity(B)
    item_rows = np.stack([kn.item_score_row(B, S, u) for u in range(U)])
    nb = [kn.neighbours(B, u, k) for u in range(U)]
    nb_ids, nb_sims = np.stack([a for a, _ in nb]), np.stack([b for _, b in nb])
    user_rows = np.stack([kn.user_score_row(B, u, k) for u in range(U)])
    for a in (B, S, item_rows, nb_ids, nb_sims, user_rows):
        a.setflags(write=False)
    return U, I, k, users, items, B, S, item_rows, nb_ids, nb_sims, user_rows, golden


def make(cls_name, name, lds_cap):
    import beta_recsys_amd as hp

    U, I, k, users, items = case(name)[:5]
    model = getattr(hp, cls_name)(dict(n_users=U, n_items=I, neighbourhood_size=k, device_str="cuda:0", lds_cap=lds_cap))
    model.prepare_model((users, items))
    return model


def all_pairs(U, I):
    return np.repeat(np.arange(U), I), np.tile(np.arange(I), U)


def test_edge_shapes_reach_what_they_are_named_for():
    U, I, k, users, items, B = case("big_rows")[:6]
    assert (B[0] > 0).sum() > 256 and (B[1] > 0).sum() > 256 and B.max() == 3 and not B[5].any() and not B[:, 299].any()
    assert (U, k) == (130, 128) and 1 in case("big_rows")[8][0]          # user 1 is a neighbour of user 0
    U, I, k, users, items, B = case("tile_edge")[:6]
    assert I == 257 and B[:, 256].any() and not B[6].any()
    assert case("k1")[2] == 1 and case("clamp5")[:3] == (5, 7, 8) and case("clamp5")[8].shape == (5, 5)
    for name in GOLDENS:
        B = case(name)[5]
        assert B.max() == 2 and (~B.any(axis=1)).any()


@pytest.mark.parametrize("lds_cap", FORMS)
@pytest.mark.parametrize("name", GOLDENS + EDGES)
def test_itemknn_matrix_and_predict_are_bit_equal(name, lds_cap):
    U, I, k, users, items, B, S, item_rows, _, _, _, golden = case(name)
    model = make("ItemKNN", name, lds_cap)
    got = model.item_sim_matrix.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (I, I)
    assert got.tobytes() == S.tobytes(), f"S differs in {(got != S).sum()} entries, max {np.abs(got - S).max()}"
    if golden is not None:
        assert got.tobytes() == golden["S"].tobytes()
    pu, pi = all_pairs(U, I)
    perm = np.random.default_rng(0).permutation(len(pu))               # pairs in no order, users repeated
    pred = model.predict(pu[perm], pi[perm])
    assert pred.dtype == torch.float32
    rows = np.empty((U, I), dtype=np.float32)
    rows[pu[perm], pi[perm]] = pred.cpu().numpy()
    assert rows.tobytes() == item_rows.tobytes()
    if golden is not None:
        valid = golden["item_rows_valid"]
        assert rows[valid].tobytes() == golden["item_rows"][valid].tobytes()
    # two runs give identical bits
    assert torch.equal(model.generate_item_sim_matrix(), model.item_sim_matrix)
    assert torch.equal(model.predict(pu[perm], pi[perm]), pred)


@pytest.mark.parametrize("lds_cap", FORMS)
@pytest.mark.parametrize("name", GOLDENS + EDGES)
def test_userknn_neighbours_and_predict(name, lds_cap):
    U, I, k, users, items, B, _, _, nb_ids, nb_sims, user_rows, golden = case(name)
    k_eff = min(k, U)
    model = make("UserKNN", name, lds_cap)
    query = np.concatenate([np.arange(U), [0, U - 1, 0]])               # a query list with repeated users
    ids, sims = model.neighbours(query)
    assert ids.dtype == torch.int64 and sims.dtype == torch.float64 and tuple(ids.shape) == (len(query), k_eff)
    ids, sims = ids.cpu().numpy(), sims.cpu().numpy()
    assert np.array_equal(ids, nb_ids[query])
    assert sims.tobytes() == nb_sims[query].tobytes()
    pu, pi = all_pairs(U, I)
    pred = model.predict(pu, pi)
    assert pred.dtype == torch.float64
    rows = pred.cpu().numpy().reshape(U, I)
    fin = np.isfinite(user_rows)
    assert np.array_equal(np.isfinite(rows), fin) and (rows[~fin] == -np.inf).all()
    bound = k_eff * 2.0 ** -52 * user_rows[fin]
    err = np.abs(rows[fin] - user_rows[fin])
    print(f"{name} lds_cap={lds_cap}: UserKNN predict max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}, "
          f"bit-equal {rows.tobytes() == user_rows.tobytes()}")
    assert np.all(err <= bound)
    if golden is not None:
        un = golden["untied"]
        ref = golden["user_rows"][un]
        gfin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(rows[un]), gfin)
        assert np.all(np.abs(rows[un][gfin] - ref[gfin]) <= k_eff * 2.0 ** -52 * ref[gfin])
        for u in np.nonzero(un)[0]:
            ref_ids, ref_sims = golden["nb_ids"][u], golden["nb_sims"][u]
            assert set(ids[u][sims[u] > 0]) == set(ref_ids[ref_sims > 0]), u
            assert np.array_equal(np.sort(sims[u]), np.sort(ref_sims)), u
    ids2, sims2 = model.neighbours(query)
    assert np.array_equal(ids2.cpu().numpy(), ids) and sims2.cpu().numpy().tobytes() == sims.tobytes()
    assert model.predict(pu, pi).cpu().numpy().tobytes() == pred.cpu().numpy().tobytes()


def check_lists(items, scores, K, seen_rows, ref_rows32, exact):
    """recommend()'s rules on every list; ``ref_rows32``: the restatement's score rows rounded to float32."""
    for q, (got_i, got_s) in enumerate(zip(items, scores)):
        seen, ref = seen_rows[q], ref_rows32[q]
        want_i, want_s = kn.topk_of_row(ref, seen, K)
        n = int((got_i >= 0).sum())
        assert n == int((want_i >= 0).sum()), q
        assert (got_i[n:] == -1).all() and (got_s[n:] == -np.inf).all(), q                     # the tail
        assert len(set(got_i[:n])) == n and not set(got_i[:n]) & set(seen), q                  # no repeat, nothing seen
        assert np.isfinite(got_s[:n]).all(), q
        order = np.lexsort((got_i[:n], -(got_s[:n] + np.float32(0))))
        assert np.array_equal(order, np.arange(n)), q                                          # score desc, id asc
        if exact:
            assert np.array_equal(got_i, want_i) and got_s.tobytes() == (want_s + np.float32(0)).tobytes(), q
            continue
        ulp = np.spacing(np.abs(ref[got_i[:n]]).astype(np.float32))
        assert np.all(np.abs(got_s[:n] - ref[got_i[:n]]) <= ulp), q
        if n:
            left = np.ones(len(ref), dtype=bool)
            left[got_i[:n]] = False
            left[np.asarray(list(seen), dtype=np.int64)] = False
            left &= np.isfinite(ref)
            if left.any():
                last = got_s[n - 1]
                assert ref[left].max() <= last + np.spacing(np.abs(last)), q


@pytest.mark.parametrize("lds_cap", FORMS)
@pytest.mark.parametrize("name", ("knn_k5", "knn_kbig", "tile_edge", "big_rows"))
@pytest.mark.parametrize("cls_name", ("ItemKNN", "UserKNN"))
def test_recommend_follows_the_rules(cls_name, name, lds_cap):
    import beta_recsys_amd as hp

    U, I, k, users, items, B, _, item_rows, _, _, user_rows, _ = case(name)
    model = make(cls_name, name, lds_cap)
    ref32 = item_rows if cls_name == "ItemKNN" else user_rows.astype(np.float32)
    query = np.concatenate([np.arange(U), [1, 1]])
    own = [set(np.nonzero(B[u])[0]) for u in query]
    for K, seen, seen_rows in ((1, None, [set()] * len(query)), (10, model.seen_csr(), own),
                               (min(I, 128), (users, items), own)):
        got_i, got_s = model.recommend(query, K, seen)
        assert got_i.dtype == torch.int64 and got_s.dtype == torch.float32 and tuple(got_i.shape) == (len(query), K)
        check_lists(got_i.cpu().numpy(), got_s.cpu().numpy(), K, seen_rows, ref32[query], exact=cls_name == "ItemKNN")
        again_i, again_s = hp.recommend(model, query, K, seen)                                # the package-level entry
        assert torch.equal(again_i, got_i) and torch.equal(again_s, got_s)


@pytest.mark.parametrize("lds_cap", FORMS)
@pytest.mark.parametrize("name", ("knn_k5", "big_rows"))
@pytest.mark.parametrize("cls_name", ("ItemKNN", "UserKNN"))
def test_more_queries_than_blocks(cls_name, name, lds_cap):
    """A launch has at most 1024 blocks; with 1100 queries a block serves a second user with the accumulator the first
    one left behind (swept in the LDS form, cleared through the touched list in the workspace form)."""
    U, I, k, users, items, B, _, item_rows, nb_ids, nb_sims, user_rows, _ = case(name)
    model = make(cls_name, name, lds_cap)
    ref32 = item_rows if cls_name == "ItemKNN" else user_rows.astype(np.float32)
    query = np.random.default_rng(7).integers(0, U, 1100)
    own = [set(np.nonzero(B[u])[0]) for u in query]
    got_i, got_s = model.recommend(query, 10, model.seen_csr())
    check_lists(got_i.cpu().numpy(), got_s.cpu().numpy(), 10, own, ref32[query], exact=cls_name == "ItemKNN")
    first_i, first_s = model.recommend(np.arange(U), 10, model.seen_csr())
    assert torch.equal(got_i, first_i[query]) and torch.equal(got_s, first_s[query])
    if cls_name == "UserKNN":
        ids, sims = model.neighbours(query)
        assert np.array_equal(ids.cpu().numpy(), nb_ids[query]) and sims.cpu().numpy().tobytes() == nb_sims[query].tobytes()


@pytest.mark.parametrize("over", (0, 1))
def test_userknn_on_both_sides_of_the_librarys_own_cap(over):
    """``lds_cap = 0`` at ``n_users`` = HIPREC_KNN_LDS_CAP (the largest accumulator the library keeps in LDS) and one
    more (the first it places in the workspace): the threshold between the two forms as the library draws it."""
    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib, knn

    U, I, k = knn.LDS_CAP + over, 6, 5
    rng = np.random.default_rng(11 + over)
    users = np.concatenate([np.arange(U), rng.integers(0, U, U // 2)])
    items = rng.integers(0, I, len(users))
    B = kn.dense_matrix(users, items, U, I)
    need = _lib.load().hiprec_knn_workspace_bytes(knn.OP_USER_SCORES, U, I, 3, 0)
    assert (need > 0) == bool(over)
    model = hp.UserKNN(dict(n_users=U, n_items=I, neighbourhood_size=k, device_str="cuda:0"))
    model.prepare_model((users, items))
    query = np.array([0, 4321, U - 1])
    ids, sims = model.neighbours(query)
    pred = model.predict(np.repeat(query, I), np.tile(np.arange(I), len(query))).cpu().numpy().reshape(len(query), I)
    for n, u in enumerate(query):
        want_ids, want_sims = kn.neighbours(B, u, k)
        assert np.array_equal(ids[n].cpu().numpy(), want_ids) and sims[n].cpu().numpy().tobytes() == want_sims.tobytes()
        want = kn.user_score_row(B, u, k)
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(pred[n]), fin)
        assert np.all(np.abs(pred[n][fin] - want[fin]) <= k * 2.0 ** -52 * want[fin])


@pytest.mark.parametrize("lds_cap", FORMS)
@pytest.mark.parametrize("cls_name", ("ItemKNN", "UserKNN"))
def test_out_of_range_query_raises_with_the_other_rows_complete(cls_name, lds_cap):
    U, I = case("knn_k5")[:2]
    model = make(cls_name, "knn_k5", lds_cap)
    good_i, good_s = model.recommend([3, 0, 7], 5, model.seen_csr())
    for bad in (U, -1):
        with pytest.raises(IndexError) as exc:
            model.recommend([3, bad, 0, 7], 5, model.seen_csr())
        part_i, part_s = exc.value.partial
        assert torch.equal(part_i[[0, 2, 3]], good_i) and torch.equal(part_s[[0, 2, 3]], good_s)
        assert (part_i[1] == -1).all() and (part_s[1] == -float("inf")).all()
    with pytest.raises(IndexError):
        model.predict([0, U], [1, 1])
    with pytest.raises(IndexError):
        model.predict([0, 1], [1, I])
    # the status word is clear again
    again_i, _ = model.recommend([3, 0, 7], 5, model.seen_csr())
    assert torch.equal(again_i, good_i)
    if cls_name == "UserKNN":
        with pytest.raises(IndexError) as exc:
            model.neighbours([2, U])
        ids, sims = exc.value.partial
        assert np.array_equal(ids[0].cpu().numpy(), case("knn_k5")[8][2]) and (ids[1] == -1).all()


@pytest.mark.parametrize("cls_name", ("ItemKNNEngine", "UserKNNEngine"))
def test_engines_and_evaluate_full_go_through_the_models_hook(cls_name):
    import beta_recsys_amd as hp

    U, I, k, users, items, B, _, item_rows, _, _, user_rows, _ = case("knn_k8")
    eng = getattr(hp, cls_name)({"model": dict(n_users=U, n_items=I, neighbourhood_size=k, device_str="cuda:0")})
    eng.model.prepare_model((users, items))
    assert eng.train_single_batch(None) == 0
    ref32 = item_rows if cls_name == "ItemKNNEngine" else user_rows.astype(np.float32)
    rng = np.random.default_rng(9)
    t_users = np.repeat(np.arange(U), 2)
    t_items = rng.integers(0, I, len(t_users))
    got = hp.evaluate_full(eng, {"col_user": t_users, "col_item": t_items}, {"col_user": users, "col_item": items},
                           metrics=("precision", "recall"), k_li=[5])
    lists, _ = eng.recommend(np.arange(U), 5, eng.model.seen_csr())
    assert torch.equal(lists, hp.recommend(eng, np.arange(U), 5, (users, items))[0])
    prec, rec, n = 0.0, 0.0, 0
    for u in range(U):
        truth = set(t_items[t_users == u]) - set(np.nonzero(B[u])[0])
        if not truth:
            continue
        want, _ = kn.topk_of_row(ref32[u], set(np.nonzero(B[u])[0]), 5)
        if cls_name == "ItemKNNEngine":
            assert np.array_equal(lists[u].cpu().numpy(), want)
        hits = len(truth & set(lists[u].cpu().numpy().tolist()))
        prec, rec, n = prec + hits / 5, rec + hits / len(truth), n + 1
    assert got["precision@5"] == pytest.approx(prec / n, rel=1e-12) and got["recall@5"] == pytest.approx(rec / n, rel=1e-12)
