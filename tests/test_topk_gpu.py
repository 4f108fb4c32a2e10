"""GPU: full-catalogue top-K recommendation (csrc/topk.hip) -- the exact order on integer fixtures over every tiling /
masking / merging path, split invariance, the masking edge cases, float fixtures against fp64 scores, errors, the model
hooks against each model's own predict, and evaluate_full against evaluate on the explicit candidate frame."""
import contextlib
import io
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import topk_reference as tr

pytestmark = pytest.mark.gpu

TILE = 64          # items per wave iteration of topk_score_kernel (kTkTile)


def dev_t(a, dev, dtype=None):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).to(dev)


def run(U, I, alpha, bias, users, k, seen=None, splits=0, dev="cuda:0"):
    from beta_recsys_amd.recommend import topk_factors

    Ut = U if torch.is_tensor(U) else dev_t(U, dev)
    It = I if torch.is_tensor(I) else dev_t(I, dev)
    items, scores = topk_factors(Ut, It, alpha, dev_t(bias, dev), users, k, seen, splits)
    assert items.dtype == torch.int64 and scores.dtype == torch.float32 and items.shape == scores.shape == (len(users), k)
    return items.cpu().numpy(), scores.cpu().numpy()


# ---- exact order ------------------------------------------------------------------------------------------------------
N_QUERY, DIMS, KS, SPLITS = (1, 5, 33), (1, 8, 64, 100, 256), (1, 7, 128), (1, 3, 7)


@pytest.mark.parametrize("n_items", [1, 15, 17, 257, 1007])
def test_exact_order_on_integer_fixture(hip_device, n_items):
    """Every dot product is exact in fp32 in any summation order and ties are plentiful: ids AND scores must equal
    numpy.lexsort((id, -score)) over the unseen items, whatever the tiling, the width path (vector loads, the scalar
    path of an unaligned column slice, a partial last k chunk) and the number of item ranges."""
    n_users = 40
    for case, (n_query, dim, with_bias, alpha) in enumerate(itertools.product(N_QUERY, DIMS, (False, True), (1.0, 0.25))):
        rng = np.random.default_rng(1000 * n_items + case)
        U, I, bias = tr.integer_fixture(rng, n_users, n_items, dim, with_bias)
        users = rng.integers(0, n_users, n_query)
        ptr, pos = tr.random_seen(rng, n_users, n_items, max(1, n_items // 4))
        seen = None if case % 3 == 0 else (ptr, pos)
        want_i, want_s = tr.exact_topk(tr.scores64(U, I, alpha, bias, users), None if seen is None else
                                       tr.seen_rows(ptr, pos, users), max(KS))
        Ut, It = dev_t(U, hip_device), dev_t(I, hip_device)
        if dim == 8:     # once: a column slice of a wider buffer that starts off the 16-byte grid (ld 19 > D)
            wide_u = torch.full((n_users, 19), 7.0, device=hip_device)
            wide_i = torch.full((n_items, 19), -7.0, device=hip_device)
            wide_u[:, 3:11], wide_i[:, 5:13] = Ut, It
            Ut, It = wide_u[:, 3:11], wide_i[:, 5:13]
        for k, splits in itertools.product(KS, SPLITS):
            got_i, got_s = run(Ut, It, alpha, bias, users, k, seen, splits)
            what = (n_items, n_query, dim, with_bias, alpha, k, splits, seen is not None)
            assert np.array_equal(got_i, want_i[:, :k]), what
            assert np.array_equal(got_s, want_s[:, :k]), what


def float_fixture(seed, n_users, n_items, dim):
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((n_users, dim)).astype(np.float32)
    I = rng.standard_normal((n_items, dim)).astype(np.float32)
    bias = rng.standard_normal(n_items).astype(np.float32)
    ptr, pos = tr.random_seen(rng, n_users, n_items, 40)
    return U, I, bias, ptr, pos


def test_split_invariance_and_determinism(hip_device):
    """item_splits is not observable, and neither is the run: bit-identical ids and scores."""
    U, I, bias, ptr, pos = float_fixture(5, 70, 1007, 48)
    users = np.arange(70)
    base = run(U, I, 0.7, bias, users, 20, (ptr, pos), 1)
    for splits in (1, 3, 7, 0):
        got = run(U, I, 0.7, bias, users, 20, (ptr, pos), splits)
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1].view(np.uint32), base[1].view(np.uint32)), splits


# ---- masking ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("splits", [1, 3])
def test_masking_edge_cases(hip_device, splits):
    n_users, n_items, dim, k = 6, 4 * TILE + 9, 16, 7
    rng = np.random.default_rng(11)
    U, I, bias = tr.integer_fixture(rng, n_users, n_items, dim, True)
    every = np.arange(n_items)
    edges = np.array(sorted({t * TILE + o for t in range(5) for o in (0, TILE - 1) if t * TILE + o < n_items}
                            | {n_items - 1}))
    rows = [np.zeros(0, np.int64),                     # user 0: nothing seen
            every,                                      # user 1: everything seen
            np.delete(every, [3, TILE, n_items - 1]),   # user 2: n_items - 3 seen, k = 7: three results, then padding
            edges,                                      # user 3: first and last item of every tile
            every[every % 2 == 0],                      # user 4: more than four seen items in every tile
            every[: 2 * TILE]]                          # user 5: two whole tiles
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    pos = np.concatenate(rows).astype(np.int64)
    users = np.array([0, 1, 2, 3, 3, 4, 5, 3])          # user 3 queried three times
    s = tr.scores64(U, I, 1.0, bias, users)
    want_i, want_s = tr.exact_topk(s, tr.seen_rows(ptr, pos, users), k)
    got_i, got_s = run(U, I, 1.0, bias, users, k, (ptr, pos), splits)
    assert np.array_equal(got_i, want_i) and np.array_equal(got_s, want_s)
    assert (got_i[1] == -1).all() and np.isneginf(got_s[1]).all()
    assert sorted(got_i[2, :3]) == [3, TILE, n_items - 1] and (got_i[2, 3:] == -1).all() and np.isneginf(got_s[2, 3:]).all()
    assert not np.isin(got_i[3], edges).any() and np.array_equal(got_i[3], got_i[4]) and np.array_equal(got_i[3], got_i[7])
    assert (got_i[5] % 2 == 1).all() and (got_i[6] >= 2 * TILE).all()
    # the same lists from the id-column form of `seen`, and everything unmasked with seen=None
    cols = (np.repeat(np.arange(n_users), np.diff(ptr))[::-1].copy(), pos[::-1].copy())
    again = run(U, I, 1.0, bias, users, k, cols, splits)
    assert np.array_equal(again[0], want_i) and np.array_equal(again[1], want_s)
    free_i, free_s = run(U, I, 1.0, bias, users, k, None, splits)
    want_free = tr.exact_topk(s, None, k)
    assert np.array_equal(free_i, want_free[0]) and np.array_equal(free_s, want_free[1])


# ---- float fixtures ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(300, 1007, 64, 20), (6040, 3706, 64, 20)], ids=["small", "headline"])
def test_float_fixture_against_float64(hip_device, shape):
    n_users, n_items, dim, k = shape
    U, I, bias, ptr, pos = float_fixture(n_users, n_users, n_items, dim)
    users = np.arange(n_users)
    s64 = tr.scores64(U, I, 0.5, bias, users)
    items, scores = run(U, I, 0.5, bias, users, k, (ptr, pos), 0)
    tr.check_against_float64(items, scores, s64, tr.seen_rows(ptr, pos, users), str(shape))


# ---- errors -----------------------------------------------------------------------------------------------------------
def test_errors(hip_device):
    from beta_recsys_amd.recommend import _stats, topk_factors
    from beta_recsys_amd.mf import read_stats

    rng = np.random.default_rng(3)
    U, I, bias = tr.integer_fixture(rng, 9, 100, 8, True)
    users = np.array([2, 9, 5])                      # 9 == n_users
    with pytest.raises(IndexError) as info:
        run(U, I, 1.0, bias, users, 5)
    items, scores = (t.cpu().numpy() for t in info.value.partial)
    want_i, want_s = tr.exact_topk(tr.scores64(U, I, 1.0, bias, np.array([2, 0, 5])), None, 5)
    assert np.array_equal(items[[0, 2]], want_i[[0, 2]]) and np.array_equal(scores[[0, 2]], want_s[[0, 2]])
    assert (items[1] == -1).all() and np.isneginf(scores[1]).all()
    stats = _stats[(hip_device.type, hip_device.index)]
    assert read_stats(stats).status == 0
    got_i, _ = run(U, I, 1.0, bias, np.array([2, 0, 5]), 5)       # ... and the next call is clean
    assert np.array_equal(got_i, want_i)
    with pytest.raises(IndexError):
        run(U, I, 1.0, bias, np.array([-1]), 5)
    Ut, It = dev_t(U, hip_device), dev_t(I, hip_device)
    for k in (0, 129):
        with pytest.raises(ValueError):
            topk_factors(Ut, It, 1.0, None, [0], k)
    with pytest.raises(ValueError):
        topk_factors(torch.zeros(4, 513, device=hip_device), torch.zeros(6, 513, device=hip_device), 1.0, None, [0], 5)
    assert read_stats(stats).status == 0


# ---- model hooks ------------------------------------------------------------------------------------------------------
N_U, N_I = 40, 57


def tiny_graph(seed=7):
    rng = np.random.default_rng(seed)
    R = (rng.random((N_U, N_I)) < 0.12).astype(np.float32)
    R[np.arange(N_U), rng.integers(0, N_I, N_U)] = 1.0
    A = sp.bmat([[None, sp.csr_matrix(R)], [sp.csr_matrix(R.T), None]]).tocsr()
    d = np.asarray(A.sum(axis=1)).reshape(-1)
    dinv = np.where(d > 0, 1.0 / np.sqrt(np.maximum(d, 1e-12)), 0.0)
    norm = (sp.diags(dinv) @ A @ sp.diags(dinv)).tocoo()
    idx = torch.from_numpy(np.vstack((norm.row, norm.col)).astype(np.int64))
    adj = torch.sparse_coo_tensor(idx, torch.from_numpy(norm.data.astype(np.float32)), torch.Size(norm.shape))
    users, items = np.nonzero(R)
    return R, adj, users, items


def tiny_engine(name, R, adj):
    import beta_recsys_amd as hp
    import ultragcn_numpy as ug

    common = dict(n_users=N_U, n_items=N_I, device_str="cuda:0", optimizer="adam", lr=0.01, batch_size=32, regs=[1e-5])
    if name == "mf":
        cls, model = hp.MFEngine, dict(common, emb_dim=12, loss="bpr")
    elif name == "lightgcn":
        cls, model = hp.LightGCNEngine, dict(common, emb_dim=8, layer_size=[8, 8], keep_pro=0.6, norm_adj=adj)
    elif name == "ngcf":
        cls, model = hp.NGCFEngine, dict(common, emb_dim=8, layer_size=[8, 16], mess_dropout=[0.1, 0.1], norm_adj=adj)
    else:
        cls, model = hp.UltraGCNEngine, dict(
            common, emb_dim=20, ii_neighbor_num=4, train_mat=sp.csr_matrix(R),
            constraint_mat={"beta_uD": np.full(N_U, 0.3, np.float32), "beta_iD": np.full(N_I, 0.2, np.float32)},
            **ug.DEFAULT_HP)
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(5)
        eng = cls({"model": model, "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    # weights of a size at which scores are O(1): the tolerance is relative to a user's largest |score|
    gen = torch.Generator().manual_seed(9)
    scale = 0.3 if name == "mf" else 0.6     # (MF's logits go back through a sigmoid: kept where fp32 resolves them)
    sd = {key: torch.randn(v.shape, generator=gen) * (scale if "emb" in key or "bias" in key else 0.3)
          for key, v in eng.model.state_dict().items()}
    eng.model.load_state_dict(sd)
    eng.model.to("cuda:0")
    return eng


@pytest.mark.parametrize("name", ["mf", "lightgcn", "ngcf", "ultragcn"])
def test_model_hooks_rank_like_predict(hip_device, name):
    """Every user's recommend(k=5) against the model's own predict over all (user, item) pairs -- the float-fixture check
    with predict's scores in place of the fp64 ones (MF and LightGCN apply a sigmoid: the logits are recovered in fp64)."""
    R, adj, seen_u, seen_i = tiny_graph()
    eng = tiny_engine(name, R, adj)
    eng.model.eval()
    users = np.arange(N_U)
    uu, ii = np.repeat(users, N_I), np.tile(np.arange(N_I), N_U)
    pred = eng.model.predict(uu, ii).detach().reshape(N_U, N_I).double().cpu()
    s64 = (torch.logit(pred) if name in ("mf", "lightgcn") else pred).numpy()
    items, scores = eng.recommend(users, 5, seen=(seen_u, seen_i))
    items, scores = items.cpu().numpy(), scores.cpu().numpy().astype(np.float64)
    if name == "mf":     # the hook leaves the user and the global bias out: adding them back gives the logits
        sd = eng.model.state_dict()
        scores = scores + sd["user_bias.weight"].cpu().numpy().astype(np.float64).reshape(-1, 1) \
            + float(sd["global_bias"].cpu().reshape(-1)[0])
    rows = [seen_i[seen_u == u] for u in users]
    tr.check_against_float64(items, scores, s64, rows, name)
    again = eng.recommend(users, 5, seen=(seen_u, seen_i), item_splits=1)
    assert np.array_equal(again[0].cpu().numpy(), items)


# ---- metrics ----------------------------------------------------------------------------------------------------------
def test_evaluate_full_matches_evaluate_on_the_explicit_frame(hip_device):
    """evaluate_full == evaluate on the frame of ALL (user, unseen item) rows in ascending item order with the exact
    scores and rating 1 on the test items: both are fp64 sums of the same terms over users (1e-9 relative)."""
    import beta_recsys_amd as hp

    n_users, n_items, dim = 30, 150, 8
    rng = np.random.default_rng(21)
    U, I, bias = tr.integer_fixture(rng, n_users, n_items, dim, True)
    ptr, pos = tr.random_seen(rng, n_users, n_items, 20)
    s = tr.scores64(U, I, 1.0, bias, np.arange(n_users))
    full_i, _ = tr.exact_topk(s, tr.seen_rows(ptr, pos, np.arange(n_users)), 20)
    test_u, test_i, test_r = [], [], []
    for u in range(n_users):
        unseen = np.setdiff1d(np.arange(n_items), pos[ptr[u]:ptr[u + 1]])
        if u % 5 == 0:
            continue                                          # no test row at all
        if u == 7:
            picks = np.setdiff1d(unseen, full_i[u])[:3]       # every test item outside the top 20
        elif u == 8:
            picks = unseen[:2]                                # rows, but none relevant (rating 0)
        else:
            picks = rng.choice(unseen, size=int(rng.integers(1, 6)), replace=False)
        for it in picks:
            test_u.append(u), test_i.append(int(it)), test_r.append(0.0 if u == 8 else 1.0)
    test_u, test_i, test_r = np.array(test_u), np.array(test_i), np.array(test_r, dtype=np.float32)
    assert not np.isin(test_i[test_u == 7], full_i[7]).any()
    truth = {(int(a), int(b)) for a, b, r in zip(test_u, test_i, test_r) if r >= 1}
    fu, fs, fr = [], [], []
    for u in np.unique(test_u):
        unseen = np.setdiff1d(np.arange(n_items), pos[ptr[u]:ptr[u + 1]])
        fu.append(np.full(len(unseen), u)), fs.append(s[u, unseen])
        fr.append(np.array([1.0 if (int(u), int(it)) in truth else 0.0 for it in unseen], dtype=np.float32))
    frame = {"col_user": np.concatenate(fu), "col_rating": np.concatenate(fr)}
    metrics, ks = ["ndcg", "map", "precision", "recall"], [1, 5, 10, 20]
    want = hp.eval.evaluate(frame, np.concatenate(fs).astype(np.float32), metrics, ks, device=hip_device)

    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.MFEngine({"model": dict(n_users=n_users, n_items=n_items, emb_dim=dim, device_str="cuda:0",
                                         optimizer="sgd", lr=0.05, batch_size=16, loss="bpr"),
                           "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    eng.model.load_state_dict({"user_emb.weight": torch.from_numpy(U), "item_emb.weight": torch.from_numpy(I),
                               "user_bias.weight": torch.zeros(n_users, 1), "global_bias": torch.zeros(1),
                               "item_bias.weight": torch.from_numpy(bias).reshape(-1, 1)})
    eng.model.to("cuda:0")
    test_df = {"col_user": test_u, "col_item": test_i, "col_rating": test_r}
    train_df = {"col_user": np.repeat(np.arange(n_users), np.diff(ptr)), "col_item": pos}
    got = hp.evaluate_full(eng, test_df, train_df, metrics=metrics, k_li=ks)
    assert list(got) == list(want) == [f"{m}@{k}" for k in ks for m in metrics]
    for key in want:
        assert got[key] == pytest.approx(want[key], rel=1e-9, abs=0), (key, got[key], want[key])
    assert 0 < got["recall@20"] < 1          # some test items are found, and user 7's never are
    assert hp.evaluate_full(eng.model, test_df, train_df, metrics=metrics, k_li=ks) == got
