"""Host-side checks of the neighbourhood models that need no GPU: the symbols are declared, exported and bound; every C
entry point validates its arguments before any HIP call; ``max_sim_bytes`` is enforced; the CSR-with-multiplicity
builder agrees with scipy on the golden fixtures; ``recommend`` / ``evaluate_full`` still refuse a model with neither
hook."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("hiprec_knn_workspace_bytes", "hiprec_knn_item_similarity", "hiprec_knn_item_scores",
           "hiprec_knn_user_scores")
NONE = (1 << 64) - 1           # hiprec_knn_workspace_bytes for bad sizes


def test_symbols_are_declared_exported_and_bound():
    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib, knn

    header = open(os.path.join(ROOT, "include", "hiprec.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in header, f"{name} is not declared in include/hiprec.h"
        assert name in _lib.SIGNATURES, f"_lib.py has no prototype for {name}"
        assert hasattr(lib, name), f"libhiprec.so does not export {name}"
    assert "#define HIPREC_KNN_MAX_K 128" in header and f"#define HIPREC_KNN_LDS_CAP {knn.LDS_CAP}" in header
    assert knn.MAX_K == 128 and lib.hiprec_version() == 100
    for cls in (hp.ItemKNN, hp.ItemKNNEngine, hp.UserKNN, hp.UserKNNEngine):
        assert getattr(knn, cls.__name__) is cls
    for cls in (hp.ItemKNN, hp.UserKNN):
        for method in ("prepare_model", "predict", "recommend", "topk_items", "seen_csr"):
            assert callable(getattr(cls, method)), (cls.__name__, method)
    assert callable(hp.UserKNN.neighbours)


def test_workspace_bytes_follow_the_accumulator_form():
    from beta_recsys_amd import _lib, knn

    ws = _lib.load().hiprec_knn_workspace_bytes
    cap = knn.LDS_CAP
    # the LDS form needs no workspace; one entry more than the cap, or a forced cap of 1, gives the workspace form
    assert ws(0, 50, cap, 0, 0) == 0 and ws(1, 50, cap, 10, 0) == 0 and ws(2, cap, 100, 10, 0) == 0
    assert ws(0, 50, cap + 1, 0, 0) == 1024 * (cap + 1) * 8           # one slice per block, at most 1024 blocks
    assert ws(0, 50, 30, 0, 1) == 30 * 30 * 8                         # uint32 overlaps + int32 touched list
    assert ws(1, 50, 30, 7, 1) == 7 * 30 * 4                          # the fp32 row
    assert ws(2, 50, 30, 7, 1) == 7 * (50 * 8 + 200)                  # max(n_users, n_items) 64-bit entries + list
    assert ws(2, 30, 51, 7, 1) == 7 * (51 * 8 + 208)                  # (the list is padded to 8 bytes)
    assert ws(2, 50, 30, 5000, 1) == 1024 * (50 * 8 + 200)
    assert ws(2, 50, 30, 7, 49) == ws(2, 50, 30, 7, 1) and ws(2, 50, 30, 7, 50) == 0
    for bad in ((3, 5, 5, 1, 0), (-1, 5, 5, 1, 0), (0, 0, 5, 1, 0), (0, 5, 0, 1, 0), (1, 5, 5, -1, 0), (1, 5, 5, 1, -1),
                (2, 1 << 31, 5, 1, 0), (2, 5, 1 << 31, 1, 0)):
        assert ws(*bad) == NONE, bad


def test_entry_points_validate_before_touching_the_gpu():
    """(the non-NULL pointers are never dereferenced: validation fails first)"""
    from beta_recsys_amd import _lib

    lib = _lib.load()
    P = 64

    def sim(bt=P, b=P, val=P, cnt=P, n_users=10, n_items=20, S=P, lds=20, cap=0, work=None, work_bytes=0):
        return lib.hiprec_knn_item_similarity(bt, bt, b, b, val, cnt, n_users, n_items, S, lds, cap, work, work_bytes, None)

    assert sim(n_items=0) == -1 and b"bad sizes" in lib.hiprec_last_error()
    assert sim(n_users=0) == -1 and sim(cap=-1) == -1 and sim(n_items=1 << 31, lds=1 << 31) == -1
    assert sim(lds=19) == -1 and b"leading" in lib.hiprec_last_error()
    for null in ("bt", "b", "val", "cnt", "S"):
        assert sim(**{null: None}) == -1 and b"NULL" in lib.hiprec_last_error(), null
    assert sim(cap=1) == -1 and b"workspace" in lib.hiprec_last_error()                     # needs 3200 B, got none
    assert sim(cap=1, work=P, work_bytes=20 * 20 * 8 - 1) == -1 and b"workspace" in lib.hiprec_last_error()

    def item(b=P, n_users=10, n_items=20, S=P, lds=20, q=P, n_query=3, pp=None, pi=None, pick=None, topk=5, sp=None,
             si=None, oi=P, osc=P, cap=0, work=None, work_bytes=0, stats=P):
        return lib.hiprec_knn_item_scores(b, b, n_users, n_items, S, lds, q, n_query, pp, pi, pick, topk, sp, si, oi, osc,
                                          cap, work, work_bytes, stats, None)

    def user(b=P, val=P, bt=P, cu=P, n_users=10, n_items=20, k=4, q=P, n_query=3, nb_i=None, nb_s=None, pp=None, pi=None,
             pick=None, topk=5, sp=None, si=None, oi=P, osc=P, cap=0, work=None, work_bytes=0, stats=P):
        return lib.hiprec_knn_user_scores(b, b, val, bt, bt, val, cu, n_users, n_items, k, q, n_query, nb_i, nb_s, pp, pi,
                                          pick, topk, sp, si, oi, osc, cap, work, work_bytes, stats, None)

    for call in (item, user):
        for bad_topk in (-1, 129):
            assert call(topk=bad_topk) == -1 and b"topk=" in lib.hiprec_last_error()
        assert call(n_items=0) == -1 and b"bad sizes" in lib.hiprec_last_error()
        assert call(n_query=-1) == -1 and call(cap=-1) == -1 and call(n_users=0) == -1
        assert call(stats=None) == -1 and b"stats" in lib.hiprec_last_error()
        assert call(pp=P) == -1 and b"pair" in lib.hiprec_last_error()                      # no pair_items / out_pick
        assert call(pp=P, pi=P) == -1 and call(oi=None) == -1 and call(osc=None) == -1
        assert call(sp=P) == -1 and b"CSR" in lib.hiprec_last_error()
        assert call(si=P) == -1
        assert call(b=None) == -1 and b"NULL" in lib.hiprec_last_error()
        assert call(q=None) == -1
        assert call(cap=1) == -1 and b"workspace" in lib.hiprec_last_error()
        assert call(cap=1, work=P, work_bytes=8) == -1 and b"workspace" in lib.hiprec_last_error()
        assert call(n_query=0) == 0                                                         # nothing to do: no launch
    assert item(lds=19) == -1 and b"leading" in lib.hiprec_last_error()
    assert item(S=None) == -1
    for bad_k in (0, 129, -2):
        assert user(k=bad_k) == -1 and b"k=" in lib.hiprec_last_error()
    assert user(k=11) == -1 and b"neighbours" in lib.hiprec_last_error()                    # more than n_users
    assert user(nb_i=P) == -1 and b"neighbour" in lib.hiprec_last_error()
    assert user(cu=None) == -1 and user(val=None) == -1 and user(bt=None) == -1


def test_python_level_limits_need_no_gpu():
    import beta_recsys_amd as hp
    from beta_recsys_amd import knn

    cfg = dict(n_users=10, n_items=20, neighbourhood_size=4, device_str="cpu")
    for bad in (0, 129):
        with pytest.raises(ValueError, match="neighbourhood_size"):
            hp.UserKNN(dict(cfg, neighbourhood_size=bad))
    assert hp.UserKNN(dict(cfg, neighbourhood_size=128)).k == 10                            # clamped to n_users
    hp.ItemKNN(dict(cfg, neighbourhood_size=1000))                                          # read, never used
    with pytest.raises(ValueError, match="1600 bytes"):
        hp.ItemKNN(dict(cfg, max_sim_bytes=1599))
    hp.ItemKNN(dict(cfg, max_sim_bytes=1600))
    assert knn.DEFAULT_MAX_SIM_BYTES == 4 << 30
    with pytest.raises(ValueError, match=str(40000 * 40000 * 4)):
        hp.ItemKNN(dict(cfg, n_items=40000))                                                # 6.4 GB > the default
    model = hp.UserKNN(cfg)
    with pytest.raises(RuntimeError, match="prepare_model"):
        model.predict([0], [0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.prepare_model((np.array([0, 1]), np.array([2, 3])))
    # the engines: no base constructor, nothing to train
    with contextlib.redirect_stdout(io.StringIO()) as out:
        eng = hp.UserKNNEngine({"model": cfg})
        assert eng.train_single_batch(None) == 0
        eng.train_an_epoch(None, 3)
    assert out.getvalue() == "userKNNEngine init\n[Training Epoch 3] skipped\n"
    assert isinstance(eng.model, hp.UserKNN) and not hasattr(eng, "optimizer")
    with contextlib.redirect_stdout(io.StringIO()) as out:
        eng = hp.ItemKNNEngine({"model": cfg})
        eng.train_an_epoch(None, 0)
    assert out.getvalue() == "[Training Epoch 0] skipped\n" and eng.train_single_batch(None) == 0


@pytest.mark.parametrize("name", ("knn_k3", "knn_k8", "knn_kbig"))
def test_csr_with_multiplicity_agrees_with_scipy(name):
    import scipy.sparse as ssp

    from beta_recsys_amd.knn import _row_sums, build_interaction_csr

    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    U, I = int(g["meta"][0]), int(g["meta"][1])
    users, items = g["users"], g["items"]
    ref = ssp.coo_matrix((np.ones(len(users)), (users, items)), shape=(U, I)).tocsr()
    ref.sum_duplicates()
    ref.sort_indices()
    for (rows, cols, n_rows, n_cols), want in (((users, items, U, I), ref), ((items, users, I, U), ref.T.tocsr())):
        want.sort_indices()
        ptr, idx, val = build_interaction_csr(torch.from_numpy(rows), torch.from_numpy(cols), n_rows, n_cols)
        assert ptr.dtype == torch.int64 and idx.dtype == torch.int64 and val.dtype == torch.float32
        assert ptr.tolist() == want.indptr.tolist() and idx.tolist() == want.indices.tolist()
        assert val.tolist() == want.data.tolist() and val.max() == 2
        sums = _row_sums((ptr, idx, val))
        assert sums.dtype == torch.float64 and sums.tolist() == np.asarray(want.sum(axis=1)).ravel().tolist()
    with pytest.raises(IndexError):
        build_interaction_csr(torch.tensor([U]), torch.tensor([0]), U, I)
    with pytest.raises(ValueError):
        build_interaction_csr(torch.tensor([0, 1]), torch.tensor([0]), U, I)
    ptr, idx, val = build_interaction_csr(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), U, I)
    assert ptr.tolist() == [0] * (U + 1) and idx.numel() == 0 and val.numel() == 0


def test_recommend_and_evaluate_full_still_refuse_a_model_with_neither_hook():
    import beta_recsys_amd as hp
    from beta_recsys_amd.recommend import recommend

    class Neither:
        pass

    with pytest.raises(NotImplementedError, match="no ranking_factors"):
        recommend(Neither(), [0], 3)
    with pytest.raises(NotImplementedError, match="no ranking_factors"):
        hp.evaluate_full(Neither(), {"col_user": [0], "col_item": [1]})
    cfg = dict(n_users=6, n_items=5, emb_dim=4, mlp_config={"n_layers": 2}, dropout=0.0, device_str="cpu")
    with contextlib.redirect_stdout(io.StringIO()):
        neumf = hp.NeuMF(cfg)
    with pytest.raises(NotImplementedError, match="bilinear"):
        recommend(neumf, [0], 3)
    with pytest.raises(NotImplementedError, match="bilinear"):
        hp.evaluate_full(neumf, {"col_user": [0], "col_item": [1]})
    # the hook is taken before ranking_factors() is asked for
    calls = []

    class Hooked:
        def topk_items(self, users, k, seen, item_splits):
            calls.append((list(users), k, seen, item_splits))
            return "items", "scores"

        def ranking_factors(self):
            raise AssertionError("ranking_factors() asked for although the model has topk_items()")

    assert recommend(Hooked(), [4, 2], 3) == ("items", "scores") and calls == [([4, 2], 3, None, 0)]
