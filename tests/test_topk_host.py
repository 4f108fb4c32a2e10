"""Host-side checks of full-catalogue top-K recommendation that need no GPU: the new symbols are declared, exported and
bound; the C entry points validate their arguments before any HIP call; ``seen`` is normalised from all three input
forms; models without a bilinear score refuse the hook."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hiprec_topk_workspace_bytes", "hiprec_topk_recommend", "hiprec_topk_metrics")


def test_symbols_are_declared_exported_and_bound():
    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib

    header = open(os.path.join(ROOT, "include", "hiprec.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert name + "(" in header, f"{name} is not declared in include/hiprec.h"
        assert name in _lib.SIGNATURES, f"_lib.py has no prototype for {name}"
        assert hasattr(lib, name), f"libhiprec.so does not export {name}"
    assert "#define HIPREC_TOPK_MAX_K 128" in header
    from beta_recsys_amd.recommend import MAX_DIM, MAX_K, recommend, topk_factors  # noqa: F401

    assert (MAX_K, MAX_DIM) == (128, 512)
    assert hp.recommend is recommend and callable(hp.evaluate_full) and hp.evaluate_full is hp.eval.evaluate_full
    for cls in (hp.MF, hp.LightGCN, hp.NGCF, hp.UltraGCN, hp.NeuMF, hp.PairwiseGMF, hp.Triple2vec):
        assert callable(getattr(cls, "ranking_factors")), cls.__name__
    assert callable(hp.ModelEngine.recommend)
    import __graft_entry__ as entry

    assert "topk.hip" in entry.EVIDENCE_GROUPS["topk"] and entry.evidence_group("topk_headline") == "topk"


def test_entry_points_validate_before_touching_the_gpu():
    from beta_recsys_amd import _lib

    lib = _lib.load()
    ws = lib.hiprec_topk_workspace_bytes
    assert ws(10, 100, 5, 1) == 10 * 5 * 8 and ws(10, 1007, 7, 3) == 10 * 3 * 7 * 8
    assert ws(10, 64, 5, 7) == 10 * 5 * 8          # one tile of items: one range, whatever was asked for
    assert ws(10, 1007, 7, 0) >= 10 * 7 * 8 and ws(4096, 1000000, 20, 0) >= 4096 * 20 * 8
    assert ws(10, 100, 0, 1) == 0 and ws(10, 100, 129, 1) == 0 and ws(10, 0, 5, 1) == 0 and ws(-1, 100, 5, 1) == 0

    def call(k=5, dim=8, ldu=8, ldi=8, n_items=100, n_query=3, u=64, i=64, q=64, ptr=None, pos=None, work=64,
             work_bytes=1 << 20, out=64, stats=64, splits=0):
        return lib.hiprec_topk_recommend(u, ldu, 10, i, ldi, n_items, dim, 1.0, None, q, n_query, ptr, pos, k, splits,
                                         work, work_bytes, out, out, stats, None)

    # (the non-NULL pointers are never dereferenced: validation fails first)
    for bad_k in (0, 129, -3):
        assert call(k=bad_k) == -1 and b"k=" in lib.hiprec_last_error()
    for bad_dim in (0, 513):
        assert call(dim=bad_dim, ldu=600, ldi=600) == -1 and b"dim=" in lib.hiprec_last_error()
    assert call(n_items=0) == -1 and b"bad sizes" in lib.hiprec_last_error()
    assert call(n_query=-1) == -1 and call(splits=-1) == -1
    assert call(ldu=4) == -1 and b"leading" in lib.hiprec_last_error()
    assert call(u=None) == -1 and b"NULL" in lib.hiprec_last_error()
    assert call(out=None) == -1 and call(stats=None) == -1 and call(work=None) == -1
    assert call(ptr=64) == -1 and b"CSR" in lib.hiprec_last_error()
    assert call(work_bytes=8) == -1 and b"workspace" in lib.hiprec_last_error()

    ks = (ctypes.c_int32 * 2)(5, 10)
    out = (ctypes.c_double * 9)()
    met = lambda k=10, n_k=2, kl=ks, w=64, wb=1 << 20, o=out, items=64, ptr=64: lib.hiprec_topk_metrics(  # noqa: E731
        items, 4, k, ptr, 64, kl, n_k, w, wb, o, None)
    assert met(n_k=0) == -1 and b"n_k=0" in lib.hiprec_last_error()
    assert met(n_k=9) == -1
    assert met(k=8) == -1 and b"k[1]=10" in lib.hiprec_last_error()      # a cut-off beyond the lists' length
    assert met(kl=(ctypes.c_int32 * 2)(5, 0)) == -1
    assert met(o=None) == -1 and met(items=None) == -1 and met(ptr=None) == -1
    assert met(wb=8) == -1 and b"workspace" in lib.hiprec_last_error()


def test_python_level_argument_checks_need_no_gpu():
    from beta_recsys_amd.recommend import topk_factors

    U, I = torch.zeros(4, 8), torch.zeros(6, 8)
    for k in (0, 129):
        with pytest.raises(ValueError, match="k must be"):
            topk_factors(U, I, 1.0, None, [0], k)
    with pytest.raises(ValueError, match="factor width"):
        topk_factors(torch.zeros(4, 513), torch.zeros(6, 513), 1.0, None, [0], 5)
    with pytest.raises(ValueError):
        topk_factors(U, torch.zeros(6, 9), 1.0, None, [0], 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        topk_factors(U, I, 1.0, None, [0], 5)


def test_seen_is_normalised_from_all_three_forms():
    from beta_recsys_amd.data import build_positive_csr
    from beta_recsys_amd.recommend import normalise_seen

    cpu = torch.device("cpu")
    n_users, n_items = 5, 9
    users = np.array([3, 0, 3, 3, 1, 0, 3])
    items = np.array([8, 2, 1, 8, 0, 2, 4])       # duplicates: (3, 8) and (0, 2)
    assert normalise_seen(None, n_users, n_items, cpu) is None
    ptr, pos = normalise_seen((users, items), n_users, n_items, cpu)
    assert ptr.tolist() == [0, 1, 2, 2, 5, 5] and pos.tolist() == [2, 0, 1, 4, 8]
    assert ptr.dtype == torch.int64 and pos.dtype == torch.int64
    # the CSR form comes back as it is (int32 numpy in, int64 tensors out), lists of ids work like arrays
    ptr2, pos2 = normalise_seen((ptr.numpy().astype(np.int32), pos.numpy().astype(np.int32)), n_users, n_items, cpu)
    assert torch.equal(ptr2, ptr) and torch.equal(pos2, pos) and ptr2.dtype == torch.int64
    ptr3, pos3 = normalise_seen((users.tolist(), items.tolist()), n_users, n_items, cpu)
    assert torch.equal(ptr3, ptr) and torch.equal(pos3, pos)
    ref_ptr, ref_pos = build_positive_csr(torch.from_numpy(users), torch.from_numpy(items), n_users, n_items)
    assert torch.equal(ref_ptr, ptr) and torch.equal(ref_pos, pos)
    # n_users + 1 id rows: both readings have the right lengths; a pointer starts at 0 and ends at nnz, ids do not
    six_u, six_i = np.array([4, 4, 0, 1, 2, 3]), np.array([1, 0, 5, 5, 5, 5])
    p, s = normalise_seen((six_u, six_i), n_users, n_items, cpu)
    assert p.tolist() == [0, 1, 2, 3, 4, 6] and s.tolist() == [5, 5, 5, 5, 0, 1]
    csr6 = (np.array([0, 2, 2, 3, 6, 6]), np.array([1, 7, 0, 2, 3, 4]))
    p, s = normalise_seen(csr6, n_users, n_items, cpu)
    assert p.tolist() == csr6[0].tolist() and s.tolist() == csr6[1].tolist()
    # an empty history
    p, s = normalise_seen((np.zeros(0, np.int64), np.zeros(0, np.int64)), n_users, n_items, cpu)
    assert p.tolist() == [0] * 6 and s.numel() == 0
    with pytest.raises(ValueError):
        normalise_seen((users, items[:-1]), n_users, n_items, cpu)
    with pytest.raises(ValueError):
        normalise_seen((np.array([0, 1, 1, 2, 2, 7]), np.array([1, 2])), n_users, n_items, cpu)   # ends beyond nnz
    with pytest.raises(IndexError):
        normalise_seen((np.array([0, 1, 1, 2, 2, 2]), np.array([1, 9])), n_users, n_items, cpu)   # item id 9 of 9
    with pytest.raises(IndexError):
        normalise_seen((np.array([5]), np.array([0])), n_users, n_items, cpu)                     # user id 5 of 5
    with pytest.raises(ValueError):
        normalise_seen(users, n_users, n_items, cpu)


def test_models_without_a_bilinear_score_refuse_the_hook():
    import beta_recsys_amd as hp
    from beta_recsys_amd.recommend import ranking_factors, recommend

    cfg = dict(n_users=6, n_items=5, emb_dim=4, mlp_config={"n_layers": 2}, dropout=0.0, device_str="cpu")
    with contextlib.redirect_stdout(io.StringIO()):
        made = [cls(cfg) for cls in (hp.NeuMF, hp.GMF, hp.MLP)]
    for m in made:
        with pytest.raises(NotImplementedError, match="bilinear"):
            ranking_factors(m)
    with pytest.raises(NotImplementedError, match="bilinear"):
        recommend(made[0], [0], 3)
    with pytest.raises(NotImplementedError, match="stub"):
        hp.PairwiseGMF.ranking_factors(hp.PairwiseGMF.__new__(hp.PairwiseGMF))
    with pytest.raises(NotImplementedError, match="derived item table"):
        hp.Triple2vec.ranking_factors(hp.Triple2vec.__new__(hp.Triple2vec))
    with pytest.raises(NotImplementedError, match="no ranking_factors"):
        ranking_factors(object())


def test_float_check_is_one_fp32_arithmetic_can_meet():
    """The GPU suite's float-fixture bound (tests/topk_reference.py) on the CPU: the top 20 of plain fp32 numpy scores,
    ranked by those scores, pass it against the fp64 scores at the small float fixture's shape -- and a list with one
    item swapped for a clearly worse one, or one score off by 3e-5 of the row's scale, does not."""
    import topk_reference as tr

    rng = np.random.default_rng(300)
    U = rng.standard_normal((300, 64)).astype(np.float32)
    I = rng.standard_normal((1007, 64)).astype(np.float32)
    bias = rng.standard_normal(1007).astype(np.float32)
    ptr, pos = tr.random_seen(rng, 300, 1007, 40)
    users = np.arange(300)
    seen = tr.seen_rows(ptr, pos, users)
    s64 = tr.scores64(U, I, 0.5, bias, users)
    s32 = (np.float32(0.5) * (U @ I.T) + bias[None, :]).astype(np.float32)
    items, scores = tr.exact_topk(s32, seen, 20)
    tr.check_against_float64(items, scores, s64, seen, "fp32 numpy")
    worst = int(np.argmin(s64[0]))
    bad = items.copy()
    bad[0, 19] = worst if worst not in seen[0] and worst not in items[0] else bad[0, 19]
    if bad[0, 19] != items[0, 19]:
        bad_scores = scores.copy()
        bad_scores[0, 19] = s32[0, worst]
        with pytest.raises(AssertionError):
            tr.check_against_float64(bad, bad_scores, s64, seen, "swapped")
    off = scores.copy()
    off[3, 0] += np.float32(3e-5 * np.abs(s64[3]).max())
    with pytest.raises(AssertionError):
        tr.check_against_float64(items, off, s64, seen, "score off")
