"""The numpy restatement of ItemKNN / UserKNN (tests/knn_numpy.py) against vectors captured from the real reference
(tools/gen_golden_knn.py -> tests/golden/knn_*.npz).  CPU only.

The golden holds two kinds of record: the reference's building blocks driven with the user's real items (what the
mirror computes), and the reference's unmodified ``predict`` output, which the restatement reproduces exactly with its
``sequence="row_coordinate"`` switch -- the pin on the reading that ``getrow(u).nonzero()[0]`` is ``nnz(u)`` zeros.
Reference-produced neighbours and scores are compared on ``untied`` users only (argpartition leaves ties at the cut
open); the neighbour ids compared are those with a non-zero sim (which zero-sim users fill the list is open too)."""
import os

import numpy as np
import pytest

import knn_numpy as kn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("knn_k3", "knn_k5", "knn_k8", "knn_kbig")


def load(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    U, I, k, _ = (int(x) for x in g["meta"])
    return g, kn.dense_matrix(g["users"], g["items"], U, I), U, I, k


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_gives_the_golden_similarity_matrix_and_item_rows_bit_for_bit(name):
    g, B, U, I, k = load(name)
    assert np.array_equal(B.sum(axis=0), g["cnt"]) and np.array_equal(B.sum(axis=1), g["cu"])
    assert B.max() >= 2, "the fixture has no duplicated pair"
    S = kn.item_similarity(B)
    assert S.dtype == np.float32 and S.tobytes() == g["S"].tobytes()
    for u in range(U):
        row = kn.item_score_row(B, S, u)
        assert row.dtype == np.float32
        if g["item_rows_valid"][u]:
            assert row.tobytes() == g["item_rows"][u].tobytes(), u
        else:
            assert not row.any()            # no defined answer in the reference: zeros


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_gives_the_golden_neighbours_and_user_scores_on_untied_users(name):
    g, B, U, I, k = load(name)
    k_eff = min(k, U)
    untied = g["untied"]
    assert untied.sum() >= 10
    for u in range(U):
        assert kn.user_similarity(B, kn.sequence_of(B, u)).tobytes() == g["sims"][u].tobytes(), u
        if not untied[u]:
            continue
        ids, sims = kn.neighbours(B, u, k)
        assert len(ids) == k_eff
        ref_ids, ref_sims = g["nb_ids"][u], g["nb_sims"][u]
        assert set(ids[sims > 0]) == set(ref_ids[ref_sims > 0]), u
        assert np.array_equal(np.sort(sims), np.sort(ref_sims)), u
        row, ref = kn.user_score_row(B, u, k), g["user_rows"][u]
        fin = np.isfinite(ref)
        assert np.array_equal(fin, np.isfinite(row)), u
        # both sides sum at most k non-negative doubles, in different orders
        assert np.all(np.abs(row[fin] - ref[fin]) <= k_eff * 2.0 ** -52 * ref[fin]), u


@pytest.mark.parametrize("name", FIXTURES[:3])
def test_row_coordinate_sequence_gives_the_references_raw_predict_exactly(name):
    """The defect, pinned: fed nnz(u) zeros as the sequence, the restatement IS the reference's predict."""
    g, B, U, I, k = load(name)
    S = kn.item_similarity(B)
    users, items = g["raw_users"], g["raw_items"]
    got_item = np.array([kn.item_score_row(B, S, u, "row_coordinate")[j] for u, j in zip(users, items)], dtype=np.float32)
    assert got_item.tobytes() == g["raw_item_predict"].tobytes()
    got_user = np.array([kn.user_score_row(B, u, k, "row_coordinate")[j] for u, j in zip(users, items)])
    raw = g["raw_user_predict"]
    assert raw.dtype == np.float64 and got_user.tobytes() == raw.tobytes()
    # ... and it is NOT what the user's items give: the two readings differ on these fixtures
    real_item = np.array([kn.item_score_row(B, S, u)[j] for u, j in zip(users, items)], dtype=np.float32)
    assert not np.array_equal(real_item, g["raw_item_predict"])
    assert (got_user[items == 0] == -np.inf).all()      # every non-empty user "has" item 0 under the defect


def test_topk_of_row_follows_the_rules_of_recommend():
    row = np.array([1.0, -0.0, 3.0, 0.0, 3.0, -np.inf, 2.0], dtype=np.float32)
    ids, scores = kn.topk_of_row(row, {6}, 6)
    assert ids.tolist() == [2, 4, 0, 1, 3, -1] and scores[:5].tolist() == [3.0, 3.0, 1.0, 0.0, 0.0]
    assert scores[5] == -np.inf and scores.dtype == np.float32


def test_wiring_entries_are_present():
    import __graft_entry__ as ge
    from beta_recsys_amd import compat

    assert compat.MIRRORS["beta_rec.models.itemKNN"] == "knn" and compat.MIRRORS["beta_rec.models.userKNN"] == "knn"
    assert ge.EVIDENCE_GROUPS["knn"] == ["common.hpp", "util.hip", "knn.hip"]
    assert ge.evidence_group("knn") == "knn" and ge.evidence_group("knn_ml1m") == "knn"
