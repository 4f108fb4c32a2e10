"""float64 / float32 numpy restatement of ItemKNN and UserKNN (test infrastructure): what beta_rec/models/itemKNN.py
and userKNN.py compute when their building blocks are handed the user's items, on a dense ``B``.

``B[u, i]`` is the number of times the pair (u, i) occurs in the training frame (the reference does not binarise).
Neighbour order is ``lexsort((ids, -sim))``: by sim descending, ties to the lower user id (the reference's
``argpartition`` leaves ties at the cut open).

One named defect switch: ``sequence="row_coordinate"`` feeds ``nnz(u)`` zeros as the user's sequence, which is what the
reference's ``predict`` does (``getrow(u).nonzero()[0]`` is the row coordinate of a one-row matrix); ``"items"`` feeds
the user's items.
"""
import numpy as np

SEQUENCES = ("items", "row_coordinate")


def dense_matrix(users, items, n_users, n_items):
    B = np.zeros((n_users, n_items), dtype=np.float64)
    np.add.at(B, (np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)), 1.0)
    return B


def sequence_of(B, u, sequence="items"):
    if sequence not in SEQUENCES:
        raise ValueError(f"sequence must be one of {SEQUENCES}")
    own = np.nonzero(B[u])[0]
    return own if sequence == "items" else np.zeros(len(own), dtype=np.int64)


def _scaled(overlap, mass):
    out = overlap.astype(np.float64).copy()
    nz = out != 0
    out[nz] /= np.sqrt(mass[nz])
    return out


def item_similarity(B):
    """S [n_items, n_items] float32: S[i, j] = overlap_i[j] / sqrt(cnt[j]), overlap over the distinct users of i."""
    cnt = B.sum(axis=0)
    overlap = (B > 0).astype(np.float64).T @ B          # integers: exact in any order
    S = np.zeros(overlap.shape, dtype=np.float32)
    for i in range(B.shape[1]):
        S[i] = _scaled(overlap[i], cnt)
    return S


def item_score_row(B, S, u, sequence="items"):
    """float32 [n_items]: the rows S[i, :] of the sequence added one at a time, in order; zeros for an empty one."""
    acc = None
    for i in sequence_of(B, u, sequence):
        acc = S[i] if acc is None else np.add(acc, S[i])
    return np.zeros(B.shape[1], dtype=np.float32) if acc is None else acc.copy()


def user_similarity(B, seq):
    """float64 [n_users]: overlap of the sequence (a repeated entry counts as often as it is repeated, as
    get_sparse_vector sums it) with every user's row, over sqrt(cu)."""
    x = np.zeros(B.shape[1], dtype=np.float64)
    np.add.at(x, seq, 1.0)
    return _scaled(B @ x, B.sum(axis=1))


def neighbours(B, u, k, sequence="items"):
    """(ids[k] int64, sims[k] float64), best first; k is clamped to n_users."""
    sim = user_similarity(B, sequence_of(B, u, sequence))
    k = min(int(k), B.shape[0])
    ids = np.lexsort((np.arange(B.shape[0]), -sim))[:k]
    return ids.astype(np.int64), sim[ids]


def user_score_row(B, u, k, sequence="items"):
    """float64 [n_items]: sum over the neighbours, best first, of sim[v] * B[v, :]; -inf on the sequence."""
    ids, sims = neighbours(B, u, k, sequence)
    acc = np.zeros(B.shape[1], dtype=np.float64)
    for v, s in zip(ids, sims):
        acc = acc + s * B[v]
    acc[sequence_of(B, u, sequence)] = -np.inf
    return acc


def topk_of_row(row32, seen, k):
    """(ids[k] int64, scores[k] float32) of a float32 score row: recommend()'s rules -- score descending, ties to the
    lower id, -0 == +0, never a seen item nor one at -inf, -1 / -inf in the tail."""
    row = np.asarray(row32, dtype=np.float32) + np.float32(0)      # -0 -> +0
    ok = np.isfinite(row) | (row == np.inf)
    ok[np.asarray(list(seen), dtype=np.int64)] = False
    cand = np.nonzero(ok)[0]
    order = cand[np.argsort(-row[cand], kind="stable")][:k]
    ids = np.full(k, -1, dtype=np.int64)
    scores = np.full(k, -np.inf, dtype=np.float32)
    ids[:len(order)] = order
    scores[:len(order)] = row[order]
    return ids, scores
