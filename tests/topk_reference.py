"""numpy restatement of full-catalogue top-K (tests only): the exact order for fixtures whose scores are exact in fp32,
and the tolerance check for float fixtures."""
import numpy as np

REL = 1e-5       # the suite's relative bound (helpers.REL), here on the scale of a user's largest |score|


def integer_fixture(rng, n_users, n_items, dim, with_bias):
    """Tables of integers in [-3, 3] and a bias in multiples of 0.5: every dot product (|.| <= 9 * 512) and every
    alpha in {1, 0.25} multiple of it is exact in fp32 in any summation order, and ties are plentiful."""
    U = rng.integers(-3, 4, (n_users, dim)).astype(np.float32)
    I = rng.integers(-3, 4, (n_items, dim)).astype(np.float32)
    bias = (rng.integers(-4, 5, n_items) * 0.5).astype(np.float32) if with_bias else None
    return U, I, bias


def scores64(U, I, alpha, bias, users):
    s = alpha * (U[users].astype(np.float64) @ I.astype(np.float64).T)
    return s if bias is None else s + bias.astype(np.float64)[None, :]


def seen_rows(ptr, pos, users):
    return [np.asarray(pos[ptr[u]:ptr[u + 1]]) for u in users]


def random_seen(rng, n_users, n_items, mean_len):
    """(user_ptr, pos_sorted) numpy int64: per user a random subset, ascending."""
    rows = [np.sort(rng.choice(n_items, size=min(n_items, int(rng.integers(0, 2 * mean_len + 1))), replace=False))
            for _ in range(n_users)]
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int64)


def exact_topk(scores, seen, k):
    """(items[n, k] int64, scores[n, k] float32): score descending, ties to the lower id, seen rows left out, -1 / -inf
    padding.  ``scores``: [n, n_items] exact values; ``seen``: per row an array of item ids (or None)."""
    n, n_items = scores.shape
    out_i = np.full((n, k), -1, dtype=np.int64)
    out_s = np.full((n, k), -np.inf, dtype=np.float32)
    ids = np.arange(n_items)
    for r in range(n):
        ok = np.ones(n_items, dtype=bool)
        if seen is not None:
            ok[seen[r]] = False
        cand = ids[ok]
        order = cand[np.lexsort((cand, -scores[r, cand]))][:k]
        out_i[r, :len(order)] = order
        out_s[r, :len(order)] = scores[r, order]
    return out_i, out_s


def check_against_float64(items, scores, s64, seen, what=""):
    """The float-fixture check: per user, with tol = REL * max|s64[u, :]|,
    * returned ids are distinct, unseen and in range (k <= number of unseen items is the caller's business: a -1 is only
      accepted once every unseen item has been returned);
    * |score - s64[id]| <= tol;
    * the returned s64 sequence is non-increasing within 2 tol;
    * the smallest returned s64 is at least the largest s64 of the unseen items not returned, minus 2 tol.
    No user is left out and there is no outlier allowance."""
    n, n_items = s64.shape
    assert items.shape == scores.shape and items.shape[0] == n
    for r in range(n):
        tol = REL * np.abs(s64[r]).max()
        ok = np.ones(n_items, dtype=bool)
        if seen is not None:
            ok[seen[r]] = False
        got = items[r]
        n_got = int((got >= 0).sum())
        assert (got[:n_got] >= 0).all() and (got[n_got:] == -1).all(), (what, r, got)
        assert n_got == min(len(got), int(ok.sum())), (what, r, n_got, int(ok.sum()))
        assert np.isneginf(scores[r, n_got:]).all(), (what, r)
        ids = got[:n_got]
        assert (ids < n_items).all() and len(np.unique(ids)) == n_got and ok[ids].all(), (what, r, ids)
        ref = s64[r, ids]
        err = np.abs(scores[r, :n_got].astype(np.float64) - ref)
        assert (err <= tol).all(), (what, r, float(err.max()), tol)
        assert (np.diff(ref) <= 2 * tol).all(), (what, r, float(np.diff(ref).max(initial=0.0)), tol)
        ok[ids] = False
        if ok.any() and n_got:
            assert ref.min() >= s64[r, ok].max() - 2 * tol, (what, r, float(ref.min()), float(s64[r, ok].max()), tol)
