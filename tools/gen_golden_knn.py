"""ORACLE tooling (test infrastructure): capture the ItemKNN / UserKNN golden vectors from the REAL reference.

Runs only where the reference tree exists (REFERENCE_ROOT, default: where oracle/gen_golden.py looks); the reference
itself never travels -- only the small .npz fixtures written to tests/golden/knn_*.npz do.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_knn.py

Imports ``beta_rec.models.itemKNN`` / ``userKNN`` with the shims of tools/gen_golden_ultragcn.py.  Two kinds of record:

* the reference's own building blocks (``prepare_model``, ``generate_item_sim_matrix``, ``similarity_with_users``,
  ``top_k``, ``get_sparse_vector``, and ItemKNN's row-adding loop) driven with the user's REAL items -- what the mirror
  is held to;
* the reference's actual, unmodified ``predict`` output (``raw_*``), whose sequence is ``getrow(u).nonzero()[0]``: the
  row coordinate of a one-row matrix.  tests/test_oracle_golden_knn.py reproduces it with the restatement's
  ``sequence="row_coordinate"`` switch, which pins that reading of the defect.

``untied[u]``: the k-th and (k+1)-th largest sim of user u differ, or the k-th is zero -- only then do the reference's
``argpartition`` neighbours (those with a non-zero sim) have a defined answer.
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_ultragcn as gu  # noqa: E402  (the shims and REFERENCE_ROOT)


class RealSequence:
    """The reference's ``binary_user_item`` with ``getrow(u).nonzero()[0]`` yielding the user's items: lets the
    reference's own ItemKNN.predict loop run on the sequence its building blocks are written for."""

    def __init__(self, matrix):
        self._m = matrix

    def getrow(self, u):
        cols = self._m.getrow(u).nonzero()[1]
        return types.SimpleNamespace(nonzero=lambda: (cols, cols))

    def __getattr__(self, name):
        return getattr(self._m, name)


def frame(rng, U, I, density, empty_user, empty_item, n_dup):
    m = rng.random((U, I)) < density
    if empty_user is not None:
        m[empty_user] = False
    if empty_item is not None:
        m[:, empty_item] = False
    u, i = np.nonzero(m)
    u, i = np.concatenate([u, u[:n_dup]]), np.concatenate([i, i[:n_dup]])     # duplicated pairs: multiplicity 2
    perm = rng.permutation(len(u))
    return u[perm].astype(np.int64), i[perm].astype(np.int64)


def fixture(name, U, I, k, seed, density=0.15, empty_user=4, empty_item=7, n_dup=3, min_untied=10):
    import pandas as pd
    from beta_rec.models import itemKNN as ri
    from beta_rec.models import userKNN as ru

    rng = np.random.default_rng(seed)
    users, items = frame(rng, U, I, density, empty_user, empty_item, n_dup)
    data = types.SimpleNamespace(train=pd.DataFrame({"col_user": users, "col_item": items}))
    cfg = {"device_str": "cpu", "n_users": U, "n_items": I, "neighbourhood_size": k}
    k_eff = min(k, U)                       # the reference raises for k > n_users; the mirror clamps

    mi = ri.ItemKNN(cfg)
    mi.prepare_model(data)                  # generate_item_sim_matrix
    mu = ru.UserKNN(cfg)
    mu.prepare_model(data)
    B = mu.binary_user_item
    nnz = np.asarray([B.getrow(u).nnz for u in range(U)])
    out = {"meta": np.array([U, I, k, seed], dtype=np.int64), "users": users, "items": items,
           "S": mi.item_sim_matrix.copy(), "cnt": mi._users_count_per_item().copy(),
           "cu": mu._items_count_per_user().copy()}

    # --- the building blocks on the REAL sequence
    nb_ids = np.full((U, k_eff), -1, dtype=np.int64)
    nb_sims = np.zeros((U, k_eff), dtype=np.float64)
    sims = np.zeros((U, U), dtype=np.float64)
    user_rows = np.zeros((U, I), dtype=np.float64)
    untied = np.zeros(U, dtype=bool)
    n_nonzero = np.zeros(U, dtype=np.int64)
    for u in range(U):
        seq = B.getrow(u).nonzero()[1]
        s = mu.similarity_with_users(seq)
        sims[u] = s
        nn = ru.top_k(s, k_eff)
        nb_ids[u], nb_sims[u] = nn, s[nn]
        ni = ru.get_sparse_vector(nn, U, values=s[nn])
        row = B.T.dot(ni).toarray().ravel()
        row[seq] = -np.inf
        user_rows[u] = row
        o = np.sort(s)[::-1]
        untied[u] = k_eff >= U or o[k_eff - 1] != o[k_eff] or o[k_eff - 1] == 0
        n_nonzero[u] = int((s != 0).sum())
    out.update(sims=sims, nb_ids=nb_ids, nb_sims=nb_sims, user_rows=user_rows, untied=untied)

    item_rows = np.zeros((U, I), dtype=np.float32)
    item_rows_valid = nnz > 0               # (the reference's loop reads a stale variable for a user without rows)
    mi_real = ri.ItemKNN(cfg)
    mi_real.binary_user_item = RealSequence(mi.binary_user_item)
    mi_real.item_sim_matrix = mi.item_sim_matrix
    for u in np.nonzero(item_rows_valid)[0]:
        item_rows[u] = mi_real.predict([int(u)] * I, list(range(I))).numpy()
    out.update(item_rows=item_rows, item_rows_valid=item_rows_valid)

    # --- the reference's actual predict, untouched
    if k <= U:
        qs = np.nonzero(nnz > 0)[0]
        raw_users = np.repeat(qs, 3)
        raw_items = rng.integers(0, I, len(raw_users))
        raw_items[::3] = 0                   # item 0 is where the defect puts its -inf
        out["raw_users"], out["raw_items"] = raw_users.astype(np.int64), raw_items.astype(np.int64)
        ru_pred = mu.predict(list(raw_users), list(raw_items))
        ri_pred = mi.predict(list(raw_users), list(raw_items))
        assert str(ru_pred.dtype) == "torch.float64" and str(ri_pred.dtype) == "torch.float32"
        out["raw_user_predict"], out["raw_item_predict"] = ru_pred.numpy().copy(), ri_pred.numpy().copy()

    n_untied = int(untied.sum())
    fewer = int((untied & (n_nonzero < k_eff)).sum())
    more = int((untied & (n_nonzero > k_eff)).sum())
    assert n_untied >= min_untied, f"{name}: only {n_untied} untied users"
    if k <= U:
        assert fewer >= 1 and more >= 1, f"{name}: untied users with fewer / more than k non-zero sims: {fewer} / {more}"
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {U} x {I}, {len(users)} rows, k {k}: {n_untied} of {U} users untied ({fewer} with fewer than k "
          f"non-zero sims, {more} with more), max multiplicity {int(B.max())}, {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    gu.import_reference()
    fixture("knn_k3", 37, 29, 3, seed=3)
    fixture("knn_k5", 37, 29, 5, seed=3)
    fixture("knn_k8", 37, 29, 8, seed=5)
    # neighbourhood_size beyond n_users: the reference raises, the mirror clamps to every user
    # (no user can have more than k non-zero sims there, so that half of the assertion does not apply)
    fixture("knn_kbig", 12, 9, 16, seed=11, density=0.3, empty_user=2, empty_item=None, n_dup=2)


if __name__ == "__main__":
    main()
