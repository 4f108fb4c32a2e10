"""ORACLE (test infrastructure -- never imported by the product path).

numpy restatement of the LCFN training step for any ``layer`` and for ``train_filters``.  Runs in fp32, or in fp64 inside
``helpers.float64_oracle(lcfn_numpy)`` (the working precision is the module global ``F32``).

Reference lines (relative to beta_rec/models/lcfn.py):
    :28-48     the filters (torch.normal(1, 0.001)) and transformers (numpy: N(0, 0.001) + diag N(1, 0.001)): plain
               tensors, no parameters
    :55-87     LCFN.forward: X_k = sigmoid((P diag(f_k)) (P^T X_{k-1}) W_k) per side, all-embeddings = cat(X_0 .. X_L)
               (the reference reads ``.weight`` of a tensor for k >= 2 and raises; here layer k feeds on layer k - 1)
    :171-205   loss_comput: -mean logsigmoid(pos - neg) + lamda * (the three batch norms + the norms of every filter and
               transformer), unsquared
    :115-152   train_single_batch: backward, optimizer step over the two tables
Pinned against golden vectors captured from the real reference (tests/golden/lcfn_*.npz); see
tests/test_oracle_golden_lcfn.py.

``w`` is ONE dict: the reference's two state_dict keys and the tail ``user_filters.k`` / ``item_filters.k`` /
``transformers.k`` (k = 0 .. L - 1).  ``bases`` = ``(P, Q)``.  ``hp`` = dict(L, lamda).  ``defect``: one of DEFECTS, a
deliberately wrong step (tests/test_lcfn_host.py); ``tile`` = (row tile, frequency granule, column granule) the
tail-dropping defects cut at.
"""
import numpy as np

from oracle.mf_numpy import new_opt_state, opt_step  # noqa: F401  (shared optimizer arithmetic)

F32 = np.float32
KEYS = ("user_embeddings.weight", "item_embeddings.weight")
DEFECTS = ("no_filter", "w_transposed", "no_sigmoid_derivative", "no_hop_gradient", "squared_norms", "reg_deduplicated",
           "dw_user_only", "tile_tail_rows", "freq_tail", "dim_tail")
TILE = (32, 4, 16)


def tail_keys(L):
    return tuple(f"{n}.{k}" for n in ("user_filters", "item_filters", "transformers") for k in range(L))


def all_keys(L):
    return KEYS + tail_keys(L)


def init_tail(P, Q, D, L, rng):
    """Filters and transformers with the reference's distributions (not its draws: those come from torch / numpy's
    global generators and are held by the goldens)."""
    out = {}
    for k in range(L):
        out[f"user_filters.{k}"] = rng.normal(1, 0.001, P.shape[1]).astype(np.float32)
        out[f"item_filters.{k}"] = rng.normal(1, 0.001, Q.shape[1]).astype(np.float32)
        out[f"transformers.{k}"] = (rng.normal(0, 0.001, (D, D)) + np.diag(rng.normal(1, 0.001, D))).astype(np.float32)
    return out


def _sigmoid(x):
    return (1.0 / (1.0 + np.exp(-x))).astype(F32)


def _softplus(x):
    """log(1 + exp(x)), stable."""
    return (np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))).astype(F32)


def _cut(T, defect, tile):
    """The [F, D] partial with the tail a defective kernel would drop."""
    if defect == "freq_tail" and T.shape[0] % tile[1]:
        T = T.copy()
        T[T.shape[0] - T.shape[0] % tile[1]:] = 0
    if defect == "dim_tail" and T.shape[1] % tile[2]:
        T = T.copy()
        T[:, T.shape[1] - T.shape[1] % tile[2]:] = 0
    return T


def _project(B, X, defect, tile):
    if defect == "tile_tail_rows" and B.shape[0] % tile[0]:
        n = B.shape[0] - B.shape[0] % tile[0]
        return _cut((B[:n].T @ X[:n]).astype(F32), defect, tile)
    return _cut((B.T @ X).astype(F32), defect, tile)


def _forward_side(E, B, filters, trans, defect, tile):
    """``(hops [X_0 .. X_L], T [T_1 .. T_L])`` of one side."""
    hops, Ts = [E.astype(F32)], []
    for f, W in zip(filters, trans):
        T = _project(B, hops[-1], defect, tile)
        A = T if defect == "no_filter" else (f[:, None] * T).astype(F32)
        M = (A @ (W.T if defect == "w_transposed" else W)).astype(F32)
        hops.append(_sigmoid((B @ M).astype(F32)))
        Ts.append(T)
    return hops, Ts


def _backward_side(G, hops, Ts, B, filters, trans, defect, tile):
    """From G = [G_0 .. G_L]: ``(dE, df [L], dW [L])`` of one side."""
    L = len(filters)
    dX, df, dW = G[L], [None] * L, [None] * L
    for k in range(L, 0, -1):
        f, W, X = filters[k - 1], trans[k - 1], hops[k]
        dZ = dX if defect == "no_sigmoid_derivative" else (dX * X * (1 - X)).astype(F32)
        dM = _project(B, dZ, defect, tile)
        dA = (dM @ (W if defect == "w_transposed" else W.T)).astype(F32)
        fdA = dA if defect == "no_filter" else (f[:, None] * dA).astype(F32)
        back = (B @ fdA).astype(F32)
        dX = back if defect == "no_hop_gradient" else (G[k - 1] + back).astype(F32)
        A = Ts[k - 1] if defect == "no_filter" else (f[:, None] * Ts[k - 1]).astype(F32)
        dW[k - 1] = (A.T @ dM).astype(F32)
        df[k - 1] = (dA * Ts[k - 1]).sum(1).astype(F32)
    return dX, df, dW


def _tail(w, L):
    cast = lambda n: [np.asarray(w[f"{n}.{k}"]).astype(F32) for k in range(L)]  # noqa: E731
    return cast("user_filters"), cast("item_filters"), cast("transformers")


def _norm(x):
    return F32(np.sqrt((x.astype(F32) ** 2).sum(dtype=F32)))


def lcfn_all_embeddings(w, bases, hp, defect=None, tile=TILE):
    """``(U_all [n_users, (L + 1) D], I_all)`` (lcfn.py:74, :87)."""
    fu, fi, tr = _tail(w, hp["L"])
    hu, _ = _forward_side(np.asarray(w[KEYS[0]]), np.asarray(bases[0]).astype(F32), fu, tr, defect, tile)
    hi, _ = _forward_side(np.asarray(w[KEYS[1]]), np.asarray(bases[1]).astype(F32), fi, tr, defect, tile)
    return np.concatenate(hu, 1), np.concatenate(hi, 1)


def lcfn_predict(w, bases, hp, users, items):
    ua, ia = lcfn_all_embeddings(w, bases, hp)
    return (ua[np.asarray(users)] * ia[np.asarray(items)]).sum(1)


def lcfn_grads(w, bases, hp, batch, defect=None, train_filters=False, tile=TILE):
    """One forward + backward: ``((bpr, reg), loss, grads)``; ``grads`` holds the two tables, and the tail keys when
    ``train_filters``."""
    L, lam = hp["L"], F32(hp["lamda"])
    P, Q = (np.asarray(b).astype(F32) for b in bases)
    Eu, Ei = np.asarray(w[KEYS[0]]).astype(F32), np.asarray(w[KEYS[1]]).astype(F32)
    fu, fi, tr = _tail(w, L)
    D = Eu.shape[1]
    users, pos, neg = (np.asarray(b, dtype=np.int64) for b in batch)
    B = users.size
    hu, Tu = _forward_side(Eu, P, fu, tr, defect, tile)
    hi, Ti = _forward_side(Ei, Q, fi, tr, defect, tile)
    ua, ia = np.concatenate(hu, 1), np.concatenate(hi, 1)
    x = (ua[users] * (ia[pos] - ia[neg])).sum(1).astype(F32)
    bpr = F32(_softplus(-x).mean(dtype=F32))
    sig = (1.0 / (1.0 + np.exp(x))).astype(F32)             # sigmoid(-x)
    gx = (-sig / F32(B)).astype(F32)
    Gu, Gi = np.zeros_like(ua), np.zeros_like(ia)
    np.add.at(Gu, users, gx[:, None] * (ia[pos] - ia[neg]))
    np.add.at(Gi, pos, gx[:, None] * ua[users])
    np.add.at(Gi, neg, -gx[:, None] * ua[users])
    # the regulariser: norms of whole gathered batch matrices (a repeated row counts as often as it occurs)
    dEu, dEi = np.zeros_like(Eu), np.zeros_like(Ei)
    reg = F32(0)
    for table, grad, idx in ((Eu, dEu, users), (Ei, dEi, pos), (Ei, dEi, neg)):
        if defect == "reg_deduplicated":
            idx = np.unique(idx)
        rows = table[idx]
        if defect == "squared_norms":
            reg += F32((rows ** 2).sum(dtype=F32))
            np.add.at(grad, idx, (lam * 2 * rows).astype(F32))
            continue
        nrm = _norm(rows)
        reg += nrm
        if nrm > 0:                  # not kept: the reference writes x / 0 = NaN into the tables
            np.add.at(grad, idx, (lam * rows / nrm).astype(F32))
    tail_norm = {}
    for k in range(L):
        for name, x_ in (("user_filters", fu[k]), ("item_filters", fi[k]), ("transformers", tr[k])):
            tail_norm[f"{name}.{k}"] = F32((x_ ** 2).sum(dtype=F32)) if defect == "squared_norms" else _norm(x_)
            reg += tail_norm[f"{name}.{k}"]
    reg = F32(lam * reg)
    split = lambda G: [G[:, k * D:(k + 1) * D] for k in range(L + 1)]  # noqa: E731
    du, dfu, dWu = _backward_side(split(Gu), hu, Tu, P, fu, tr, defect, tile)
    di, dfi, dWi = _backward_side(split(Gi), hi, Ti, Q, fi, tr, defect, tile)
    grads = {KEYS[0]: (dEu + du).astype(F32), KEYS[1]: (dEi + di).astype(F32)}
    if train_filters:
        for k in range(L):
            for name, x_, d in (("user_filters", fu[k], dfu[k]), ("item_filters", fi[k], dfi[k]),
                                ("transformers", tr[k], dWu[k] if defect == "dw_user_only" else dWu[k] + dWi[k])):
                nrm = tail_norm[f"{name}.{k}"]
                r = 2 * x_ if defect == "squared_norms" else (x_ / nrm if nrm > 0 else 0 * x_)
                grads[f"{name}.{k}"] = (d + lam * r).astype(F32)
    return (float(bpr), float(reg)), float(F32(bpr + reg)), grads


def trained(w, L, train_filters):
    """The sub-dict of ``w`` the optimizer moves (views of the same arrays)."""
    return {k: w[k] for k in (all_keys(L) if train_filters else KEYS)}


def lcfn_train_step(w, st, bases, hp, batch, opt, lr, train_filters=False):
    """One optimizer step in place; ``st`` is the optimizer state over ``trained(w, ...)``."""
    parts, loss, grads = lcfn_grads(w, bases, hp, batch, train_filters=train_filters)
    sub = trained(w, hp["L"], train_filters)
    opt_step(sub, grads, st, opt, lr)
    w.update(sub)
    return loss, parts, grads
