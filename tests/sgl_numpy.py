"""ORACLE (test infrastructure -- never imported by the product path).

numpy restatement of the SGL training step.  Runs in fp32, or in fp64 inside ``helpers.float64_oracle(sgl_numpy)`` (the
working precision is the module global ``F32``).

Reference lines (relative to beta_rec/models/sgl.py):
    :464-527   create_sgl_mat: keep int(n (1 - ratio)) interactions, symmetrise, D^-1/2 A D^-1/2 in fp32
    :545-580   sub_mat_refresher: view 1 then view 2 (per layer for aug_type 2) -- the order of the np.random.choice calls
    :277-356   SGL.forward: three propagations of L hops, each mean-pooled over L + 1 hops
    :82-145    calc_ssl_loss_v2: InfoNCE of the batch's view-1 rows against every view-2 row of their side
    :188-226   create_bpr_loss: BPR SUM + regs / 2 * squares of the batch's hop-0 rows
    :423-445   train_single_batch: loss = the sum of the three, backward, optimizer step
Pinned against golden vectors captured from the real reference (tests/golden/sgl_*.npz); see
tests/test_oracle_golden_sgl.py.

Parameters are a dict with the reference's state_dict keys.  ``graph`` = ``(rows, cols, vals, N)``: the COO entries of
norm_adj.  ``subs`` = ``[view][layer]`` dense ``[N, N]`` matrices (or None with ``pretrain``).  ``hp`` = dict(L, regs,
ssl_reg, ssl_temp, ssl_mode, pretrain).  ``defect``: one of DEFECTS, a deliberately wrong step (tests/test_sgl_host.py).
"""
import numpy as np

from oracle.mf_numpy import new_opt_state, opt_step  # noqa: F401  (shared optimizer arithmetic)

F32 = np.float32
KEYS = ("user_embedding", "item_embedding")
DEFECTS = ("no_onehot", "views_swapped", "deduplicated", "bpr_mean", "hop0_unscaled")


# ---- sub-graphs ------------------------------------------------------------------------------------------------------
def keep_sets(n_inter, n_users, n_items, aug_type, ssl_ratio, n_layers, is_subgraph=True):
    """The reference's draws of ONE sub_mat_refresher call from the global numpy generator, in its order:
    ``keep[view][layer]`` = 0/1 over the interactions (aug_type 1, 2), a pair of 0/1 node arrays (aug_type 0, with
    int(n * ratio) dropped nodes per side) or None (nothing is dropped: no draw)."""
    L = max(n_layers, 1)
    out = [[None] * L for _ in range(2)]
    calls = [(v, l) for l in range(n_layers if aug_type == 2 else 1) for v in range(2)]
    for v, l in calls:
        if not (is_subgraph and ssl_ratio > 0):
            drawn = None
        elif aug_type == 0:
            drawn = []
            for n in (n_users, n_items):
                keep = np.ones(n, dtype=np.uint8)
                keep[np.random.choice(np.arange(n), size=int(n * ssl_ratio), replace=False)] = 0
                drawn.append(keep)
            drawn = tuple(drawn)
        else:
            drawn = np.zeros(n_inter, dtype=np.uint8)
            drawn[np.random.choice(np.arange(n_inter), size=int(n_inter * (1 - ssl_ratio)), replace=False)] = 1
        for ll in (range(L) if aug_type != 2 else (l,)):
            out[v][ll] = drawn
    return out


def sub_matrix(users, items, n_users, n_items, keep):
    """Dense ``[N, N]`` D^-1/2 A D^-1/2 of the kept interactions (sgl.py:513-527): d = deg^-1/2 in the working
    precision (0 for an isolated node), value = (d_r * 1) * d_c."""
    users, items = np.asarray(users), np.asarray(items)
    if keep is None:
        on = np.ones(users.size, dtype=bool)
    elif isinstance(keep, tuple):
        on = (keep[0][users] != 0) & (keep[1][items] != 0)
    else:
        on = np.asarray(keep) != 0
    N = n_users + n_items
    A = np.zeros((N, N), dtype=F32)
    A[users[on], n_users + items[on]] = 1
    A = A + A.T
    deg = A.sum(axis=1)
    with np.errstate(divide="ignore"):
        d = np.power(deg, F32(-0.5)).astype(F32)
    d[np.isinf(d)] = 0
    return ((d[:, None] * A).astype(F32) * d[None, :]).astype(F32)


def dense_adj(graph):
    rows, cols, vals, N = graph
    A = np.zeros((N, N), dtype=F32)
    np.add.at(A, (np.asarray(rows), np.asarray(cols)), np.asarray(vals, dtype=F32))
    return A


# ---- the step --------------------------------------------------------------------------------------------------------
def pooled(E0, mats, defect=None):
    """Mean over the L + 1 hops of E_l = M_l E_{l-1}."""
    E = [E0]
    for M in mats:
        E.append((M @ E[-1]).astype(F32))
    H = F32(len(E))
    if defect == "hop0_unscaled":
        return (E[0] + sum(E[1:], np.zeros_like(E0)) / H).astype(F32)
    return (sum(E[1:], E[0]) / H).astype(F32)


def pooled_backward(dP, mats, defect=None):
    """dE_0 of ``pooled``: dP / (L + 1) enters at every hop, dE_{l-1} += M_l^T dE_l."""
    H = F32(len(mats) + 1)
    d = (dP / H).astype(F32)
    t = d
    for l in range(len(mats) - 1, -1, -1):
        t = (mats[l].T @ t).astype(F32)
        t = (t + (dP if (l == 0 and defect == "hop0_unscaled") else d)).astype(F32)
    if not mats and defect == "hop0_unscaled":
        return dP
    return t


def _normalize(X):
    nrm = np.sqrt((X * X).sum(axis=1, keepdims=True)).astype(F32)
    return (X / nrm).astype(F32), nrm


def _normalize_backward(dXn, Xn, nrm):
    return ((dXn - Xn * (Xn * dXn).sum(axis=1, keepdims=True)) / nrm).astype(F32)


def sgl_grads(w, graph, subs, hp, batch, defect=None):
    """``(parts, loss, grads)``: parts = (bpr, emb, ssl), loss their sum, grads keyed like the weights."""
    users, pos, neg = (np.asarray(a, dtype=np.int64).reshape(-1) for a in batch)
    U = w["user_embedding"].shape[0]
    L = hp["L"]
    E0 = np.concatenate([w["user_embedding"], w["item_embedding"]], axis=0).astype(F32)
    A = dense_adj(graph)
    main = [A] * L
    P0 = pooled(E0, main, defect)
    # BPR sum + regs (sgl.py:204-224), softplus in its stable form
    u, p, n = P0[users], P0[U + pos], P0[U + neg]
    x = (u * (p - n)).sum(axis=1).astype(F32)
    soft = (np.log1p(np.exp(-np.abs(x))) + np.maximum(-x, 0)).astype(F32)
    sig = (1 / (1 + np.exp(x))).astype(F32)                       # sigmoid(-x) = -d softplus(-x) / dx
    bpr = soft.mean() if defect == "bpr_mean" else soft.sum()
    gx = (-sig / F32(x.size if defect == "bpr_mean" else 1)).astype(F32)
    dP0 = np.zeros_like(P0)
    np.add.at(dP0, users, gx[:, None] * (p - n))
    np.add.at(dP0, U + pos, gx[:, None] * u)
    np.add.at(dP0, U + neg, -gx[:, None] * u)
    rows0 = np.concatenate([users, U + pos, U + neg])
    emb = F32(hp["regs"]) * F32(0.5) * (E0[rows0] ** 2).sum()
    g = np.zeros_like(E0)
    np.add.at(g, rows0, F32(hp["regs"]) * E0[rows0])
    g = (g + pooled_backward(dP0, main, defect)).astype(F32)
    ssl = F32(0)
    if not hp.get("pretrain"):
        P = [pooled(E0, subs[v][:L], defect) for v in range(2)]
        Xn, nrm = zip(*[_normalize(P[v]) for v in range(2)])
        dXn = [np.zeros_like(E0), np.zeros_like(E0)]
        q_view, k_view = (1, 0) if defect == "views_swapped" else (0, 1)
        T = F32(hp["ssl_temp"])
        c = F32(hp["ssl_reg"]) / T
        sides = []
        if hp["ssl_mode"] in ("user_side", "both_side"):
            sides.append((users, 0, U))
        if hp["ssl_mode"] in ("item_side", "both_side"):
            sides.append((pos, U, E0.shape[0] - U))
        for idx, off, cnt in sides:
            if defect == "deduplicated":
                idx = np.unique(idx)
            K = Xn[k_view][off:off + cnt]
            Q = Xn[q_view][off + idx]
            Z = ((Q @ K.T - 1) / T).astype(F32)                   # cosines are <= 1: the shift 1 / T is exact
            ez = np.exp(Z)
            tot = ez.sum(axis=1)
            pos_z = (((Q * K[idx]).sum(axis=1) - 1) / T).astype(F32)
            ssl = ssl + F32(hp["ssl_reg"]) * (np.log(tot) - pos_z).sum()
            G = (ez / tot[:, None]).astype(F32)
            if defect != "no_onehot":
                G[np.arange(idx.size), idx] -= 1
            G = (G * c).astype(F32)
            np.add.at(dXn[q_view], off + idx, (G @ K).astype(F32))
            dXn[k_view][off:off + cnt] += (G.T @ Q).astype(F32)
        for v in range(2):
            dP = _normalize_backward(dXn[v], Xn[v], nrm[v])
            g = (g + pooled_backward(dP, subs[v][:L], defect)).astype(F32)
    parts = (float(bpr), float(emb), float(ssl))
    loss = float(F32(bpr) + F32(emb) + F32(ssl))
    return parts, loss, {"user_embedding": g[:U], "item_embedding": g[U:]}


def sgl_train_step(w, st, graph, subs, hp, batch, opt, lr):
    parts, loss, grads = sgl_grads(w, graph, subs, hp, batch)
    opt_step(w, grads, st, opt, lr)
    return parts, loss


def sgl_factors(w, graph, hp):
    """The mean-pooled main view, split: predict is the dot product of a user row and an item row (sgl.py:396-405)."""
    U = w["user_embedding"].shape[0]
    E0 = np.concatenate([w["user_embedding"], w["item_embedding"]], axis=0).astype(F32)
    P = pooled(E0, [dense_adj(graph)] * hp["L"])
    return P[:U], P[U:]


def sgl_predict(w, graph, hp, users, items):
    fu, fi = sgl_factors(w, graph, hp)
    return (fu[np.asarray(users)] * fi[np.asarray(items)]).sum(axis=1)
