"""ORACLE (test infrastructure -- never imported by the product path).

numpy restatement of the SimGCL training step.  Runs in fp32, or in fp64 inside ``helpers.float64_oracle(simgcl_numpy)``
(the working precision is the module global ``F32``).

Reference lines (relative to beta_rec/models/simgcl.py):
    :25-47     SimGCL.forward: Y_k = A X_{k-1}; perturbed: X_k = Y_k + sign(Y_k) * normalize(rand_like(Y_k)) * eps; the
               output is the mean of X_1 .. X_L (hop 0 is not in it), and the perturbed X_k feeds hop k + 1
    :49-55     infoNCE: -log(exp(pos / T) / sum_j exp(s_ij / T)) summed over rows, the positive inside the total
    :57-70     cal_cl_loss: unique users / unique positive items, view 1 then view 2 (fresh noise each), T = 0.2;
               :65 ``user_view_2 = normalize(user_view_1)``: the user side contrasts view 1 with itself
    :72-82     predict: dot product of the RAW table rows
    :101-133   train_single_batch: bpr + reg * (|u_b| + |p_b| + |n_b|) + lambda * cl on the CLEAN pooled rows
    :153-157   bpr_loss: -log(10e-8 + sigmoid(pos - neg)).sum() -- 10e-8 is 1e-7
    :159-163   l2_reg_loss: unsquared Frobenius norms (torch.norm(emb, p=2) of a matrix), duplicates count
Pinned against golden vectors captured from the real reference (tests/golden/simgcl_*.npz); see
tests/test_oracle_golden_simgcl.py.

Parameters are a dict with the reference's state_dict keys.  ``graph`` = ``(rows, cols, vals, N)``: the COO entries of
norm_adj.  ``hp`` = dict(L, eps, reg, lam, temp, user_view).  ``noise`` = ``[2, L, N, D]`` uniforms (view, hop, row,
column).  ``defect``: one of DEFECTS, a deliberately wrong step (tests/test_simgcl_host.py).

``device_uniforms`` restates the device draw of csrc/simgcl.hip (sim_uniform) bit for bit; ``settle_noise`` is the rule
that makes a fixture independent of the sign of near-zero elements.
"""
import numpy as np

from oracle.mf_numpy import new_opt_state, opt_step  # noqa: F401  (shared optimizer arithmetic)

F32 = np.float32
KEYS = ("user_embedding.weight", "item_embedding.weight")
DEFECTS = ("no_sign", "noise_unnormalised", "noise_not_carried", "hop0_in_mean", "divisor_l_plus_1", "same_noise",
           "duplicates_kept", "user_view2", "cl_unscaled", "wrong_temp", "reg_hop0", "reg_squared", "no_1e7")
MAX_LAYERS = 4           # HIPREC_SIMGCL_MAX_LAYERS: the stride of (view, hop) in the draw's key
FRAGILE = 1e-4           # an element with 0 < |y| < FRAGILE * max|Y_k| gets no noise in a fixture
ZEROED_CAP = 0.01        # ... and a fixture with more than this share of such elements is rejected


# ---- the device draw -------------------------------------------------------------------------------------------------
def device_uniforms(seed, step, L, n, D):
    """``[2, L, n, D]`` fp32: sim_uniform(seed, step, view, hop, row * D + col) of csrc/simgcl.hip, bit for bit."""
    e = np.arange(n * D, dtype=np.uint64) + np.uint64(1)
    out = np.empty((2, L, n * D), dtype=np.float32)
    one = np.ones(1, dtype=np.uint64)
    base = (one * np.uint64(seed % (1 << 64))) + np.uint64(0xD1B54A32D192ED03) * (one * np.uint64(step) + one)
    for view in range(2):
        for hop in range(L):
            z = base + np.uint64(0x9E3779B97F4A7C15) * e + np.uint64(0x8CB92BA72F3D8DD7) * (
                one * np.uint64(view * MAX_LAYERS + hop + 1))
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
            out[view, hop] = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return out.reshape(2, L, n, D)


# ---- the forward -----------------------------------------------------------------------------------------------------
def dense_adj(graph):
    rows, cols, vals, N = graph
    A = np.zeros((N, N), dtype=F32)
    np.add.at(A, (np.asarray(rows), np.asarray(cols)), np.asarray(vals, dtype=F32))
    return A


def perturb(Y, u, eps, defect=None):
    """simgcl.py:35-40: Y + sign(Y) * u / max(|u|, 1e-12) * eps."""
    u = np.asarray(u, dtype=F32)
    if defect != "noise_unnormalised":
        u = (u / np.maximum(np.sqrt((u * u).sum(axis=1, keepdims=True)), F32(1e-12))).astype(F32)
    sg = np.ones_like(Y) if defect == "no_sign" else np.sign(Y).astype(F32)
    return (Y + sg * u * F32(eps)).astype(F32)


def fragile_mask(Y):
    """Elements whose sign another summation order could flip: 0 < |y| < FRAGILE * max|Y|."""
    a = np.abs(Y)
    return (a > 0) & (a < FRAGILE * a.max())


def settle_noise(E0, A, L, eps, noise_view):
    """One view's ``[L, n, D]`` uniforms with the fragile elements zeroed, hop by hop (hop k + 1 depends on hop k's
    noise): ``(settled copy, share zeroed)``.  Always evaluated in fp32, as the reference's forward is."""
    out = np.array(noise_view, dtype=np.float32, copy=True)
    X = np.asarray(E0, dtype=np.float32)
    A = np.asarray(A, dtype=np.float32)
    zeroed = 0
    for k in range(L):
        Y = (A @ X).astype(np.float32)
        m = fragile_mask(Y)
        zeroed += int((m & (out[k] != 0)).sum())
        out[k][m] = 0
        u = out[k] / np.maximum(np.sqrt((out[k] * out[k]).sum(axis=1, keepdims=True)), np.float32(1e-12))
        X = (Y + np.sign(Y) * u * np.float32(eps)).astype(np.float32)
    return out, zeroed / max(out.size, 1)


def pooled(E0, A, L, eps=0.0, noise_view=None, defect=None):
    """simgcl.py:25-47: mean over hops 1 .. L; ``noise_view`` None = the clean forward."""
    X, hops = E0, []
    for k in range(L):
        Y = (A @ X).astype(F32)
        Xk = Y if noise_view is None else perturb(Y, noise_view[k], eps, defect)
        hops.append(Xk)
        X = Y if defect == "noise_not_carried" else Xk
    total = sum(hops[1:], hops[0])
    if defect == "hop0_in_mean":
        return ((total + E0) / F32(L + 1)).astype(F32)
    return (total / F32(L + 1 if defect == "divisor_l_plus_1" else L)).astype(F32)


def pooled_backward(dP, A, L, defect=None):
    """dE_0 of ``pooled``: sign() has no derivative, so every view is E_0 -> (1 / L) sum_k A^k E_0 + const."""
    div = F32(L + 1 if defect in ("hop0_in_mean", "divisor_l_plus_1") else L)
    d = (dP / div).astype(F32)
    t = np.zeros_like(d)
    for _ in range(L):
        t = (A.T @ (t + d)).astype(F32)
    return (t + d).astype(F32) if defect == "hop0_in_mean" else t


def _normalize(X):
    nrm = np.maximum(np.sqrt((X * X).sum(axis=1, keepdims=True)), F32(1e-12)).astype(F32)
    return (X / nrm).astype(F32), nrm


def _normalize_backward(dXn, Xn, nrm):
    return ((dXn - Xn * (Xn * dXn).sum(axis=1, keepdims=True)) / nrm).astype(F32)


def simgcl_grads(w, graph, hp, batch, noise, defect=None):
    """``(parts, loss, grads)``: parts = (bpr, reg, cl_user, cl_item) -- the two InfoNCE sums before ``lambda`` --, loss =
    bpr + reg + lambda * (cl_user + cl_item), grads keyed like the weights."""
    users, pos, neg = (np.asarray(a, dtype=np.int64).reshape(-1) for a in batch)
    U = w[KEYS[0]].shape[0]
    L, eps = int(hp["L"]), hp["eps"]
    if L < 1:
        raise ValueError("n_layer < 1: the reference stacks nothing (simgcl.py:42)")
    E0 = np.concatenate([w[KEYS[0]], w[KEYS[1]]], axis=0).astype(F32)
    A = dense_adj(graph)
    noise = np.asarray(noise)
    P0 = pooled(E0, A, L, defect=defect)
    P = [pooled(E0, A, L, eps, noise[0], defect), pooled(E0, A, L, eps, noise[0 if defect == "same_noise" else 1], defect)]
    # BPR sum (simgcl.py:153-157)
    u, p, n = P0[users], P0[U + pos], P0[U + neg]
    x = (u * (p - n)).sum(axis=1).astype(F32)
    sig = (1 / (1 + np.exp(-x))).astype(F32)
    c = F32(0 if defect == "no_1e7" else 1e-7)
    with np.errstate(divide="ignore", invalid="ignore"):
        bpr = (-np.log(c + sig)).sum()
        gx = (-(sig * (1 - sig)) / (c + sig)).astype(F32)
    dP0 = np.zeros_like(P0)
    np.add.at(dP0, users, gx[:, None] * (p - n))
    np.add.at(dP0, U + pos, gx[:, None] * u)
    np.add.at(dP0, U + neg, -gx[:, None] * u)
    # reg * unsquared Frobenius norms of the three batch matrices of the clean POOLED rows (simgcl.py:159-163)
    g_direct = np.zeros_like(E0)
    src, dst = (E0, g_direct) if defect == "reg_hop0" else (P0, dP0)
    reg_loss = F32(0)
    for rows in (users, U + pos, U + neg):
        M = src[rows]
        sq = (M * M).sum()
        if defect == "reg_squared":
            reg_loss = reg_loss + F32(hp["reg"]) * sq
            np.add.at(dst, rows, F32(2 * hp["reg"]) * M)
        else:
            nrm = np.sqrt(sq).astype(F32)
            reg_loss = reg_loss + F32(hp["reg"]) * nrm
            if nrm > 0:                       # the mirror's recorded deviation: norm 0 -> gradient 0, not NaN
                np.add.at(dst, rows, (F32(hp["reg"]) / nrm) * M)
    # InfoNCE among the unique rows (simgcl.py:49-70)
    T = F32(hp.get("temp", 0.2) * (2.0 if defect == "wrong_temp" else 1.0))
    lam = F32(1.0 if defect == "cl_unscaled" else hp["lam"])
    Xn, nrm = zip(*[_normalize(P[v]) for v in range(2)])
    dXn = [np.zeros_like(E0), np.zeros_like(E0)]
    user_k = 1 if (hp.get("user_view", "reference") == "two_views") != (defect == "user_view2") else 0
    cl = []
    for idx, off, k_view in ((users, 0, user_k), (pos, U, 1)):
        if defect != "duplicates_kept":
            idx = np.unique(idx)
        Q, K = Xn[0][off + idx], Xn[k_view][off + idx]
        Z = ((Q @ K.T - 1) / T).astype(F32)                   # cosines are <= 1: the shift 1 / T is exact
        ez = np.exp(Z)
        tot = ez.sum(axis=1)
        pos_z = (((Q * K).sum(axis=1) - 1) / T).astype(F32)
        cl.append((np.log(tot) - pos_z).sum())
        G = (ez / tot[:, None]).astype(F32)
        G[np.arange(idx.size), np.arange(idx.size)] -= 1
        G = (G * (lam / T)).astype(F32)
        np.add.at(dXn[0], off + idx, (G @ K).astype(F32))
        np.add.at(dXn[k_view], off + idx, (G.T @ Q).astype(F32))
    dP = dP0
    for v in range(2):
        dP = (dP + _normalize_backward(dXn[v], Xn[v], nrm[v])).astype(F32)
    g = (g_direct + pooled_backward(dP, A, L, defect)).astype(F32)
    parts = (float(bpr), float(reg_loss), float(cl[0]), float(cl[1]))
    loss = float(F32(bpr) + F32(reg_loss) + lam * (F32(cl[0]) + F32(cl[1])))
    return parts, loss, {KEYS[0]: g[:U], KEYS[1]: g[U:]}


def simgcl_predict(w, users, items):
    """simgcl.py:72-82."""
    return (w[KEYS[0]][np.asarray(users)] * w[KEYS[1]][np.asarray(items)]).sum(axis=1)
