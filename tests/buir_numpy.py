"""ORACLE (test infrastructure -- never imported by the product path).

numpy restatement of the BUIR training step.  Runs in fp32, or in fp64 inside ``helpers.float64_oracle(buir_numpy)`` (the
working precision is the module global ``F32``).

Reference lines (relative to beta_rec/models/buir.py):
    :160-178   LGCN_Encoder.forward: E_k = A E_{k-1}; the output is the mean of E_0 .. E_L -- hop 0 IS in it
    :56-59     forward: x from the online encoder, t from the target encoder, ONE predictor for users and items
    :66-77     get_loss: F.normalize (v / max(|v|, 1e-12)) of all four; (2 - 2 y_u.t_i) + (2 - 2 y_i.t_u); the batch mean
    :41-46     _init_target: the target is a copy of the online encoder and takes no gradient
    :48-54     _update_target: t * m + o * (1 - m) -- defined, never called by the reference
    :79-100    predict: on the ONLINE encoder only: p(P[u]).P[U + i] + P[u].p(P[U + i])
    :215-233   train_single_batch: the negatives are unpacked and never used
Pinned against golden vectors captured from the real reference (tests/golden/buir_*.npz); see
tests/test_oracle_golden_buir.py.

Parameters are a dict with the reference's state_dict keys.  ``graph`` = ``(rows, cols, vals, N)``: the COO entries of
norm_adj.  ``defect``: one of DEFECTS, a deliberately wrong step (tests/test_buir_host.py).
"""
import numpy as np

from oracle import mf_numpy as _mf

F32 = np.float32
ONLINE = ("online_encoder.embedding_dict.user_emb", "online_encoder.embedding_dict.item_emb")
TARGET = ("target_encoder.embedding_dict.user_emb", "target_encoder.embedding_dict.item_emb")
PREDICTOR = ("predictor.weight", "predictor.bias")
KEYS = ONLINE[::-1] + TARGET[::-1] + PREDICTOR   # the reference's state_dict order: nn.ParameterDict sorts a dict's keys
TRAINABLE = ONLINE + PREDICTOR
DEFECTS = ("no_layer0", "divide_by_l", "two_predictors", "targets_swapped", "target_gradient", "predict_from_target",
           "no_clamp")
CLAMP = 1e-12


def dense_adj(graph):
    rows, cols, vals, N = graph
    A = np.zeros((N, N), dtype=F32)
    np.add.at(A, (np.asarray(rows), np.asarray(cols)), np.asarray(vals, dtype=F32))
    return A


def pooled(E0, A, L, defect=None):
    """buir.py:160-170: mean over hops 0 .. L."""
    X = np.asarray(E0, dtype=F32)
    total = np.zeros_like(X) if defect == "no_layer0" else X.copy()
    for _ in range(L):
        X = (A @ X).astype(F32)
        total = total + X
    return (total / F32(L if defect in ("no_layer0", "divide_by_l") else L + 1)).astype(F32)


def pooled_backward(dP, A, L, defect=None):
    """dE_0 of ``pooled``: (1 / (L + 1)) sum_{k = 0 .. L} (A^T)^k dP."""
    d = (dP / F32(L if defect in ("no_layer0", "divide_by_l") else L + 1)).astype(F32)
    if defect == "no_layer0":
        t = np.zeros_like(d)
        for _ in range(L):
            t = (A.T @ (t + d)).astype(F32)
        return t
    acc = d
    for _ in range(L):
        acc = (d + A.T @ acc).astype(F32)
    return acc


def _normalize(X, defect=None):
    """F.normalize: ``(X / den, |X|, den)`` with den = max(|X|, 1e-12)."""
    nrm = np.sqrt((X * X).sum(axis=1, keepdims=True)).astype(F32)
    den = nrm if defect == "no_clamp" else np.maximum(nrm, F32(CLAMP)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (X / den).astype(F32), nrm, den


RADIAL = True       # False: the radial term of the normalisation's backward is dropped (term_scale only)


def _normalize_backward(dXn, X, nrm, den):
    """autograd through v / clamp_min(|v|, 1e-12): below the clamp the denominator is a constant."""
    live = (nrm >= F32(CLAMP)) & RADIAL
    safe = np.where(nrm > 0, nrm, F32(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        through = np.where(live, X * ((dXn * X).sum(axis=1, keepdims=True) / (den * den * safe)), F32(0))
        return (dXn / den - through).astype(F32)


def tables(w, keys):
    return np.concatenate([w[keys[0]], w[keys[1]]], axis=0).astype(F32)


def buir_grads(w, graph, L, batch, defect=None):
    """``(loss, grads)`` of buir.py:215-233; grads carry every state_dict key, the target's being zero."""
    users, pos = (np.asarray(a, dtype=np.int64).reshape(-1) for a in batch[:2])
    U = w[ONLINE[0]].shape[0]
    B = users.size
    A = dense_adj(graph)
    W, b = w[PREDICTOR[0]].astype(F32), w[PREDICTOR[1]].astype(F32)
    W_i = W.T if defect == "two_predictors" else W          # a second predictor for the item side
    P_on, P_tg = pooled(tables(w, ONLINE), A, L, defect), pooled(tables(w, TARGET), A, L, defect)
    x_u, x_i, t_u, t_i = P_on[users], P_on[U + pos], P_tg[users], P_tg[U + pos]
    if defect == "targets_swapped":
        t_u, t_i = t_i, t_u
    y_u, y_i = (x_u @ W.T + b).astype(F32), (x_i @ W_i.T + b).astype(F32)
    (yn_u, nu, du), (yn_i, ni, di) = _normalize(y_u, defect), _normalize(y_i, defect)
    (tn_u, tnu, tdu), (tn_i, tni, tdi) = _normalize(t_u, defect), _normalize(t_i, defect)
    loss = ((F32(2) - F32(2) * (yn_u * tn_i).sum(axis=1)) + (F32(2) - F32(2) * (yn_i * tn_u).sum(axis=1))).mean()
    c = F32(-2.0 / B)
    dy_u = _normalize_backward(c * tn_i, y_u, nu, du)
    dy_i = _normalize_backward(c * tn_u, y_i, ni, di)
    dP = np.zeros_like(P_on)
    np.add.at(dP, users, (dy_u @ W).astype(F32))
    np.add.at(dP, U + pos, (dy_i @ W_i).astype(F32))
    g_on = pooled_backward(dP, A, L, defect)
    dW_i = (dy_i.T @ x_i).astype(F32)
    g = {ONLINE[0]: g_on[:U], ONLINE[1]: g_on[U:],
         PREDICTOR[0]: (dy_u.T @ x_u + (dW_i.T if defect == "two_predictors" else dW_i)).astype(F32),
         PREDICTOR[1]: (dy_u.sum(axis=0) + dy_i.sum(axis=0)).astype(F32)}
    dT = np.zeros_like(P_tg)
    if defect == "target_gradient":
        np.add.at(dT, U + pos, _normalize_backward(c * yn_u, t_i, tni, tdi))
        np.add.at(dT, users, _normalize_backward(c * yn_i, t_u, tnu, tdu))
        dT = pooled_backward(dT, A, L, defect)
    g[TARGET[0]], g[TARGET[1]] = dT[:U], dT[U:]
    return float(loss), g


def term_scale(w, graph, L, batch):
    """Per trained tensor, the scale of the TERMS its gradient sums: the gradient with the radial term of the
    normalisation's backward dropped.  d loss / d y = coef (n(t) - (n(y).n(t)) n(y)) is a difference of two vectors of
    length <= |coef|; for D = 1 they cancel exactly (n(y) = +-1 whatever y is) and an fp32 evaluation is left with its
    rounding error, which is relative to the terms."""
    global RADIAL
    RADIAL = False
    try:
        g = buir_grads(w, graph, L, batch)[1]
    finally:
        RADIAL = True
    return {k: float(np.abs(g[k]).max()) for k in TRAINABLE}


def buir_predict(w, graph, L, users, items, defect=None):
    """buir.py:79-100."""
    users, items = np.asarray(users, dtype=np.int64).reshape(-1), np.asarray(items, dtype=np.int64).reshape(-1)
    U = w[ONLINE[0]].shape[0]
    P = pooled(tables(w, TARGET if defect == "predict_from_target" else ONLINE), dense_adj(graph), L)
    W, b = w[PREDICTOR[0]].astype(F32), w[PREDICTOR[1]].astype(F32)
    pu, pi = P[users], P[U + items]
    return ((pu @ W.T + b) * pi).sum(axis=1) + (pu * (pi @ W.T + b)).sum(axis=1)


def new_opt_state(w, optimizer):
    """The optimizer's state: the four trained tensors only (the target never has a gradient, hence no state)."""
    return _mf.new_opt_state({k: w[k] for k in TRAINABLE}, optimizer)


def opt_step(w, g, st, optimizer, lr):
    """One optimizer step over the trained tensors, in place; the target tables are not touched."""
    sub = {k: w[k] for k in TRAINABLE}
    _mf.opt_step(sub, g, st, optimizer, lr)
    for k in TRAINABLE:
        w[k] = sub[k]


def ema(w, momentum):
    """buir.py:48-54, in place: t * m + o * (1 - m), the difference taken in double as python takes it."""
    for o, t in zip(ONLINE, TARGET):
        w[t] = (w[t] * F32(momentum) + w[o] * F32(1.0 - momentum)).astype(F32)
