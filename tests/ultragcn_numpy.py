"""ORACLE (test infrastructure -- never imported by the product path).

numpy restatement of the UltraGCN training step.  Runs in fp32, or in fp64 inside ``helpers.float64_oracle(ultragcn_numpy)``
(the working precision is the module global ``F32``).

Reference lines (relative to beta_rec/):
    data/base_data.py:410-431      create_constraint_mat: beta_uD = sqrt(d_u + 1) / d_u, beta_iD = 1 / sqrt(d_i + 1), fp32
    models/ultragcn.py:9-33        get_ii_constraint_mat: A = M^T M, Omega = (beta_u' beta_i'^T) o A, topk per row
    models/ultragcn.py:72-100      get_omegas: wp = w1 + w2 bu[u] bi[p]; wn = w3 + w4 bu[u] bi[n] (w3 when w4 <= 0)
    models/ultragcn.py:102-134     cal_loss_L: sum_b [wp bce(s+, 1) + negative_weight mean_n(wn bce(s-, 0))]
    models/ultragcn.py:136-151     cal_loss_I: sum -sim log(sigmoid(s))
    models/ultragcn.py:153-157     norm_loss: sum of squares of every parameter / 2
    models/ultragcn.py:159-165     forward: L + gamma norm + lambda I
    models/ultragcn.py:196-216     train_single_batch: zero_grad, forward, backward, step
Pinned against golden vectors captured from the real reference by ``tools/gen_golden_ultragcn.py``
(tests/golden/ug_*.npz); see tests/test_oracle_golden_ultragcn.py.

Parameters are a dict with the reference's state_dict keys: user_embeds.weight [U,D], item_embeds.weight [I,D].
``hp`` is a dict with w1 w2 w3 w4 negative_weight gamma lambda.
"""
import numpy as np

from oracle.mf_numpy import new_opt_state, opt_step  # noqa: F401  (shared optimizer arithmetic)

F32 = np.float32
KEYS = ("user_embeds.weight", "item_embeds.weight")
DEFAULT_HP = {"w1": 1e-7, "w2": 1.0, "w3": 1e-7, "w4": 1.0, "negative_weight": 200.0, "gamma": 1e-4, "lambda": 1e-3}


def softplus(x):
    """log(1 + e^x), stable: binary_cross_entropy_with_logits(s, 1) = softplus(-s), (s, 0) = softplus(s)."""
    return (np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))).astype(F32)


def sigmoid(x):
    z = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + z), z / (1 + z)).astype(F32)


def betas(train_mat):
    """base_data.py:424-428 on a dense 0/1 [U, I] matrix: fp32 like the reference's float32 dok matrix."""
    M = np.asarray(train_mat, dtype=np.float32)
    items_D, users_D = M.sum(axis=0), M.sum(axis=1)
    return (np.sqrt(users_D + 1) / users_D).astype(np.float32), (1 / np.sqrt(items_D + 1)).astype(np.float32)


def omega_matrix(train_mat, ii_diagonal_zero=False):
    """ultragcn.py:11-22: the dense [I, I] matrix whose rows get_ii_constraint_mat takes the top K of (fp32)."""
    M = np.asarray(train_mat, dtype=np.float32)
    A = (M.T @ M).astype(np.float32)
    if ii_diagonal_zero:
        np.fill_diagonal(A, 0)
    items_D, users_D = A.sum(axis=0), A.sum(axis=1)
    beta_uD = (np.sqrt(users_D + 1) / users_D).astype(np.float32)
    beta_iD = (1 / np.sqrt(items_D + 1)).astype(np.float32)
    return (beta_uD[:, None] * beta_iD[None, :]).astype(np.float32) * A


def ii_constraint_tables(train_mat, num_neighbors, ii_diagonal_zero=False):
    """ultragcn.py:23-33: (neighbour ids [I, K], sims [I, K]); ties go to the smaller id (topk leaves them open)."""
    om = omega_matrix(train_mat, ii_diagonal_zero)
    order = np.argsort(-om, axis=1, kind="stable")[:, :num_neighbors]
    return order.astype(np.int64), np.take_along_axis(om, order, axis=1)


def omegas(hp, beta_u, beta_i, users, pos, neg):
    """get_omegas: (pos_weight [B], neg_weight [B, N]), fp32 as in the reference (beta is fp32 there)."""
    bu = np.asarray(beta_u, dtype=F32)[users]
    bi = np.asarray(beta_i, dtype=F32)
    wp = F32(hp["w1"]) + F32(hp["w2"]) * (bu * bi[pos])
    if hp["w4"] > 0:
        wn = F32(hp["w3"]) + F32(hp["w4"]) * (bu[:, None] * bi[neg])
    else:
        wn = np.full(np.shape(neg), F32(hp["w3"]), dtype=F32)
    return wp.astype(F32), wn.astype(F32)


def ug_scores(w, users, items):
    """UltraGCN.predict: <U[u], V[i]>."""
    return (w["user_embeds.weight"][users] * w["item_embeds.weight"][items]).sum(axis=-1, dtype=F32)


def ug_grads(w, users, pos, neg, hp, beta_u, beta_i, nbr, sim):
    """forward + loss + backward of train_single_batch: (loss, grads), the gamma term included in both."""
    U, V = w["user_embeds.weight"].astype(F32), w["item_embeds.weight"].astype(F32)
    users, pos, neg = (np.asarray(x, dtype=np.int64) for x in (users, pos, neg))
    N = neg.shape[1]
    u = U[users]                                                   # [B, D]
    sp = (u * V[pos]).sum(axis=-1, dtype=F32)                      # [B]
    sn = np.einsum("bd,bnd->bn", u, V[neg]).astype(F32)            # [B, N]
    wp, wn = omegas(hp, beta_u, beta_i, users, pos, neg)
    nw, gamma, lam = F32(hp["negative_weight"]), F32(hp["gamma"]), F32(hp["lambda"])
    loss_L = (wp * softplus(-sp) + (wn * softplus(sn)).mean(axis=-1, dtype=F32) * nw).sum(dtype=F32)
    norm = ((U * U).sum(dtype=F32) + (V * V).sum(dtype=F32)) / F32(2)
    K = 0 if nbr is None else np.shape(nbr)[1]
    dsp = -wp * sigmoid(-sp)
    dsn = (nw / F32(N)) * wn * sigmoid(sn)
    g = {"user_embeds.weight": gamma * U, "item_embeds.weight": gamma * V}
    gu = dsp[:, None] * V[pos] + np.einsum("bn,bnd->bd", dsn, V[neg]).astype(F32)
    np.add.at(g["item_embeds.weight"], pos, dsp[:, None] * u)
    np.add.at(g["item_embeds.weight"], neg.reshape(-1), (dsn[:, :, None] * u[:, None, :]).reshape(-1, u.shape[1]))
    loss_I = F32(0)
    if K and lam != 0:
        nb, sm = np.asarray(nbr, dtype=np.int64)[pos], np.asarray(sim, dtype=F32)[pos]   # [B, K]
        sk = np.einsum("bd,bkd->bk", u, V[nb]).astype(F32)
        loss_I = (sm * softplus(-sk)).sum(dtype=F32)               # -sim * log(sigmoid(s))
        dsk = -lam * sm * sigmoid(-sk)
        gu = gu + np.einsum("bk,bkd->bd", dsk, V[nb]).astype(F32)
        np.add.at(g["item_embeds.weight"], nb.reshape(-1), (dsk[:, :, None] * u[:, None, :]).reshape(-1, u.shape[1]))
    np.add.at(g["user_embeds.weight"], users, gu)
    loss = loss_L + gamma * norm + lam * loss_I
    return float(loss), {k: v.astype(F32) for k, v in g.items()}


def ug_train_step(w, st, batch, hp, beta_u, beta_i, nbr, sim, optimizer="adam", lr=0.05):
    """UltraGCNEngine.train_single_batch: returns the loss; ``w`` and ``st`` move in place."""
    loss, g = ug_grads(w, batch[0], batch[1], batch[2], hp, beta_u, beta_i, nbr, sim)
    opt_step(w, g, st, optimizer, lr)
    return loss
