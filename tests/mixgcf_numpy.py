"""ORACLE (test infrastructure -- never imported by the product path).

numpy restatement of the MixGCF training step.  Runs in fp32, or in fp64 inside ``helpers.float64_oracle(mixgcf_numpy)``
(the working precision is the module global ``F32``).

Reference lines (relative to beta_rec/models/mixgcf.py):
    :31-44     _sparse_dropout: edge e kept iff floor(rate + r_e) == 1, kept values times 1 / (1 - rate)
    :46-67     GraphConv.forward: E_{l+1} = dropout(A_l E_l), all hops stacked [N, L + 1, D]
    :123-133   pooling: mean / sum / concat / final over the hop axis
    :222-251   negative_sampling: n' = seed p + (1 - seed) n, score against the user, per-hop argmax
    :253-286   create_bpr_loss: mean log(1 + sum_k exp(s_neg_k - s_pos)) + l2 / 2 / B (|u_0|^2 + |p_0|^2 + |n'_0|^2)
    :176-203   train_single_batch -- which stops at the loss; the backward pass and the optimizer step restated here are
               what tools/gen_golden_mixgcf.py performs on the reference's loss tensor itself.
Pinned against golden vectors captured from the real reference (tests/golden/mix_*.npz); see
tests/test_oracle_golden_mixgcf.py.

Parameters are a dict with the reference's state_dict keys.  ``graph`` = ``(rows, cols, vals, N)``: the COO entries of
norm_adj in the order the reference holds them.  ``hp`` = dict(pool, L, n_negs, K, ns, l2, edge_rate, mess_rate) with a
rate of None for a dropout that is off.  ``masks`` = ``(edge, mess)``: per hop a 0/1 array [nnz] in COO order /
[N, D], or None.
"""
import numpy as np

from oracle.mf_numpy import new_opt_state, opt_step  # noqa: F401  (shared optimizer arithmetic)

F32 = np.float32
KEYS = ("user_embedding.weight", "item_embedding.weight")
POOLS = ("concat", "mean", "sum", "final")


def hop_matrix(graph, keep=None, rate=None):
    """Dense [N, N] matrix of one hop: the kept entries times 1 / (1 - rate), as ``out * (1.0 / (1 - rate))`` does."""
    rows, cols, vals, N = graph
    v = np.asarray(vals, dtype=F32)
    if keep is not None:
        v = np.where(np.asarray(keep) != 0, v * F32(1.0 / (1 - rate)), F32(0)).astype(F32)
    A = np.zeros((N, N), dtype=F32)
    np.add.at(A, (np.asarray(rows), np.asarray(cols)), v)
    return A


def mess_factor(keep, rate):
    """The factor nn.Dropout multiplies by: mask / (1 - p) in fp32; None -> no dropout."""
    if keep is None:
        return None
    return (np.asarray(keep, dtype=F32) / F32(1 - rate)).astype(F32)


def propagate(w, graph, hp, masks=None):
    """``(E [L + 1, N, D], mats, factors)``: the hop tables, and per hop the matrix and message factor that made them."""
    E0 = np.concatenate([w["user_embedding.weight"], w["item_embedding.weight"]], axis=0).astype(F32)
    edge, mess = masks if masks is not None else (None, None)
    E, mats, facs = [E0], [], []
    for l in range(hp["L"]):
        A = hop_matrix(graph, None if edge is None else edge[l], hp.get("edge_rate"))
        f = None if mess is None else mess_factor(mess[l], hp.get("mess_rate"))
        x = (A @ E[-1]).astype(F32)
        if f is not None:
            x = (x * f).astype(F32)
        E.append(x)
        mats.append(A)
        facs.append(f)
    return np.stack(E, axis=0), mats, facs


def pooling(x, pool):
    """mixgcf.py:123-133 on [..., H, D]."""
    if pool == "mean":
        return x.mean(axis=-2, dtype=F32)
    if pool == "sum":
        return x.sum(axis=-2, dtype=F32)
    if pool == "concat":
        return x.reshape(x.shape[:-2] + (-1,))
    if pool == "final":
        return x[..., -1, :]
    raise ValueError(pool)


def unpool(d, pool, H):
    """Gradient of :func:`pooling`: [..., D or H D] -> [..., H, D]."""
    if pool == "concat":
        return d.reshape(d.shape[:-1] + (H, -1))
    out = np.zeros(d.shape[:-1] + (H, d.shape[-1]), dtype=F32)
    if pool == "mean":
        out[...] = (d / F32(H))[..., None, :]
    elif pool == "sum":
        out[...] = d[..., None, :]
    else:
        out[..., -1, :] = d
    return out


def candidates(neg, hp):
    """[B, K, n] candidate ids of every negative (rns: n = 1, column k)."""
    neg = np.asarray(neg, dtype=np.int64)
    K = hp["K"]
    if hp["ns"] == "rns":
        return neg[:, :K, None]
    n = hp["n_negs"]
    return neg[:, : K * n].reshape(neg.shape[0], K, n)


def mixed(E, n_users, pos, cand, seeds):
    """n' [B, K, n, H, D] = seed * p + (1 - seed) * cand rows; seeds [B, K, H] (None: no mixing)."""
    Et = np.transpose(E, (1, 0, 2))                       # [N, H, D]
    n_e = Et[n_users + cand]                              # [B, K, n, H, D]
    if seeds is None:
        return n_e
    sd = np.asarray(seeds, dtype=F32)[:, :, None, :, None]
    p_e = Et[n_users + np.asarray(pos)][:, None, None]    # [B, 1, 1, H, D]
    return (sd * p_e + (F32(1) - sd) * n_e).astype(F32)


def sampler_scores(E, n_users, users, pos, cand, seeds, pool):
    """[B, K, n, H]: every mixed candidate's score at every hop (mixgcf.py:227-242)."""
    Et = np.transpose(E, (1, 0, 2))
    s_e = Et[np.asarray(users)]                           # [B, H, D]
    if pool != "concat":
        s_e = pooling(s_e, pool)[:, None, :]              # [B, 1, D]
    return (s_e[:, None, None] * mixed(E, n_users, pos, cand, seeds)).sum(axis=-1, dtype=F32)


def mix_grads(w, graph, hp, batch, seeds, masks=None, choice=None, defect=None):
    """forward + sampler + loss + backward: ``(loss, grads, choice)``.  ``choice`` [B, K, H] given: differentiate under
    that choice instead of the argmax.  ``defect`` (tests/test_mixgcf_edges_host.py only) plants one known mistake:
    "drop_pos_seed_term" leaves seed * d n' out of the positive's gradient, "reg_unmixed" takes the regulariser on the
    unmixed candidate."""
    users, pos, neg = (np.asarray(x, dtype=np.int64) for x in batch)
    U = w["user_embedding.weight"].shape[0]
    pool, L, K = hp["pool"], hp["L"], hp["K"]
    H, B = L + 1, users.shape[0]
    E, mats, facs = propagate(w, graph, hp, masks)
    cand = candidates(neg, hp)
    sd = None if hp["ns"] == "rns" else np.asarray(seeds, dtype=F32)
    if choice is None:
        choice = sampler_scores(E, U, users, pos, cand, sd, pool).argmax(axis=2)     # first maximum = lowest j
    choice = np.asarray(choice, dtype=np.int64)
    item = np.take_along_axis(cand, choice if cand.shape[2] > 1 else np.zeros_like(choice), axis=2)   # [B, K, H]
    Et = np.transpose(E, (1, 0, 2))
    hop = np.arange(H)
    u, p = Et[users], Et[U + pos]                         # [B, H, D]
    c = Et[U + item, hop[None, None, :]]                  # [B, K, H, D]: hop l of the item chosen at hop l
    if sd is None:
        n = c
        sdx = np.zeros((B, K, H, 1), dtype=F32)
    else:
        sdx = sd[..., None]
        n = (sdx * p[:, None] + (F32(1) - sdx) * c).astype(F32)
    pu, pp, pn = pooling(u, pool), pooling(p, pool), pooling(n, pool)
    s_pos = (pu * pp).sum(axis=-1, dtype=F32)
    s_neg = (pu[:, None] * pn).sum(axis=-1, dtype=F32)    # [B, K]
    x = s_neg - s_pos[:, None]
    m = np.maximum(x.max(axis=1), 0)
    ex = np.exp(x - m[:, None])
    z = np.exp(-m) + ex.sum(axis=1, dtype=F32)
    mf = (m + np.log(z)).mean(dtype=F32)
    l2 = F32(hp["l2"])
    n_reg = c if defect == "reg_unmixed" else n
    reg = l2 * ((u[:, 0] ** 2).sum(dtype=F32) + (p[:, 0] ** 2).sum(dtype=F32) + (n_reg[:, :, 0] ** 2).sum(dtype=F32)) / F32(2) / F32(B)
    loss = mf + reg
    gk = (ex / z[:, None] / F32(B)).astype(F32)           # d loss / d x_k
    dpu = (gk[:, :, None] * (pn - pp[:, None])).sum(axis=1, dtype=F32)
    dpp = -gk.sum(axis=1, dtype=F32)[:, None] * pu
    dpn = gk[:, :, None] * pu[:, None]
    dU, dP, dN = unpool(dpu, pool, H), unpool(dpp, pool, H), unpool(dpn, pool, H)
    cr = l2 / F32(B)
    dU[:, 0] += cr * u[:, 0]
    dP[:, 0] += cr * p[:, 0]
    if defect != "reg_unmixed":
        dN[:, :, 0] += cr * n[:, :, 0]
    if defect != "drop_pos_seed_term":
        dP = dP + (sdx * dN).sum(axis=1, dtype=F32)
    dC = ((F32(1) - sdx) * dN).astype(F32)
    if defect == "reg_unmixed":
        dC[:, :, 0] += cr * c[:, :, 0]
    N, D = E.shape[1], E.shape[2]
    G = np.zeros((H, N, D), dtype=F32)
    for l in range(H):
        np.add.at(G[l], users, dU[:, l])
        np.add.at(G[l], U + pos, dP[:, l])
        np.add.at(G[l], (U + item[:, :, l]).reshape(-1), dC[:, :, l].reshape(-1, D))
    dE = G[L]
    for l in range(L - 1, -1, -1):
        t = dE if facs[l] is None else (dE * facs[l]).astype(F32)
        dE = (G[l] + mats[l].T @ t).astype(F32)
    g = {"user_embedding.weight": dE[:U].astype(F32), "item_embedding.weight": dE[U:].astype(F32)}
    return float(loss), g, choice


def mix_predict(w, graph, hp, users, items):
    """LightGCN.predict: eval-mode propagation, pooled rows, dot product."""
    E, _, _ = propagate(w, graph, hp)
    U = w["user_embedding.weight"].shape[0]
    Et = np.transpose(E, (1, 0, 2))
    return (pooling(Et[np.asarray(users)], hp["pool"]) * pooling(Et[U + np.asarray(items)], hp["pool"])).sum(axis=-1, dtype=F32)


def mix_factors(w, graph, hp):
    """The pooled (user, item) tables of ``ranking_factors``."""
    E, _, _ = propagate(w, graph, hp)
    U = w["user_embedding.weight"].shape[0]
    pooled = pooling(np.transpose(E, (1, 0, 2)), hp["pool"])
    return pooled[:U], pooled[U:]


def mix_train_step(w, st, graph, hp, batch, seeds, masks=None, optimizer="adam", lr=0.05):
    """The step the mirror performs: returns (loss, choice); ``w`` and ``st`` move in place."""
    loss, g, choice = mix_grads(w, graph, hp, batch, seeds, masks)
    opt_step(w, g, st, optimizer, lr)
    return loss, choice
