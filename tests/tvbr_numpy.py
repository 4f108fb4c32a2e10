"""Numpy restatement of beta_rec/models/tvbr.py (test infrastructure): forward, loss, the analytic backward and the
optimizer step of one ``TVBREngine.train_single_batch``, pinned to the real reference by
tests/test_oracle_golden_tvbr.py.

The working precision is the module global ``F32`` (``helpers.float64_oracle`` turns it into float64).  Weights are a
dict keyed like the reference's ``state_dict``; ``fea = (user_fea [U, Fu], item_fea [I, Fi])``; a batch is the
reference's eight-tuple ``(pos_u, pos_i_1, pos_i_2 [B], neg_u, neg_i_1, neg_i_2 [B, n_neg], pos_t [B], neg_t [B n_neg])``;
``eps`` the six noise blocks of ``reparameterize`` in the reference's call order (pos_u, pos_i_1, pos_i_2, neg_u,
neg_i_1, neg_i_2), each ``[rows, D]``; ``scale`` is ``1 / (3 * config batch_size)``.  It restates the reference as it
is written: the concatenated input ``[table[id] | time row | fea[id]]`` goes through every ``Linear`` twice.

Five deliberately WRONG variants exist for the visibility checks only: ``z_from_std`` reparameterizes with ``std``
itself instead of ``exp(0.5 std)``; ``swap_time`` gives the prior the time row ``t + 1`` and the posterior ``t``;
``time_onehot`` takes the time table as the identity it is constructed as; ``kl_sign`` drops the minus of ``kl_loss``;
``neg_kl_over_b`` takes the negative groups' KL mean over ``B`` instead of ``B n_neg``.  A wrong ``scale`` is simply
passed in by the caller.
"""
import numpy as np

from oracle import mf_numpy

F32 = np.float32
ESP = 1e-10
ENCODERS = ("time2mean_u", "time2std_u", "time2mean_i", "time2std_i")
TABLES = {"time2mean_u": "user_mean.weight", "time2std_u": "user_std.weight", "time2mean_i": "item_mean.weight",
          "time2std_i": "item_std.weight"}
ACTIVATORS = ("tanh", "hardtanh", "logsigmoid", "sigmoid", "relu", "lrelu", "prelu")
PIECEWISE = {"relu": (0.0,), "lrelu": (0.0,), "prelu": (0.0,), "hardtanh": (-1.0, 1.0)}     # where act' jumps


def shapes(U, I, D, T, Fu, Fi, prelu=False):
    """``{name: shape}`` in the reference's ``state_dict`` order."""
    T1 = T + 1
    out = {"user_emb.weight": (U, D), "item_emb.weight": (I, D), "time_embdding.weight": (T1, T1),
           "user_mean.weight": (U, D), "user_std.weight": (U, D), "item_mean.weight": (I, D), "item_std.weight": (I, D)}
    for name, F in zip(ENCODERS, (Fu, Fu, Fi, Fi)):
        out[name + ".0.weight"] = (D, D + T1 + F)
        out[name + ".0.bias"] = (D,)
        if prelu:
            out[name + ".1.weight"] = (1,)
    return out


def keys(prelu=False):
    return tuple(shapes(1, 1, 1, 1, 1, 1, prelu))


def _sigmoid(x):
    e = np.exp(-np.abs(x), dtype=F32)
    return np.where(x >= 0, F32(1.0) / (F32(1.0) + e), e / (F32(1.0) + e)).astype(F32)


def _neg_logsigmoid(x):
    """-F.logsigmoid(x) = log1p(exp(-|x|)) - min(x, 0)."""
    return np.log1p(np.exp(-np.abs(x), dtype=F32), dtype=F32) - np.minimum(x, F32(0.0))


def act(x, name, slope=None):
    if name == "tanh":
        return np.tanh(x, dtype=F32)
    if name == "hardtanh":
        return np.clip(x, F32(-1.0), F32(1.0)).astype(F32)
    if name == "logsigmoid":
        return (-_neg_logsigmoid(x)).astype(F32)
    if name == "sigmoid":
        return _sigmoid(x)
    if name == "relu":
        return np.where(x > 0, x, F32(0.0)).astype(F32)
    if name == "lrelu":
        return np.where(x > 0, x, F32(0.01) * x).astype(F32)
    if name == "prelu":
        return np.where(x > 0, x, F32(slope) * x).astype(F32)
    raise ValueError(name)


def act_grad(pre, name, slope=None):
    if name == "tanh":
        h = np.tanh(pre, dtype=F32)
        return F32(1.0) - h * h
    if name == "hardtanh":
        return ((pre > -1) & (pre < 1)).astype(F32)
    if name == "logsigmoid":
        return _sigmoid(-pre)
    if name == "sigmoid":
        h = _sigmoid(pre)
        return h * (F32(1.0) - h)
    if name == "relu":
        return (pre > 0).astype(F32)
    if name == "lrelu":
        return np.where(pre > 0, F32(1.0), F32(0.01)).astype(F32)
    if name == "prelu":
        return np.where(pre > 0, F32(1.0), F32(slope)).astype(F32)
    raise ValueError(name)


def _slope(w, enc, activator):
    return F32(w[enc + ".1.weight"][0]) if activator == "prelu" else None


def _linear(w, enc, fea, ids, time_rows, activator):
    """``(X, pre, h)`` of ``act(Linear([table[ids] | time_rows | fea[ids]]))`` for encoder ``enc``."""
    X = np.concatenate([w[TABLES[enc]][ids], time_rows, np.asarray(fea, dtype=F32)[ids]], 1)
    pre = X @ w[enc + ".0.weight"].T + w[enc + ".0.bias"]
    return X, pre, act(pre, activator, _slope(w, enc, activator))


def encode(w, fea, ids, side, activator):
    """Eval mode (tvbr.py:380-407): ``[posterior mean(id) at t = time_step | emb[id]]`` as ``[n, 2D]``; ``side`` ``"u"``
    or ``"i"``."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    ids = np.asarray(ids)
    TE = w["time_embdding.weight"]
    rows = np.repeat(TE[TE.shape[0] - 1][None], len(ids), 0)
    table = w["user_emb.weight" if side == "u" else "item_emb.weight"]
    return np.concatenate([_linear(w, "time2mean_" + side, fea, ids, rows, activator)[2], table[ids]], 1)


def predict(w, fea, users, items, activator):
    """``TVBR.predict`` (tvbr.py:371-412)."""
    return (encode(w, fea[0], users, "u", activator) * encode(w, fea[1], items, "i", activator)).sum(1, dtype=F32)


def tvbr_grads(w, fea, batch, eps, alpha, scale, activator, z_from_std=False, swap_time=False, time_onehot=False,
               kl_sign=False, neg_kl_over_b=False):
    """``(loss, rec_loss, kl_loss, {name: gradient}, info)`` of ``TVBR.forward`` (tvbr.py:242-369) and its backward."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    pos_u, pos_1, pos_2, neg_u, neg_1, neg_2 = (np.asarray(a, dtype=np.int64) for a in batch[:6])
    pos_t, neg_t = (np.asarray(a, dtype=np.int64).ravel() for a in batch[6:])
    B = pos_u.shape[0]
    n_neg = neg_u.size // B
    Bn = B * n_neg
    D = w["user_emb.weight"].shape[1]
    T1 = w["time_embdding.weight"].shape[0]
    eps = [np.asarray(e, dtype=F32).reshape(-1, D) for e in eps]
    alpha, scale, one, half = F32(alpha), F32(scale), F32(1.0), F32(0.5)
    TE = np.eye(T1, dtype=F32) if time_onehot else w["time_embdding.weight"]
    kl_coef = F32(0.5) if kl_sign else F32(-0.5)            # kl_loss = -0.5 sum of the six terms

    sides, gap = {}, np.inf
    for side, ids, t, noise, blocks, table in (
            ("u", np.concatenate([pos_u, neg_u.ravel()]), np.concatenate([pos_t, neg_t]),
             np.concatenate([eps[0], eps[3]]), (B, Bn), "user_emb.weight"),
            ("i", np.concatenate([pos_1, pos_2, neg_1.ravel(), neg_2.ravel()]), np.concatenate([pos_t, pos_t, neg_t, neg_t]),
             np.concatenate([eps[1], eps[2], eps[4], eps[5]]), (B, B, Bn, Bn), "item_emb.weight")):
        t_pri, t_post = (t + 1, t) if swap_time else (t, t + 1)
        c = dict(ids=ids, t_pri=t_pri, t_post=t_post, noise=noise, table=table)
        for kind in ("mean", "std"):
            enc = f"time2{kind}_{side}"
            for tag, rows in (("p", t_pri), ("q", t_post)):
                c[f"X{kind}{tag}"], c[f"pre{kind}{tag}"], c[f"h{kind}{tag}"] = _linear(w, enc, fea[0 if side == "u" else 1],
                                                                                   ids, TE[rows], activator)
                for kink in PIECEWISE.get(activator, ()):
                    gap = min(gap, float(np.abs(c[f"pre{kind}{tag}"] - kink).min()))
        mp, mq = c["hmeanp"], c["hmeanq"]
        sp, sq = np.exp(half * c["hstdp"], dtype=F32), np.exp(half * c["hstdq"], dtype=F32)
        ez = noise if z_from_std else noise * np.exp(half * sq, dtype=F32)
        z = mq + (ez * sq if z_from_std else ez)
        groups = [B if (neg_kl_over_b and n == Bn) else n for n in blocks]
        klw = np.concatenate([np.full(n, one / F32(m), dtype=F32) for n, m in zip(blocks, groups)])[:, None]
        var1, var2 = sp * sp + F32(ESP), sq * sq + F32(ESP)
        dm = mq - mp
        kl = (half * (np.log(var2 / var1, dtype=F32) - one + (one / var2) * var1 + dm * (one / var2) * dm) * klw).sum(dtype=F32)
        c["kl_terms"] = float((half * (np.abs(np.log(var2 / var1)) + one + var1 / var2 + dm * dm / var2) * klw).sum())
        c.update(kl=kl, klw=klw, sp=sp, sq=sq, ez=ez, var1=var1, var2=var2, dm=dm,
                 e=np.concatenate([z, w[table][ids]], 1))
        sides[side] = c

    eu_all, ei_all = sides["u"]["e"], sides["i"]["e"]
    eu, nu = eu_all[:B], eu_all[B:].reshape(B, n_neg, 2 * D)
    e1, e2 = ei_all[:B], ei_all[B:2 * B]
    n1 = ei_all[2 * B:2 * B + Bn].reshape(B, n_neg, 2 * D)
    n2 = ei_all[2 * B + Bn:].reshape(B, n_neg, 2 * D)
    # (vector, the two vectors whose SUM it is scored against) -- tvbr.py:338-358
    partners = {"u": ("1", "2"), "1": ("u", "2"), "2": ("u", "1")}
    vec = {"u": eu, "1": e1, "2": e2}
    negs = {"u": nu, "1": n1, "2": n2}
    gen = F32(0.0)
    d = {k: np.zeros_like(eu) for k in vec}
    dn = {}
    for k in ("u", "1", "2"):
        inp = vec[partners[k][0]] + vec[partners[k][1]]
        x = (vec[k] * inp).sum(1, dtype=F32)
        y = np.einsum("bnd,bd->bn", negs[k], vec[k]).astype(F32)
        gen = gen + _neg_logsigmoid(x).sum(dtype=F32) + _neg_logsigmoid(-y).sum(dtype=F32)
        dx = (-_sigmoid(-x) * scale)[:, None]
        dy = _sigmoid(y) * scale
        d[k] = d[k] + dx * inp + np.einsum("bn,bnd->bd", dy, negs[k]).astype(F32)
        for other in partners[k]:
            d[other] = d[other] + dx * vec[k]
        dn[k] = dy[:, :, None] * vec[k][:, None, :]
    rec = gen * scale
    kl_loss = kl_coef * (sides["u"]["kl"] + sides["i"]["kl"])
    loss = (one - alpha) * rec + alpha * kl_loss

    de = {"u": np.concatenate([d["u"], dn["u"].reshape(Bn, 2 * D)]),
          "i": np.concatenate([d["1"], d["2"], dn["1"].reshape(Bn, 2 * D), dn["2"].reshape(Bn, 2 * D)])}
    g = {k: np.zeros_like(v) for k, v in w.items()}
    for side, c in sides.items():
        dE = (one - alpha) * de[side]
        dz, dt = dE[:, :D], dE[:, D:]
        np.add.at(g[c["table"]], c["ids"], dt)
        ck = alpha * kl_coef * c["klw"]
        r2, var1, dm, sp, sq = one / c["var2"], c["var1"], c["dm"], c["sp"], c["sq"]
        g_m = ck * dm * r2
        dh = {"meanp": -g_m, "meanq": dz + g_m,
              "stdp": ck * half * (r2 - one / var1) * sp * sp,
              "stdq": dz * c["ez"] * (half if z_from_std else F32(0.25)) * sq
              + ck * half * (r2 - var1 * r2 * r2 - dm * dm * r2 * r2) * sq * sq}
        for kind in ("mean", "std"):
            enc = f"time2{kind}_{side}"
            W, slope = w[enc + ".0.weight"], _slope(w, enc, activator)
            for tag, rows in (("p", c["t_pri"]), ("q", c["t_post"])):
                pre, X = c[f"pre{kind}{tag}"], c[f"X{kind}{tag}"]
                dpre = dh[kind + tag] * act_grad(pre, activator, slope)
                g[enc + ".0.weight"] += dpre.T @ X
                g[enc + ".0.bias"] += dpre.sum(0, dtype=F32)
                if activator == "prelu":
                    g[enc + ".1.weight"] += (dh[kind + tag] * np.where(pre > 0, F32(0.0), pre)).sum(dtype=F32)
                dX = dpre @ W
                np.add.at(g[TABLES[enc]], c["ids"], dX[:, :D])
                np.add.at(g["time_embdding.weight"], rows, dX[:, D:D + T1])
    g = {k: np.asarray(v, dtype=F32) for k, v in g.items()}
    # kl_terms: 0.5 x the summed MAGNITUDES of what kl_loss adds up (log, -1, the variance ratio, the mean term): they
    # cancel where prior and posterior are close, the rounding error of an fp32 evaluation does not
    info = {"min_kink_gap": gap, "kl_terms": 0.5 * (sides["u"]["kl_terms"] + sides["i"]["kl_terms"])}
    return float(loss), float(rec), float(kl_loss), g, info


new_opt_state = mf_numpy.new_opt_state
opt_step = mf_numpy.opt_step


def train_step(w, st, fea, batch, eps, alpha, scale, activator, optimizer, lr):
    loss, rec, kl, g, _ = tvbr_grads(w, fea, batch, eps, alpha, scale, activator)
    opt_step(w, g, st, optimizer, lr)
    return loss, rec, kl
