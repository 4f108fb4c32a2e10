"""ORACLE (test infrastructure -- never imported by the product path).

numpy restatement of the CMN training step.  Runs in fp32, or in fp64 inside ``helpers.float64_oracle(cmn_numpy)``
(the working precision is the module global ``F32``).

Reference lines (relative to beta_rec/):
    models/vlml.py:28-57        mask_mod: padded slots score finfo.min, i.e. the softmax runs over the list only
    models/vlml.py:59-91        apply_attention_memory: a_j = z . M[n_j], p = softmax(a), o = sum_j p_j C[n_j]
    models/vlml.py:93-124       hops: z0 = m_u + e_i; z1 = relu(W z0 + b + o0)
    models/cmn.py:63-121        output module: s = w . relu(Wd [m_u * e_i ; o1] + bd)
    models/cmn.py:153-200       train_single_batch: mean(-log(sigmoid(s+ - s-) + 1e-12)) + lambda ||W||_2 (the norm, on
                                mem_layer.hop_mapping.1.weight only), backward, clip_grad_norm_, optimizer.step()
    models/cmn.py:147-149       the engine's own optimizer: RMSprop(lr, momentum)
Pinned against golden vectors captured from the real reference by ``tools/gen_golden_cmn.py`` (tests/golden/cmn_*.npz);
see tests/test_oracle_golden_cmn.py.

Parameters are a dict with the reference's state_dict keys (KEYS, in named_parameters() order).  A batch is the seven
arrays of cmn.py:166-174: users [B], items [B], neg items [B], neighbourhoods [B, Lp], lengths [B], negative
neighbourhoods [B, Ln], negative lengths [B].
"""
import numpy as np

from oracle import mf_numpy

F32 = np.float32
KEYS = ("user_memory.weight", "item_memory.weight", "user_output.weight", "mem_layer.hop_mapping.1.weight",
        "mem_layer.hop_mapping.1.bias", "dense.weight", "dense.bias", "out.weight")
HOP_W = "mem_layer.hop_mapping.1.weight"


def _attend(z, Mn, Cn, mask):
    a = np.einsum("bd,bld->bl", z, Mn).astype(F32)
    a = np.where(mask, a, -np.inf)
    e = np.exp(a - a.max(axis=1, keepdims=True)).astype(F32)
    p = (e / e.sum(axis=1, keepdims=True, dtype=F32)).astype(F32)
    return p, np.einsum("bl,bld->bd", p, Cn).astype(F32)


def cmn_query(w, users, items, nbr, lens):
    """Forward of B queries: the scores [B] and everything the backward needs."""
    M, E, C = (w[k].astype(F32) for k in KEYS[:3])
    W, b, Wd, bd, wo = (w[k].astype(F32) for k in KEYS[3:])
    users, items, nbr, lens = (np.asarray(x, dtype=np.int64) for x in (users, items, nbr, lens))
    L = int(lens.max())
    nb = nbr[:, :L]
    mask = np.arange(L)[None, :] < lens[:, None]
    nb = np.where(mask, nb, 0)
    mu, ei = M[users], E[items]
    Mn, Cn = M[nb], C[nb]
    z0 = mu + ei
    p0, o0 = _attend(z0, Mn, Cn, mask)
    pre1 = (z0 @ W.T + b + o0).astype(F32)
    z1 = np.maximum(pre1, 0)
    p1, o1 = _attend(z1, Mn, Cn, mask)
    x = np.concatenate([mu * ei, o1], axis=1)
    preh = (x @ Wd.T + bd).astype(F32)
    h = np.maximum(preh, 0)
    s = (h @ wo[0]).astype(F32)
    return s, dict(users=users, items=items, nb=nb, mask=mask, mu=mu, ei=ei, Mn=Mn, Cn=Cn, z0=z0, p0=p0, pre1=pre1,
                   z1=z1, p1=p1, x=x, preh=preh, h=h)


def _hop_backward(z, p, do, c):
    dp = np.einsum("bd,bld->bl", do, c["Cn"]).astype(F32)
    da = (p * (dp - (p * dp).sum(axis=1, keepdims=True, dtype=F32))).astype(F32)
    dC = p[:, :, None] * do[:, None, :]
    dM = da[:, :, None] * z[:, None, :]
    return dM, dC, np.einsum("bl,bld->bd", da, c["Mn"]).astype(F32)


def _query_backward(w, c, ds, g):
    W, Wd, wo = w[KEYS[3]].astype(F32), w[KEYS[5]].astype(F32), w[KEYS[7]].astype(F32)
    D = W.shape[0]
    ds = ds.astype(F32)
    dh = (ds[:, None] * wo[0][None, :]) * (c["preh"] > 0)
    g["out.weight"] += (ds[:, None] * c["h"]).sum(axis=0, dtype=F32)[None, :]
    g["dense.weight"] += (dh.T @ c["x"]).astype(F32)
    g["dense.bias"] += dh.sum(axis=0, dtype=F32)
    dx = (dh @ Wd).astype(F32)
    dx0, do1 = dx[:, :D], dx[:, D:]
    dM1, dC1, dz1 = _hop_backward(c["z1"], c["p1"], do1, c)
    t = dz1 * (c["pre1"] > 0)
    c["dh"], c["t"] = dh, t          # per-query vectors, kept for the tests' term-magnitude floors
    g[HOP_W] += (t.T @ c["z0"]).astype(F32)
    g["mem_layer.hop_mapping.1.bias"] += t.sum(axis=0, dtype=F32)
    dM0, dC0, dz0 = _hop_backward(c["z0"], c["p0"], t, c)
    dz0 = dz0 + (t @ W).astype(F32)
    m = c["mask"]
    np.add.at(g["user_memory.weight"], c["nb"][m], (dM1 + dM0)[m])
    np.add.at(g["user_output.weight"], c["nb"][m], (dC1 + dC0)[m])
    np.add.at(g["user_memory.weight"], c["users"], dx0 * c["ei"] + dz0)
    np.add.at(g["item_memory.weight"], c["items"], dx0 * c["mu"] + dz0)


def cmn_grads(w, batch, l2_lambda, with_cache=False):
    """forward + loss + backward of train_single_batch BEFORE the clip: (loss, grads)."""
    users, pos, neg, pn, pl, nn_, nl = batch
    sp, cp = cmn_query(w, users, pos, pn, pl)
    sn, cn = cmn_query(w, users, neg, nn_, nl)
    B = len(sp)
    x = (sp - sn).astype(F32)
    y = (1 / (1 + np.exp(-x))).astype(F32)
    W = w[HOP_W].astype(F32)
    l2 = np.sqrt((W * W).sum(dtype=F32))
    loss = (-np.log(y + F32(1e-12))).mean(dtype=F32) + F32(l2_lambda) * l2
    dx = (-(F32(1) / F32(B)) / (y + F32(1e-12)) * (y * (1 - y))).astype(F32)
    g = {k: np.zeros(np.shape(w[k]), dtype=F32) for k in KEYS}
    _query_backward(w, cp, dx, g)
    _query_backward(w, cn, -dx, g)
    g[HOP_W] += F32(l2_lambda) * W / l2
    g = {k: v.astype(F32) for k, v in g.items()}
    if with_cache:
        return float(loss), g, (cp, cn)
    return float(loss), g


def clip_grads(g, max_norm):
    """torch.nn.utils.clip_grad_norm_: (total_norm, the scaled gradients)."""
    total = np.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values()))
    total = float(F32(total))
    coef = F32(max_norm) / (F32(total) + F32(1e-6))
    if coef >= 1:
        return total, {k: v.copy() for k, v in g.items()}
    return total, {k: (v * F32(coef)).astype(F32) for k, v in g.items()}


def new_opt_state(w, optimizer):
    """``optimizer``: sgd / adam / rmsprop, or rmsprop_momentum (cmn.py:147-149: exp_avg holds the momentum buffer)."""
    if optimizer == "rmsprop_momentum":
        return {"step": 0, "square_avg": mf_numpy.zeros_like_params(w), "momentum_buffer": mf_numpy.zeros_like_params(w)}
    return mf_numpy.new_opt_state(w, optimizer)


def opt_step(w, g, st, optimizer, lr, momentum=0.9):
    if optimizer != "rmsprop_momentum":
        return mf_numpy.opt_step(w, g, st, optimizer, lr)
    # torch/optim/rmsprop.py with momentum > 0: square_avg as without; buf = mu buf + g / (sqrt(square_avg) + eps);
    # p -= lr buf
    st["step"] += 1
    f = mf_numpy.F32
    alpha, eps = 0.99, 1e-8
    for k in w:
        v, buf = st["square_avg"][k], st["momentum_buffer"][k]
        v *= f(alpha)
        v += f(1.0 - alpha) * g[k] * g[k]
        avg = np.sqrt(v, dtype=f) + f(eps)
        buf *= f(momentum)
        buf += g[k] / avg
        w[k] -= f(lr) * buf


def cmn_train_step(w, st, batch, l2_lambda, grad_clip, optimizer, lr, momentum=0.9):
    """cmnEngine.train_single_batch: returns (loss, total_norm); ``w`` and ``st`` move in place."""
    loss, g = cmn_grads(w, batch, l2_lambda)
    total, g = clip_grads(g, grad_clip)
    opt_step(w, g, st, optimizer, lr, momentum)
    return loss, total


def cmn_predict(w, users, items):
    return (w["user_memory.weight"][users] * w["item_memory.weight"][items]).sum(axis=-1, dtype=F32)


def padded_batch(rowptr, col, users, pos, neg, lpad=None):
    """The seven arrays ``cmn_train_loader`` (data/deprecated_data.py:766-860) builds for triples from an item -> users
    CSR: every list copied into a zero-padded row of ``lpad`` (default: the longest list of the CSR) slots."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    lpad = int(np.diff(rowptr).max()) if lpad is None else int(lpad)
    out = [np.asarray(users, dtype=np.int64), np.asarray(pos, dtype=np.int64), np.asarray(neg, dtype=np.int64)]
    for items in (out[1], out[2]):
        nbr = np.zeros((len(items), lpad), dtype=np.int64)
        lens = np.zeros(len(items), dtype=np.int64)
        for r, i in enumerate(items):
            lst = col[rowptr[i]:rowptr[i + 1]]
            nbr[r, :len(lst)] = lst
            lens[r] = len(lst)
        out += [nbr, lens]
    return (out[0], out[1], out[2], out[3], out[4], out[5], out[6])
