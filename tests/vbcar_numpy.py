"""Numpy restatement of beta_rec/models/vbcar.py (test infrastructure): forward, loss, the analytic backward and the
optimizer step of one ``VBCAREngine.train_single_batch``, pinned to the real reference by
tests/test_oracle_golden_vbcar.py.

The working precision is the module global ``F32`` (``helpers.float64_oracle`` turns it into float64).  Weights are a
dict keyed like the reference's ``state_dict``; ``fea = (user_fea [U, Fu], item_fea [I, Fi])``; a batch is ``(pos_u,
pos_i_1, pos_i_2 [B], neg_u, neg_i_1, neg_i_2 [B, n_neg])``; ``eps`` the six noise blocks of ``reparameterize`` in the
reference's call order (pos_u, pos_i_1, pos_i_2, neg_u, neg_i_1, neg_i_2), each ``[rows, D]``; ``scale`` is
``1 / (3 * config batch_size)``.

Four deliberately WRONG variants exist for the visibility checks only: ``kl_from_std`` takes the KL variance from
``exp(0.5 s)`` instead of the raw ``s``; ``swap_eps`` exchanges the ``neg_i_1`` and ``neg_i_2`` noise blocks;
``pos_single`` scores each positive against ONE other vector instead of the sum of two; a wrong ``scale`` is simply
passed in by the caller.
"""
import numpy as np

from oracle import mf_numpy

F32 = np.float32
ESP = 1e-10

KEYS = ("user_emb.weight", "item_emb.weight", "fc_u_1_mu.weight", "fc_u_1_mu.bias", "fc_u_2_mu.weight", "fc_u_2_mu.bias",
        "fc_i_1_mu.weight", "fc_i_1_mu.bias", "fc_i_2_mu.weight", "fc_i_2_mu.bias")


def shapes(U, I, D, L, Fu, Fi):
    return {"user_emb.weight": (U, D), "item_emb.weight": (I, D),
            "fc_u_1_mu.weight": (L, Fu), "fc_u_1_mu.bias": (L,), "fc_u_2_mu.weight": (2 * D, L), "fc_u_2_mu.bias": (2 * D,),
            "fc_i_1_mu.weight": (L, Fi), "fc_i_1_mu.bias": (L,), "fc_i_2_mu.weight": (2 * D, L), "fc_i_2_mu.bias": (2 * D,)}


def _sigmoid(x):
    e = np.exp(-np.abs(x), dtype=F32)
    return np.where(x >= 0, F32(1.0) / (F32(1.0) + e), e / (F32(1.0) + e)).astype(F32)


def _neg_logsigmoid(x):
    """-F.logsigmoid(x) = log1p(exp(-|x|)) - min(x, 0)."""
    return np.log1p(np.exp(-np.abs(x), dtype=F32), dtype=F32) - np.minimum(x, F32(0.0))


def act(x, name):
    if name == "tanh":
        return np.tanh(x, dtype=F32)
    if name == "sigmoid":
        return _sigmoid(x)
    if name == "relu":
        return np.where(x > 0, x, F32(0.0)).astype(F32)
    if name == "lrelu":
        return np.where(x > 0, x, F32(0.01) * x).astype(F32)
    return x


def act_grad(h, pre, name):
    if name == "tanh":
        return F32(1.0) - h * h
    if name == "sigmoid":
        return h * (F32(1.0) - h)
    if name == "relu":
        return (pre > 0).astype(F32)
    if name == "lrelu":
        return np.where(pre > 0, F32(1.0), F32(0.01)).astype(F32)
    return np.ones_like(h)


def _encoder(w, fea, ids, side, activator):
    """``(X, pre, h, out)`` of ``fc_2(act(fc_1(fea[ids])))`` for side ``"u"`` or ``"i"``."""
    X = np.asarray(fea, dtype=F32)[ids]
    pre = X @ w[f"fc_{side}_1_mu.weight"].T + w[f"fc_{side}_1_mu.bias"]
    h = act(pre, activator)
    out = h @ w[f"fc_{side}_2_mu.weight"].T + w[f"fc_{side}_2_mu.bias"]
    return X, pre, h, out


def encode(w, fea, ids, side, activator):
    """Eval mode: ``[mu(id) | emb[id]]`` as ``[n, 2D]``; ``side`` ``"u"`` or ``"i"``."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    ids = np.asarray(ids)
    table = w["user_emb.weight" if side == "u" else "item_emb.weight"]
    D = table.shape[1]
    return np.concatenate([_encoder(w, fea, ids, side, activator)[3][:, :D], table[ids]], 1)


def predict(w, fea, users, items, activator):
    """``VBCAR.predict`` (vbcar.py:180-193)."""
    return (encode(w, fea[0], users, "u", activator) * encode(w, fea[1], items, "i", activator)).sum(1, dtype=F32)


def vbcar_grads(w, fea, batch, eps, alpha, scale, activator, kl_from_std=False, swap_eps=False, pos_single=False):
    """``(loss, GEN, KLD, {name: gradient}, info)`` of ``VBCAR.forward`` (vbcar.py:111-178) and its backward."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    pos_u, pos_1, pos_2, neg_u, neg_1, neg_2 = (np.asarray(a, dtype=np.int64) for a in batch)
    B = pos_u.shape[0]
    n_neg = neg_u.size // B
    Bn = B * n_neg
    D = w["user_emb.weight"].shape[1]
    eps = [np.asarray(e, dtype=F32).reshape(-1, D) for e in eps]
    if swap_eps:
        eps[4], eps[5] = eps[5], eps[4]
    alpha, scale, one = F32(alpha), F32(scale), F32(1.0)
    var2 = one + F32(ESP)

    sides = {}
    for side, ids, noise, blocks, table in (
            ("u", np.concatenate([pos_u, neg_u.ravel()]), np.concatenate([eps[0], eps[3]]), (B, Bn), "user_emb.weight"),
            ("i", np.concatenate([pos_1, pos_2, neg_1.ravel(), neg_2.ravel()]),
             np.concatenate([eps[1], eps[2], eps[4], eps[5]]), (B, B, Bn, Bn), "item_emb.weight")):
        X, pre, h, out = _encoder(w, fea[0 if side == "u" else 1], ids, side, activator)
        mu, s = out[:, :D], out[:, D:]
        sd = np.exp(F32(0.5) * s, dtype=F32)
        z = mu + sd * noise
        klw = np.concatenate([np.full(n, one / F32(n), dtype=F32) for n in blocks])[:, None]   # each term a mean
        var1 = (sd * sd if kl_from_std else s * s) + F32(ESP)
        kl = (F32(0.5) * (np.log(var2 / var1, dtype=F32) - one + var1 / var2 + mu * mu / var2) * klw).sum(dtype=F32)
        dvar1 = sd * sd if kl_from_std else F32(2.0) * s
        dkl_mu = klw * mu / var2
        dkl_s = klw * F32(0.5) * (one / var2 - one / var1) * dvar1
        sides[side] = dict(ids=ids, X=X, pre=pre, h=h, mu=mu, s=s, sd=sd, noise=noise, kl=kl, dkl_mu=dkl_mu, dkl_s=dkl_s,
                           e=np.concatenate([z, w[table][ids]], 1), table=table)

    eu_all, ei_all = sides["u"]["e"], sides["i"]["e"]
    eu, nu = eu_all[:B], eu_all[B:].reshape(B, n_neg, 2 * D)
    e1, e2 = ei_all[:B], ei_all[B:2 * B]
    n1 = ei_all[2 * B:2 * B + Bn].reshape(B, n_neg, 2 * D)
    n2 = ei_all[2 * B + Bn:].reshape(B, n_neg, 2 * D)
    zero = np.zeros_like(eu)
    # (vector, what it is scored against as (a, b): a + b) -- vbcar.py:137-159
    partners = {"u": (e1, zero if pos_single else e2), "1": (e2 if pos_single else eu, zero if pos_single else e2),
                "2": (eu, zero if pos_single else e1)}
    vec = {"u": eu, "1": e1, "2": e2}
    negs = {"u": nu, "1": n1, "2": n2}
    gen = F32(0.0)
    d = {k: np.zeros_like(eu) for k in vec}
    dn = {}
    for k in ("u", "1", "2"):
        inp = partners[k][0] + partners[k][1]
        x = (vec[k] * inp).sum(1, dtype=F32)
        y = np.einsum("bnd,bd->bn", negs[k], vec[k]).astype(F32)
        gen = gen + _neg_logsigmoid(x).sum(dtype=F32) + _neg_logsigmoid(-y).sum(dtype=F32)
        dx = (-_sigmoid(-x) * scale)[:, None]
        dy = _sigmoid(y) * scale
        d[k] = d[k] + dx * inp + np.einsum("bn,bnd->bd", dy, negs[k]).astype(F32)
        for j, other in enumerate(partners[k]):      # the gradient flows into whichever vectors made up the partner
            for name, v in vec.items():
                if other is v:
                    d[name] = d[name] + dx * vec[k]
        dn[k] = dy[:, :, None] * vec[k][:, None, :]
    gen = gen * scale
    kld = (sides["u"]["kl"] + sides["i"]["kl"]) * scale
    loss = (one - alpha) * gen + alpha * kld

    de = {"u": np.concatenate([d["u"], dn["u"].reshape(Bn, 2 * D)]),
          "i": np.concatenate([d["1"], d["2"], dn["1"].reshape(Bn, 2 * D), dn["2"].reshape(Bn, 2 * D)])}
    g = {}
    for side, c in sides.items():
        dE = (one - alpha) * de[side]
        dz, dt = dE[:, :D], dE[:, D:]
        dmu = dz + alpha * scale * c["dkl_mu"]
        ds = dz * c["noise"] * F32(0.5) * c["sd"] + alpha * scale * c["dkl_s"]
        dout = np.concatenate([dmu, ds], 1)
        W2 = w[f"fc_{side}_2_mu.weight"]
        g[f"fc_{side}_2_mu.weight"] = dout.T @ c["h"]
        g[f"fc_{side}_2_mu.bias"] = dout.sum(0, dtype=F32)
        dpre = (dout @ W2) * act_grad(c["h"], c["pre"], activator)
        g[f"fc_{side}_1_mu.weight"] = dpre.T @ c["X"]
        g[f"fc_{side}_1_mu.bias"] = dpre.sum(0, dtype=F32)
        gt = np.zeros_like(w[c["table"]])
        np.add.at(gt, c["ids"], dt)
        g[c["table"]] = gt
        c["dout"] = dout
    g = {k: np.asarray(g[k], dtype=F32) for k in KEYS}
    info = {"min_abs_s": float(min(np.abs(sides["u"]["s"]).min(), np.abs(sides["i"]["s"]).min())),
            "dout_u": sides["u"]["dout"], "dout_i": sides["i"]["dout"]}
    return float(loss), float(gen), float(kld), g, info


new_opt_state = mf_numpy.new_opt_state
opt_step = mf_numpy.opt_step


def train_step(w, st, fea, batch, eps, alpha, scale, activator, optimizer, lr):
    loss, gen, kld, g, _ = vbcar_grads(w, fea, batch, eps, alpha, scale, activator)
    opt_step(w, g, st, optimizer, lr)
    return loss, gen, kld
