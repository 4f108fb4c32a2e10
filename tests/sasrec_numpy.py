"""Numpy restatement of beta_rec/models/sasrec.py (test infrastructure): forward, loss and the analytic backward of
``SASRecEngine.train_single_batch``, pinned to the real reference by tests/test_oracle_golden_sasrec.py.

The working precision is the module global ``F32`` (``helpers.float64_oracle`` turns it into float64).  Weights are a
dict keyed like the reference's ``state_dict`` (conv weights ``[D, D, 1]``); a batch is ``(seq, pos, neg)``, each
``[B, T]`` int64 with 0 = padding.  ``keep``: ``None`` or the ``1 + 3 * blocks`` dropout keep masks in the reference's
call order (embedding; per block the attention probabilities ``[B * H, T, T]``, dropout1, dropout2), ``p`` the rate.
"""
import numpy as np

from oracle import mf_numpy

F32 = np.float32
LN_EPS = 1e-8


def keys(n_blocks):
    out = ["item_emb.weight", "pos_emb.weight"]
    for b in range(n_blocks):
        out += [f"attention_layernorms.{b}.weight", f"attention_layernorms.{b}.bias"]
    for b in range(n_blocks):
        out += [f"attention_layers.{b}.in_proj_weight", f"attention_layers.{b}.in_proj_bias",
                f"attention_layers.{b}.out_proj.weight", f"attention_layers.{b}.out_proj.bias"]
    for b in range(n_blocks):
        out += [f"forward_layernorms.{b}.weight", f"forward_layernorms.{b}.bias"]
    for b in range(n_blocks):
        out += [f"forward_layers.{b}.conv1.weight", f"forward_layers.{b}.conv1.bias",
                f"forward_layers.{b}.conv2.weight", f"forward_layers.{b}.conv2.bias"]
    return tuple(out + ["last_layernorm.weight", "last_layernorm.bias"])


def shapes(n_items, maxlen, D, n_blocks):
    out = {}
    for k in keys(n_blocks):
        if k == "item_emb.weight":
            out[k] = (n_items + 1, D)
        elif k == "pos_emb.weight":
            out[k] = (maxlen, D)
        elif k.endswith("in_proj_weight"):
            out[k] = (3 * D, D)
        elif k.endswith("in_proj_bias"):
            out[k] = (3 * D,)
        elif k.endswith("out_proj.weight"):
            out[k] = (D, D)
        elif "conv" in k and k.endswith("weight"):
            out[k] = (D, D, 1)
        else:
            out[k] = (D,)
    return out


def n_blocks_of(w):
    return sum(1 for k in w if k.startswith("attention_layernorms.") and k.endswith(".weight"))


def _ln(x, gamma, beta):
    mu = x.mean(-1, keepdims=True, dtype=F32)
    c = x - mu
    var = (c * c).mean(-1, keepdims=True, dtype=F32)
    rstd = F32(1.0) / np.sqrt(var + F32(LN_EPS), dtype=F32)
    xh = c * rstd
    return xh * gamma + beta, (xh, rstd)


def _ln_bwd(dy, cache, gamma):
    xh, rstd = cache
    g = dy * gamma
    m1 = g.mean(-1, keepdims=True, dtype=F32)
    m2 = (g * xh).mean(-1, keepdims=True, dtype=F32)
    lead = tuple(range(dy.ndim - 1))
    return rstd * (g - m1 - xh * m2), (dy * xh).sum(lead, dtype=F32), dy.sum(lead, dtype=F32)


def _drop(x, keep, i, p):
    if keep is None or p == 0.0:
        return x
    return x * keep[i].reshape(x.shape).astype(F32) * F32(1.0 / (1.0 - p))


def sasrec_forward(w, seq, H, keep=None, p=0.0, mask_padded_keys=False):
    """``(feats [B, T, D], cache)``: log2feats, with the keep masks applied when given (training mode).
    ``mask_padded_keys``: what the reference does NOT do (its key_padding_mask is commented out) -- the counterfactual
    the tests hold the kernels against: keys at padded positions excluded (a query with no key left keeps them all)."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    seq = np.asarray(seq)
    B, T = seq.shape
    D = w["item_emb.weight"].shape[1]
    nb, hd = n_blocks_of(w), D // H
    live = (seq != 0).astype(F32)[..., None]
    x = w["item_emb.weight"][seq] * F32(D ** 0.5) + w["pos_emb.weight"][:T][None]
    x = _drop(x, keep, 0, p) * live
    cache = {"blocks": [], "live": live}
    tril = np.tril(np.ones((T, T), dtype=bool))
    for b in range(nb):
        c = {"x": x}
        q_in, c["ln_a"] = _ln(x, w[f"attention_layernorms.{b}.weight"], w[f"attention_layernorms.{b}.bias"])
        Wi, bi = w[f"attention_layers.{b}.in_proj_weight"], w[f"attention_layers.{b}.in_proj_bias"]
        q = q_in @ Wi[:D].T + bi[:D]
        k = x @ Wi[D:2 * D].T + bi[D:2 * D]
        v = x @ Wi[2 * D:].T + bi[2 * D:]
        split = lambda a: a.reshape(B, T, H, hd).transpose(0, 2, 1, 3)   # noqa: E731
        qh, kh, vh = split(q) * F32(hd ** -0.5), split(k), split(v)
        s = qh @ kh.transpose(0, 1, 3, 2)
        allowed = np.broadcast_to(tril, s.shape)
        if mask_padded_keys:
            real = allowed & (seq != 0)[:, None, None, :]
            allowed = np.where(real.any(-1, keepdims=True), real, allowed)
        s = np.where(allowed, s, F32(-np.inf))
        e = np.exp(s - s.max(-1, keepdims=True))
        prob = (e / e.sum(-1, keepdims=True, dtype=F32)).astype(F32)
        pd = _drop(prob.reshape(B * H, T, T), keep, 1 + 3 * b, p).reshape(B, H, T, T)
        o = (pd @ vh).transpose(0, 2, 1, 3).reshape(B, T, D)
        mha = o @ w[f"attention_layers.{b}.out_proj.weight"].T + w[f"attention_layers.{b}.out_proj.bias"]
        y = q_in + mha
        f, c["ln_f"] = _ln(y, w[f"forward_layernorms.{b}.weight"], w[f"forward_layernorms.{b}.bias"])
        W1, W2 = w[f"forward_layers.{b}.conv1.weight"][:, :, 0], w[f"forward_layers.{b}.conv2.weight"][:, :, 0]
        pre1 = f @ W1.T + w[f"forward_layers.{b}.conv1.bias"]
        h1 = np.maximum(_drop(pre1, keep, 2 + 3 * b, p), F32(0))
        z = _drop(h1 @ W2.T + w[f"forward_layers.{b}.conv2.bias"], keep, 3 + 3 * b, p)
        c.update(q_in=q_in, qh=qh, kh=kh, vh=vh, prob=prob, pd=pd, o=o, f=f, pre1=pre1, h1=h1)
        x = (f + z) * live
        cache["blocks"].append(c)
    cache["x_last"] = x
    feats, cache["ln_l"] = _ln(x, w["last_layernorm.weight"], w["last_layernorm.bias"])
    return feats, cache


def _softplus(x):
    return np.maximum(x, F32(0)) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    return F32(1.0) / (F32(1.0) + np.exp(-x))


def sasrec_loss(w, batch, H, l2_emb, keep=None, p=0.0, mask_padded_keys=False):
    return sasrec_grads(w, batch, H, l2_emb, keep, p, backward=False, mask_padded_keys=mask_padded_keys)[0]


def sasrec_grads(w, batch, H, l2_emb, keep=None, p=0.0, backward=True, with_cache=False, mask_padded_keys=False):
    """``(loss, gradients keyed like w)`` of sasrec.py:205-221."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    seq, pos, neg = (np.asarray(a) for a in batch)
    B, T = seq.shape
    E = w["item_emb.weight"]
    D = E.shape[1]
    nb, hd = n_blocks_of(w), D // H
    assert not (backward and mask_padded_keys), "the counterfactual is forward only"
    feats, cache = sasrec_forward(w, seq, H, keep, p, mask_padded_keys)
    valid = pos != 0
    n = F32(valid.sum())
    ep, en = E[pos], E[neg]
    pl, nl = (feats * ep).sum(-1, dtype=F32), (feats * en).sum(-1, dtype=F32)
    norm = np.sqrt((E * E).sum(dtype=F32), dtype=F32)
    loss = (_softplus(-pl)[valid].sum(dtype=F32) + _softplus(nl)[valid].sum(dtype=F32)) / n + F32(l2_emb) * norm
    if not backward:
        return float(loss), None
    g = {k: np.zeros_like(v) for k, v in w.items()}
    dpl = np.where(valid, -_sigmoid(-pl), F32(0)) / n
    dnl = np.where(valid, _sigmoid(nl), F32(0)) / n
    dfeats = dpl[..., None] * ep + dnl[..., None] * en
    gE = g["item_emb.weight"]
    np.add.at(gE, pos, dpl[..., None] * feats)
    np.add.at(gE, neg, dnl[..., None] * feats)
    gE[0] = 0                     # padding_idx: no lookup gradient reaches row 0
    if norm > 0:
        gE += F32(l2_emb) * E / norm
    live = cache["live"]
    dx, g["last_layernorm.weight"], g["last_layernorm.bias"] = _ln_bwd(dfeats, cache["ln_l"], w["last_layernorm.weight"])
    for b in range(nb - 1, -1, -1):
        c = cache["blocks"][b]
        dpre = dx * live
        dz = _drop(dpre, keep, 3 + 3 * b, p)
        W1, W2 = w[f"forward_layers.{b}.conv1.weight"][:, :, 0], w[f"forward_layers.{b}.conv2.weight"][:, :, 0]
        g[f"forward_layers.{b}.conv2.weight"] = np.einsum("bto,bti->oi", dz, c["h1"], dtype=F32)[:, :, None]
        g[f"forward_layers.{b}.conv2.bias"] = dz.sum((0, 1), dtype=F32)
        dh1 = (dz @ W2) * (c["h1"] > 0)
        dpre1 = _drop(dh1, keep, 2 + 3 * b, p)
        g[f"forward_layers.{b}.conv1.weight"] = np.einsum("bto,bti->oi", dpre1, c["f"], dtype=F32)[:, :, None]
        g[f"forward_layers.{b}.conv1.bias"] = dpre1.sum((0, 1), dtype=F32)
        df = dpre1 @ W1 + dpre
        dy, g[f"forward_layernorms.{b}.weight"], g[f"forward_layernorms.{b}.bias"] = _ln_bwd(
            df, c["ln_f"], w[f"forward_layernorms.{b}.weight"])
        Wo = w[f"attention_layers.{b}.out_proj.weight"]
        g[f"attention_layers.{b}.out_proj.weight"] = np.einsum("bto,bti->oi", dy, c["o"], dtype=F32)
        g[f"attention_layers.{b}.out_proj.bias"] = dy.sum((0, 1), dtype=F32)
        do = (dy @ Wo).reshape(B, T, H, hd).transpose(0, 2, 1, 3)
        dvh = c["pd"].transpose(0, 1, 3, 2) @ do
        dpd = do @ c["vh"].transpose(0, 1, 3, 2)
        dprob = _drop(dpd.reshape(B * H, T, T), keep, 1 + 3 * b, p).reshape(B, H, T, T)
        ds = c["prob"] * (dprob - (dprob * c["prob"]).sum(-1, keepdims=True, dtype=F32))
        dqh = (ds @ c["kh"]) * F32(hd ** -0.5)
        dkh = ds.transpose(0, 1, 3, 2) @ c["qh"]
        merge = lambda a: a.transpose(0, 2, 1, 3).reshape(B, T, D)   # noqa: E731
        dq, dk, dv = merge(dqh), merge(dkh), merge(dvh)
        Wi = w[f"attention_layers.{b}.in_proj_weight"]
        g[f"attention_layers.{b}.in_proj_weight"] = np.concatenate([
            np.einsum("bto,bti->oi", dq, c["q_in"], dtype=F32), np.einsum("bto,bti->oi", dk, c["x"], dtype=F32),
            np.einsum("bto,bti->oi", dv, c["x"], dtype=F32)])
        g[f"attention_layers.{b}.in_proj_bias"] = np.concatenate([a.sum((0, 1), dtype=F32) for a in (dq, dk, dv)])
        dq_in = dq @ Wi[:D] + dy
        dx_ln, g[f"attention_layernorms.{b}.weight"], g[f"attention_layernorms.{b}.bias"] = _ln_bwd(
            dq_in, c["ln_a"], w[f"attention_layernorms.{b}.weight"])
        dx = dx_ln + dk @ Wi[D:2 * D] + dv @ Wi[2 * D:]
    dx0 = _drop(dx * live, keep, 0, p)
    np.add.at(gE, seq, dx0 * F32(D ** 0.5) * live)
    g["pos_emb.weight"][:T] = dx0.sum(0, dtype=F32)
    g = {k: v.astype(F32) for k, v in g.items()}
    if with_cache:
        return float(loss), g, cache
    return float(loss), g


def predict(w, seq, item_indices, H):
    """sasrec.py:167-190 in eval mode: ``[n_seqs, n_indices]`` logits from the last position's feature."""
    feats, _ = sasrec_forward(w, seq, H)
    return feats[:, -1, :] @ np.asarray(w["item_emb.weight"], dtype=F32)[np.asarray(item_indices)].T


new_opt_state = mf_numpy.new_opt_state
opt_step = mf_numpy.opt_step


def train_step(w, st, batch, H, l2_emb, optimizer, lr, keep=None, p=0.0):
    loss, g = sasrec_grads(w, batch, H, l2_emb, keep, p)
    opt_step(w, g, st, optimizer, lr)
    return loss
