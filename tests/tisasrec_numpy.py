"""Numpy restatement of beta_rec/models/tisasrec.py (test infrastructure): forward, loss and the analytic backward of
``TiSASRecEngine.train_single_batch``, pinned to the real reference by tests/test_oracle_golden_tisasrec.py.

The working precision is the module global ``F32`` (``helpers.float64_oracle`` turns it into float64).  Weights are a
dict keyed like the reference's ``state_dict`` (conv weights ``[D, D, 1]``); a batch is ``(seq, tm, pos, neg)``: ``seq``,
``pos``, ``neg`` ``[B, T]`` int64 with 0 = padding, ``tm`` ``[B, T, T]`` integers in ``[0, time_span]``.  ``keep``:
``None`` or the ``5 + 3 * blocks`` dropout keep masks in the reference's call order (embedding, abs-pos-K, abs-pos-V
``[B, T, D]``; time-K, time-V ``[B, T, T, D]``; per block the attention probabilities ``[H * B, T, T]`` head-major,
dropout1, dropout2 ``[B, T, D]``), ``p`` the rate.

Written as the reference computes, the gathered ``[B, T, T, D]`` tensors included: a padded QUERY row has every score
replaced by ``-2^32 + 1`` and is therefore exactly uniform over all T keys, future ones included; the causal mask uses the
same finite constant; padded KEYS are attended to.
"""
import numpy as np

from oracle import mf_numpy

F32 = np.float32
LN_EPS = 1e-8
PADDING = -(2.0 ** 32) + 1.0
N_FIXED = 5        # keep masks before the per-block ones


def keys(n_blocks):
    out = ["item_emb.weight", "abs_pos_K_emb.weight", "abs_pos_V_emb.weight", "time_matrix_K_emb.weight",
           "time_matrix_V_emb.weight"]
    for b in range(n_blocks):
        out += [f"attention_layernorms.{b}.weight", f"attention_layernorms.{b}.bias"]
    for b in range(n_blocks):
        out += [f"attention_layers.{b}.{m}.{t}" for m in ("Q_w", "K_w", "V_w") for t in ("weight", "bias")]
    for b in range(n_blocks):
        out += [f"forward_layernorms.{b}.weight", f"forward_layernorms.{b}.bias"]
    for b in range(n_blocks):
        out += [f"forward_layers.{b}.conv1.weight", f"forward_layers.{b}.conv1.bias",
                f"forward_layers.{b}.conv2.weight", f"forward_layers.{b}.conv2.bias"]
    return tuple(out + ["last_layernorm.weight", "last_layernorm.bias"])


def shapes(n_items, maxlen, time_span, D, n_blocks):
    out = {}
    for k in keys(n_blocks):
        if k == "item_emb.weight":
            out[k] = (n_items + 1, D)
        elif k.startswith("abs_pos"):
            out[k] = (maxlen, D)
        elif k.startswith("time_matrix"):
            out[k] = (time_span + 1, D)
        elif "_w.weight" in k:
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
    return x * np.asarray(keep[i]).reshape(x.shape).astype(F32) * F32(1.0 / (1.0 - p))


def _heads_first(a, B, H, T):
    """The attention's keep mask is ``[H * B, T, T]`` (the reference concatenates its heads along dim 0)."""
    return a.reshape(H, B, T, T).transpose(1, 0, 2, 3)


def _drop_attn(x, keep, i, p, B, H, T):
    if keep is None or p == 0.0:
        return x
    return x * _heads_first(np.asarray(keep[i]), B, H, T).astype(F32) * F32(1.0 / (1.0 - p))


def tisasrec_forward(w, seq, tm, H, keep=None, p=0.0):
    """``(feats [B, T, D], cache)``: seq2feats, with the keep masks applied when given (training mode)."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    seq, tm = np.asarray(seq), np.asarray(tm).astype(np.int64)
    B, T = seq.shape
    D = w["item_emb.weight"].shape[1]
    nb, hd = n_blocks_of(w), D // H
    live = (seq != 0).astype(F32)[..., None]
    x = _drop(w["item_emb.weight"][seq] * F32(D ** 0.5), keep, 0, p) * live
    pk = _drop(np.broadcast_to(w["abs_pos_K_emb.weight"][:T][None], (B, T, D)), keep, 1, p)
    pv = _drop(np.broadcast_to(w["abs_pos_V_emb.weight"][:T][None], (B, T, D)), keep, 2, p)
    tk = _drop(w["time_matrix_K_emb.weight"][tm], keep, 3, p).reshape(B, T, T, H, hd)
    tv = _drop(w["time_matrix_V_emb.weight"][tm], keep, 4, p).reshape(B, T, T, H, hd)
    masked = ~np.tril(np.ones((T, T), dtype=bool))[None, None] | (seq == 0)[:, None, :, None]     # [B, 1, T, T]
    masked = np.broadcast_to(masked, (B, H, T, T))
    cache = {"blocks": [], "live": live, "tk": tk, "tv": tv, "masked": masked}
    split = lambda a: a.reshape(B, T, H, hd).transpose(0, 2, 1, 3)   # noqa: E731
    for b in range(nb):
        c = {"x": x}
        pre = f"attention_layers.{b}."
        q_in, c["ln_a"] = _ln(x, w[f"attention_layernorms.{b}.weight"], w[f"attention_layernorms.{b}.bias"])
        q = q_in @ w[pre + "Q_w.weight"].T + w[pre + "Q_w.bias"]
        k = x @ w[pre + "K_w.weight"].T + w[pre + "K_w.bias"] + pk
        v = x @ w[pre + "V_w.weight"].T + w[pre + "V_w.bias"] + pv
        qh, kh, vh = split(q), split(k), split(v)
        s = (qh @ kh.transpose(0, 1, 3, 2) + np.einsum("bhic,bijhc->bhij", qh, tk)) * F32(hd ** -0.5)
        s = np.where(masked, F32(PADDING), s)
        e = np.exp(s - s.max(-1, keepdims=True))
        prob = (e / e.sum(-1, keepdims=True, dtype=F32)).astype(F32)
        pd = _drop_attn(prob, keep, N_FIXED + 3 * b, p, B, H, T)
        o = (pd @ vh + np.einsum("bhij,bijhc->bhic", pd, tv)).transpose(0, 2, 1, 3).reshape(B, T, D)
        y = q_in + o
        f, c["ln_f"] = _ln(y, w[f"forward_layernorms.{b}.weight"], w[f"forward_layernorms.{b}.bias"])
        W1, W2 = w[f"forward_layers.{b}.conv1.weight"][:, :, 0], w[f"forward_layers.{b}.conv2.weight"][:, :, 0]
        pre1 = f @ W1.T + w[f"forward_layers.{b}.conv1.bias"]
        h1 = np.maximum(_drop(pre1, keep, N_FIXED + 1 + 3 * b, p), F32(0))
        z = _drop(h1 @ W2.T + w[f"forward_layers.{b}.conv2.bias"], keep, N_FIXED + 2 + 3 * b, p)
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


def tisasrec_loss(w, batch, H, l2_emb, keep=None, p=0.0):
    return tisasrec_grads(w, batch, H, l2_emb, keep, p, backward=False)[0]


def tisasrec_grads(w, batch, H, l2_emb, keep=None, p=0.0, backward=True, with_cache=False):
    """``(loss, gradients keyed like w)`` of tisasrec.py:375-391."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    seq, tm, pos, neg = (np.asarray(a) for a in batch)
    tm = tm.astype(np.int64)
    B, T = seq.shape
    E = w["item_emb.weight"]
    D = E.shape[1]
    nb, hd = n_blocks_of(w), D // H
    feats, cache = tisasrec_forward(w, seq, tm, H, keep, p)
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
    live, tk, tv, masked = cache["live"], cache["tk"], cache["tv"], cache["masked"]
    dpk, dpv = np.zeros((B, T, D), dtype=F32), np.zeros((B, T, D), dtype=F32)
    dtk, dtv = np.zeros(tk.shape, dtype=F32), np.zeros(tv.shape, dtype=F32)
    merge = lambda a: a.transpose(0, 2, 1, 3).reshape(B, T, D)   # noqa: E731
    dx, g["last_layernorm.weight"], g["last_layernorm.bias"] = _ln_bwd(dfeats, cache["ln_l"], w["last_layernorm.weight"])
    for b in range(nb - 1, -1, -1):
        c = cache["blocks"][b]
        pre = f"attention_layers.{b}."
        dpre = dx * live
        dz = _drop(dpre, keep, N_FIXED + 2 + 3 * b, p)
        W1, W2 = w[f"forward_layers.{b}.conv1.weight"][:, :, 0], w[f"forward_layers.{b}.conv2.weight"][:, :, 0]
        g[f"forward_layers.{b}.conv2.weight"] = np.einsum("bto,bti->oi", dz, c["h1"], dtype=F32)[:, :, None]
        g[f"forward_layers.{b}.conv2.bias"] = dz.sum((0, 1), dtype=F32)
        dh1 = (dz @ W2) * (c["h1"] > 0)
        dpre1 = _drop(dh1, keep, N_FIXED + 1 + 3 * b, p)
        g[f"forward_layers.{b}.conv1.weight"] = np.einsum("bto,bti->oi", dpre1, c["f"], dtype=F32)[:, :, None]
        g[f"forward_layers.{b}.conv1.bias"] = dpre1.sum((0, 1), dtype=F32)
        df = dpre1 @ W1 + dpre
        dy, g[f"forward_layernorms.{b}.weight"], g[f"forward_layernorms.{b}.bias"] = _ln_bwd(
            df, c["ln_f"], w[f"forward_layernorms.{b}.weight"])
        do = dy.reshape(B, T, H, hd).transpose(0, 2, 1, 3)
        dvh = c["pd"].transpose(0, 1, 3, 2) @ do
        dtv += np.einsum("bhij,bhic->bijhc", c["pd"], do)
        dpd = do @ c["vh"].transpose(0, 1, 3, 2) + np.einsum("bhic,bijhc->bhij", do, tv)
        dprob = _drop_attn(dpd, keep, N_FIXED + 3 * b, p, B, H, T)
        ds = c["prob"] * (dprob - (dprob * c["prob"]).sum(-1, keepdims=True, dtype=F32))
        ds = np.where(masked, F32(0), ds) * F32(hd ** -0.5)          # torch.where passes no gradient to a masked score
        dqh = ds @ c["kh"] + np.einsum("bhij,bijhc->bhic", ds, tk)
        dkh = ds.transpose(0, 1, 3, 2) @ c["qh"]
        dtk += np.einsum("bhij,bhic->bijhc", ds, c["qh"])
        dq, dk, dv = merge(dqh), merge(dkh), merge(dvh)
        c["dk"] = dk
        dpk += dk
        dpv += dv
        for name, d_out, inp in (("Q_w", dq, c["q_in"]), ("K_w", dk, c["x"]), ("V_w", dv, c["x"])):
            g[pre + name + ".weight"] = np.einsum("bto,bti->oi", d_out, inp, dtype=F32)
            g[pre + name + ".bias"] = d_out.sum((0, 1), dtype=F32)
        dq_in = dq @ w[pre + "Q_w.weight"] + dy
        dx_ln, g[f"attention_layernorms.{b}.weight"], g[f"attention_layernorms.{b}.bias"] = _ln_bwd(
            dq_in, c["ln_a"], w[f"attention_layernorms.{b}.weight"])
        dx = dx_ln + dk @ w[pre + "K_w.weight"] + dv @ w[pre + "V_w.weight"]
    dx0 = _drop(dx * live, keep, 0, p)
    np.add.at(gE, seq, dx0 * F32(D ** 0.5) * live)
    g["abs_pos_K_emb.weight"][:T] = _drop(dpk, keep, 1, p).sum(0, dtype=F32)
    g["abs_pos_V_emb.weight"][:T] = _drop(dpv, keep, 2, p).sum(0, dtype=F32)
    np.add.at(g["time_matrix_K_emb.weight"], tm, _drop(dtk.reshape(B, T, T, D), keep, 3, p))
    np.add.at(g["time_matrix_V_emb.weight"], tm, _drop(dtv.reshape(B, T, T, D), keep, 4, p))
    g = {k: v.astype(F32) for k, v in g.items()}
    if with_cache:
        return float(loss), g, cache
    return float(loss), g


def predict(w, seq, tm, item_indices, H):
    """tisasrec.py:337-360 in eval mode: ``[n_seqs, n_indices]`` logits from the last position's feature."""
    feats, _ = tisasrec_forward(w, seq, tm, H)
    return feats[:, -1, :] @ np.asarray(w["item_emb.weight"], dtype=F32)[np.asarray(item_indices)].T


def time_relation(time_seq, time_span):
    """recommenders/tisasrec.py:108-127 (computeRePos) as the double loop it is, for one ``[T]`` sequence."""
    size = len(time_seq)
    out = np.zeros((size, size), dtype=np.int32)
    for i in range(size):
        for j in range(size):
            out[i, j] = min(abs(int(time_seq[i]) - int(time_seq[j])), time_span)
    return out


new_opt_state = mf_numpy.new_opt_state
opt_step = mf_numpy.opt_step


def train_step(w, st, batch, H, l2_emb, optimizer, lr, keep=None, p=0.0):
    loss, g = tisasrec_grads(w, batch, H, l2_emb, keep, p)
    opt_step(w, g, st, optimizer, lr)
    return loss
