"""Numpy restatement of beta_rec/models/narm.py (test infrastructure): forward, cross-entropy loss and the analytic
backward (back-propagation through time included) of one ``NARMEngine.train_an_epoch`` iteration, pinned to the real
reference by tests/test_oracle_golden_narm.py.

The working precision is the module global ``F32`` (``helpers.float64_oracle`` turns it into float64).  Weights are a
dict keyed like the reference's ``state_dict``; a batch is ``(seq [T, B] int64 time-major with 0 = padding, target [B],
lens [B])``.  ``keep``: ``None`` or the two dropout keep masks in the reference's call order (input ``[T, B, D]``,
hidden ``[B, 2H]``; either may be ``None``), ``p = (dropout_input, dropout_hidden)`` the rates.

Two deliberately WRONG variants exist for the visibility checks only: ``ht_at_last`` takes ``h_T`` from the padded
output at ``T - 1`` instead of the state after ``lens - 1``; ``mask_from_lens`` takes the attention mask from ``lens``
instead of ``seq > 0``.
"""
import numpy as np

from oracle import mf_numpy

F32 = np.float32


def keys(n_layers):
    out = ["emb.weight"]
    for l in range(n_layers):
        out += [f"gru.weight_ih_l{l}", f"gru.weight_hh_l{l}", f"gru.bias_ih_l{l}", f"gru.bias_hh_l{l}"]
    return tuple(out + ["a_1.weight", "a_2.weight", "v_t.weight", "b.weight"])


def shapes(n_items, D, H, n_layers):
    out = {"emb.weight": (n_items, D)}
    for l in range(n_layers):
        out[f"gru.weight_ih_l{l}"] = (3 * H, D if l == 0 else H)
        out[f"gru.weight_hh_l{l}"] = (3 * H, H)
        out[f"gru.bias_ih_l{l}"] = (3 * H,)
        out[f"gru.bias_hh_l{l}"] = (3 * H,)
    out.update({"a_1.weight": (H, H), "a_2.weight": (H, H), "v_t.weight": (1, H), "b.weight": (2 * H, D)})
    return out


def n_layers_of(w):
    return sum(1 for k in w if k.startswith("gru.weight_hh_l"))


def _sigmoid(x):
    return F32(1.0) / (F32(1.0) + np.exp(-x, dtype=F32))


def _drop(x, keep, i, p):
    if keep is None or keep[i] is None or p[i] == 0.0:
        return x
    return x * np.asarray(keep[i], dtype=F32).reshape(x.shape) * F32(1.0 / (1.0 - p[i]))


def narm_forward(w, seq, lens, keep=None, p=(0.0, 0.0), ht_at_last=False, mask_from_lens=False):
    """``(scores [B, I], cache)``."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    seq, lens = np.asarray(seq), np.asarray(lens)
    T, B = seq.shape
    L = n_layers_of(w)
    H = w["a_1.weight"].shape[0]
    E = w["emb.weight"]
    inp = _drop(E[seq], keep, 0, p)
    layers = []
    for l in range(L):
        W_ih, W_hh = w[f"gru.weight_ih_l{l}"], w[f"gru.weight_hh_l{l}"]
        Gi = inp @ W_ih.T + w[f"gru.bias_ih_l{l}"]
        h = np.zeros((B, H), dtype=F32)
        out = np.zeros((T, B, H), dtype=F32)
        steps = []
        for t in range(T):
            Gh = h @ W_hh.T + w[f"gru.bias_hh_l{l}"]
            r = _sigmoid(Gi[t, :, :H] + Gh[:, :H])
            z = _sigmoid(Gi[t, :, H:2 * H] + Gh[:, H:2 * H])
            hn = Gh[:, 2 * H:]
            n = np.tanh(Gi[t, :, 2 * H:] + r * hn, dtype=F32)
            h_new = (F32(1.0) - z) * n + z * h
            live = (t < lens)[:, None]
            steps.append((r, z, n, hn, h))
            h = np.where(live, h_new, h)
            out[t] = np.where(live, h_new, F32(0.0))
        layers.append((inp, steps, out))
        inp = out
    hT = out[T - 1] if ht_at_last else h
    a1, a2, v = w["a_1.weight"], w["a_2.weight"], w["v_t.weight"][0]
    mask = (np.arange(T)[:, None] < lens[None, :]) if mask_from_lens else (seq > 0)
    mask = mask.astype(F32)[:, :, None]
    q1 = out @ a1.T
    q2 = hT @ a2.T
    s = _sigmoid(q1 + mask * q2[None])
    alpha = s @ v
    c_local = (alpha[:, :, None] * out).sum(0, dtype=F32)
    ct = _drop(np.concatenate([c_local, hT], 1), keep, 1, p)
    Eb = E @ w["b.weight"].T
    scores = ct @ Eb.T
    return scores, dict(w=w, layers=layers, out=out, hT=hT, mask=mask, s=s, alpha=alpha, ct=ct, Eb=Eb, H=H, L=L)


def _log_softmax(scores):
    mx = scores.max(1, keepdims=True)
    e = np.exp(scores - mx, dtype=F32)
    return scores - mx - np.log(e.sum(1, keepdims=True, dtype=F32), dtype=F32)


def narm_loss(w, batch, keep=None, p=(0.0, 0.0), **variant):
    seq, target, lens = batch
    scores, _ = narm_forward(w, seq, lens, keep, p, **variant)
    return float(-_log_softmax(scores)[np.arange(len(target)), np.asarray(target)].mean(dtype=F32))


def narm_grads(w, batch, keep=None, p=(0.0, 0.0), ht_at_last=False, mask_from_lens=False, with_cache=False):
    """``(loss, {name: gradient})`` of ``CrossEntropyLoss()(model(seq, lens), target)``."""
    seq, target, lens = (np.asarray(a) for a in batch)
    T, B = seq.shape
    scores, c = narm_forward(w, seq, lens, keep, p, ht_at_last, mask_from_lens)
    w, H, L = c["w"], c["H"], c["L"]
    logp = _log_softmax(scores)
    loss = -logp[np.arange(B), target].mean(dtype=F32)
    ds = np.exp(logp, dtype=F32)
    ds[np.arange(B), target] -= F32(1.0)
    ds = ds / F32(B)
    E, bw = w["emb.weight"], w["b.weight"]
    g = {}
    dct = ds @ c["Eb"]
    dEb = ds.T @ c["ct"]
    g["b.weight"] = dEb.T @ E
    gE = dEb @ bw
    dct = _drop(dct, keep, 1, p)
    dcl, dhT = dct[:, :H], dct[:, H:]
    out, s, alpha, mask, hT = c["out"], c["s"], c["alpha"], c["mask"], c["hT"]
    a1, a2, v = w["a_1.weight"], w["a_2.weight"], w["v_t.weight"][0]
    dalpha = (dcl[None] * out).sum(-1, dtype=F32)
    dout = alpha[:, :, None] * dcl[None]
    g["v_t.weight"] = (dalpha[:, :, None] * s).sum((0, 1), dtype=F32)[None]
    dpre = dalpha[:, :, None] * v[None, None] * s * (F32(1.0) - s)
    dq2 = (dpre * mask).sum(0, dtype=F32)
    g["a_1.weight"] = dpre.reshape(-1, H).T @ out.reshape(-1, H)
    g["a_2.weight"] = dq2.T @ hT
    dout = dout + dpre @ a1
    dhT = dhT + dq2 @ a2
    if ht_at_last:
        dout[T - 1] += dhT
        dhT = np.zeros_like(dhT)
    for l in range(L - 1, -1, -1):
        inp, steps, _ = c["layers"][l]
        W_ih, W_hh = w[f"gru.weight_ih_l{l}"], w[f"gru.weight_hh_l{l}"]
        dGi = np.zeros((T, B, 3 * H), dtype=F32)
        gW_hh = np.zeros_like(W_hh)
        gb_hh = np.zeros(3 * H, dtype=F32)
        dh = dhT if l == L - 1 else np.zeros((B, H), dtype=F32)    # carried untouched down to step lens - 1
        for t in range(T - 1, -1, -1):
            r, z, n, hn, h_prev = steps[t]
            live = (t < lens)[:, None]
            d = dh + dout[t]
            dn = d * (F32(1.0) - z) * (F32(1.0) - n * n)
            dz = d * (h_prev - n) * z * (F32(1.0) - z)
            dr = dn * hn * r * (F32(1.0) - r)
            dGi[t] = np.where(live, np.concatenate([dr, dz, dn], 1), F32(0.0))
            dGh = np.where(live, np.concatenate([dr, dz, dn * r], 1), F32(0.0))
            gW_hh += dGh.T @ h_prev
            gb_hh += dGh.sum(0, dtype=F32)
            dh = np.where(live, d * z + dGh @ W_hh, dh)
        g[f"gru.weight_ih_l{l}"] = dGi.reshape(T * B, -1).T @ inp.reshape(T * B, -1)
        g[f"gru.weight_hh_l{l}"] = gW_hh
        g[f"gru.bias_ih_l{l}"] = dGi.sum((0, 1), dtype=F32)
        g[f"gru.bias_hh_l{l}"] = gb_hh
        dout = dGi @ W_ih
    dX = _drop(dout, keep, 0, p)
    np.add.at(gE, seq, dX)
    gE[0] = 0                                   # padding_idx = 0, through the lookup and through the arange path
    g["emb.weight"] = gE
    g = {k: np.asarray(g[k], dtype=F32) for k in keys(L)}
    if with_cache:
        c.update(dcl=dcl)
        return float(loss), g, c
    return float(loss), g


def predict(w, user_profile):
    """``NARMEngine.predict``: softmax over all items of the eval-mode scores of one profile, ``[I]``."""
    seq = np.asarray(user_profile, dtype=np.int64)[:, None]
    scores, _ = narm_forward(w, seq, np.array([len(user_profile)]))
    return np.exp(_log_softmax(scores), dtype=F32)[0]


def scores(w, seq, lens):
    """Eval-mode ``model(seq, lens)``: ``[B, I]``."""
    return narm_forward(w, seq, lens)[0]


def step_lr(lr, lr_dc, lr_dc_step, epoch):
    """``StepLR(step_size=lr_dc_step, gamma=lr_dc)`` driven as ``scheduler.step(epoch=epoch)``."""
    return lr * lr_dc ** (epoch // lr_dc_step)


new_opt_state = mf_numpy.new_opt_state
opt_step = mf_numpy.opt_step


def train_step(w, st, batch, optimizer, lr, keep=None, p=(0.0, 0.0)):
    loss, g = narm_grads(w, batch, keep, p)
    opt_step(w, g, st, optimizer, lr)
    return loss
