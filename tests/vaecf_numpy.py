"""Numpy restatement of VAECF / Mult-VAE (test infrastructure): forward, loss, the analytic backward and the optimizer
step of one ``VAECFEngine.train_single_batch``, written from the model's mathematics and pinned to the real reference by
tests/test_oracle_golden_vaecf.py.

    h_0 = x,  h_l = act(h_{l-1} W_l^T + b_l)                        encoder, l = 1 .. n
    mu = h_n W_mu^T + b_mu,  logvar = h_n W_lv^T + b_lv,  std = exp(logvar / 2),  z = mu + eps std
    d_0 = z,  d_l = act(d_{l-1} V_l^T + c_l) (l = 1 .. n),  logits = d_n V_{n+1}^T + c_{n+1}
    p = softmax(logits) (mult) or sigmoid(logits);  ll_b = sum_j of
        mult x log(p + EPS) | bern x log(p + EPS) + (1 - x) log(1 - p + EPS) | gaus -(x - p)^2 | pois x log(p + EPS) - p
    kld_b = -1/2 sum (1 + 2 log std - mu^2 - std^2)
    loss = mean_b(beta kld_b - ll_b) over the rows of the batch

The working precision is the module global ``F32`` (``helpers.float64_oracle`` turns it into float64).  Weights are a dict
keyed like the reference's ``state_dict`` (:func:`keys`); ``x`` is the dense ``[B, n_items]`` batch (dense here only:
this is the yardstick, not the product), ``eps`` the ``[B, z_dim]`` noise.

Deliberately WRONG variants exist for the visibility checks only: ``no_eps`` leaves EPS out of the logs;
``kl_from_logvar`` takes the KL's std from ``exp(logvar)`` (logvar where log std = logvar / 2 belongs); ``mean_over``
divides by another row count than the batch's; ``drop_sparse`` leaves the ``x`` term out of d loss / d logits (the dense
``x = 0`` gradient alone); ``decay_after`` of :func:`opt_step` applies the weight decay to the stepped weights, not into
the gradient.
"""
import numpy as np

from oracle import mf_numpy

F32 = np.float32
EPS = 1e-10
ACTS = ("sigmoid", "tanh", "relu", "relu6")
LIKS = ("mult", "bern", "gaus", "pois")


def keys(n_hidden):
    out = []
    for l in range(n_hidden):
        out += [f"encoder.fc{l}.weight", f"encoder.fc{l}.bias"]
    out += ["enc_mu.weight", "enc_mu.bias", "enc_logvar.weight", "enc_logvar.bias"]
    for l in range(n_hidden + 1):
        out += [f"decoder.fc{l}.weight", f"decoder.fc{l}.bias"]
    return tuple(out)


def shapes(n_items, hidden, z_dim):
    """``{name: shape}`` in ``state_dict`` order for ``ae_structure = [n_items] + hidden``."""
    enc = [n_items] + list(hidden)
    dec = [z_dim] + enc[::-1]
    out = {}
    for l in range(len(hidden)):
        out[f"encoder.fc{l}.weight"], out[f"encoder.fc{l}.bias"] = (enc[l + 1], enc[l]), (enc[l + 1],)
    for name in ("enc_mu", "enc_logvar"):
        out[name + ".weight"], out[name + ".bias"] = (z_dim, enc[-1]), (z_dim,)
    for l in range(len(dec) - 1):
        out[f"decoder.fc{l}.weight"], out[f"decoder.fc{l}.bias"] = (dec[l + 1], dec[l]), (dec[l + 1],)
    return out


def n_hidden_of(w):
    return sum(1 for k in w if k.startswith("encoder.") and k.endswith(".weight"))


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).astype(x.dtype)


def act(x, name):
    if name == "sigmoid":
        return _sigmoid(x)
    if name == "tanh":
        return np.tanh(x)
    if name == "relu":
        return np.maximum(x, 0).astype(x.dtype)
    if name == "relu6":
        return np.minimum(np.maximum(x, 0), 6).astype(x.dtype)
    raise ValueError(name)


def act_grad(h, pre, name):
    if name == "sigmoid":
        return h * (1 - h)
    if name == "tanh":
        return 1 - h * h
    if name == "relu":
        return (pre > 0).astype(h.dtype)
    return ((pre > 0) & (pre < 6)).astype(h.dtype)


def csr_of(x):
    """``(row_ptr, items, values)`` of a dense batch: int64, int64, fp32."""
    x = np.asarray(x)
    rows, cols = np.nonzero(x)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=x.shape[0]))]).astype(np.int64)
    return row_ptr, cols.astype(np.int64), x[rows, cols].astype(np.float32)


def dense_of(row_ptr, items, values, n_items):
    x = np.zeros((len(row_ptr) - 1, n_items), dtype=np.float32)
    for b in range(len(row_ptr) - 1):
        np.add.at(x[b], items[row_ptr[b]:row_ptr[b + 1]], values[row_ptr[b]:row_ptr[b + 1]])
    return x


def encode(w, x, activation):
    """``(mu, logvar, [pre-activations], [activations])`` of the encoder."""
    h, pres, hs = np.asarray(x, dtype=F32), [], []
    for l in range(n_hidden_of(w)):
        pre = h @ w[f"encoder.fc{l}.weight"].T + w[f"encoder.fc{l}.bias"]
        h = act(pre, activation)
        pres.append(pre), hs.append(h)
    return (h @ w["enc_mu.weight"].T + w["enc_mu.bias"], h @ w["enc_logvar.weight"].T + w["enc_logvar.bias"], pres, hs)


def decode_hidden(w, z, activation):
    """``([pre-activations], [activations])`` of the decoder's hidden layers; the last activation is ``Hd``."""
    d, pres, ds = z, [], []
    for l in range(n_hidden_of(w)):
        pre = d @ w[f"decoder.fc{l}.weight"].T + w[f"decoder.fc{l}.bias"]
        d = act(pre, activation)
        pres.append(pre), ds.append(d)
    return pres, ds


def probabilities(logits, likelihood):
    if likelihood == "mult":
        e = np.exp(logits - logits.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)
    return _sigmoid(logits)


def decode(w, z, activation, likelihood):
    """``(p [B, n_items], Hd, logits)``."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    n = n_hidden_of(w)
    hd = decode_hidden(w, np.asarray(z, dtype=F32), activation)[1][-1]
    logits = hd @ w[f"decoder.fc{n}.weight"].T + w[f"decoder.fc{n}.bias"]
    return probabilities(logits, likelihood), hd, logits


def predict_scores(w, x, activation, likelihood):
    """What ``score`` returns: ``decode(mu(x))`` as ``[rows, n_items]``, plus ``Hd(mu(x))``."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    mu = encode(w, x, activation)[0]
    p, hd, _ = decode(w, mu, activation, likelihood)
    return p, hd


def reference_predict(w, users, items, n_users, n_items, activation, likelihood):
    """The reference's ``predict`` taken literally: ``x_u`` built from the query pairs themselves (duplicates summed),
    ``decode(mu(x_u))`` flattened and indexed with the item ids -- row 0's probabilities at ``items``."""
    x = np.zeros((n_users, n_items), dtype=np.float32)
    np.add.at(x, (np.asarray(users), np.asarray(items)), 1.0)
    return predict_scores(w, x, activation, likelihood)[0].ravel()[np.asarray(items)]


def vaecf_grads(w, x, eps, beta, activation, likelihood, no_eps=False, kl_from_logvar=False, mean_over=None,
                drop_sparse=False):
    """``(loss, mean ll, mean kld, {name: gradient}, info)`` of one forward + loss and its backward."""
    w = {k: np.asarray(v, dtype=F32) for k, v in w.items()}
    x, eps = np.asarray(x, dtype=F32), np.asarray(eps, dtype=F32)
    n = n_hidden_of(w)
    B = x.shape[0]
    rows = B if mean_over is None else mean_over
    E = 0.0 if no_eps else EPS
    if likelihood not in LIKS:
        raise ValueError(likelihood)

    mu, lv, pre_e, h_e = encode(w, x, activation)
    sd = np.exp(0.5 * lv)
    z = mu + eps * sd
    pre_d, h_d = decode_hidden(w, z, activation)
    hd = h_d[-1]
    logits = hd @ w[f"decoder.fc{n}.weight"].T + w[f"decoder.fc{n}.bias"]
    p = probabilities(logits, likelihood)
    xs = np.zeros_like(x) if drop_sparse else x       # the x the GRADIENT sees
    if likelihood == "mult":
        ll = x * np.log(p + E)
        dll_dp = xs / (p + E)
        if drop_sparse:                                # the dense term p c_b alone
            dlogit_ll = -p * (x * p / (p + E)).sum(1, keepdims=True)
        else:
            dlogit_ll = p * (dll_dp - (p * dll_dp).sum(1, keepdims=True))
    else:
        if likelihood == "bern":
            ll = x * np.log(p + E) + (1 - x) * np.log(1 - p + E)
            dll_dp = xs / (p + E) - (1 - xs) / (1 - p + E)
        elif likelihood == "gaus":
            ll = -((x - p) ** 2)
            dll_dp = 2 * (xs - p)
        else:
            ll = x * np.log(p + E) - p
            dll_dp = xs / (p + E) - 1
        dlogit_ll = dll_dp * p * (1 - p)
    ll_b = ll.sum(1)
    s_kl = np.exp(lv) if kl_from_logvar else sd
    kld_b = (-0.5 * (1 + 2 * np.log(s_kl) - mu * mu - s_kl * s_kl)).sum(1)
    ll_mean, kld_mean = ll_b.sum() / rows, kld_b.sum() / rows
    loss = beta * kld_mean - ll_mean

    g = {}
    dlogit = (-dlogit_ll / rows).astype(x.dtype)
    g[f"decoder.fc{n}.weight"] = dlogit.T @ hd
    g[f"decoder.fc{n}.bias"] = dlogit.sum(0)
    dh = dlogit @ w[f"decoder.fc{n}.weight"]
    for l in range(n - 1, -1, -1):
        dpre = dh * act_grad(h_d[l], pre_d[l], activation)
        g[f"decoder.fc{l}.weight"] = dpre.T @ (z if l == 0 else h_d[l - 1])
        g[f"decoder.fc{l}.bias"] = dpre.sum(0)
        dh = dpre @ w[f"decoder.fc{l}.weight"]
    dz = dh
    dmu = dz + (beta / rows) * mu
    dkl_dlv = (s_kl * s_kl - 1) if kl_from_logvar else 0.5 * (sd - 1 / sd) * sd
    dlv = dz * eps * 0.5 * sd + (beta / rows) * dkl_dlv
    g["enc_mu.weight"], g["enc_mu.bias"] = dmu.T @ h_e[-1], dmu.sum(0)
    g["enc_logvar.weight"], g["enc_logvar.bias"] = dlv.T @ h_e[-1], dlv.sum(0)
    dh = dmu @ w["enc_mu.weight"] + dlv @ w["enc_logvar.weight"]
    for l in range(n - 1, -1, -1):
        dpre = dh * act_grad(h_e[l], pre_e[l], activation)
        g[f"encoder.fc{l}.weight"] = dpre.T @ (x if l == 0 else h_e[l - 1])
        g[f"encoder.fc{l}.bias"] = dpre.sum(0)
        dh = dpre @ w[f"encoder.fc{l}.weight"]
    g = {k: np.asarray(g[k], dtype=F32) for k in keys(n)}
    pres = np.concatenate([a.ravel() for a in pre_e + pre_d])
    info = {"min_abs_pre": float(np.abs(pres).min()), "min_abs_pre_minus_6": float(np.abs(pres - 6).min()),
            "max_abs_logvar": float(np.abs(lv).max()), "max_abs_z": float(np.abs(z).max()), "mu": mu, "logvar": lv,
            "hd": hd, "p": p, "logits": logits}
    return float(loss), float(ll_mean), float(kld_mean), g, info


new_opt_state = mf_numpy.new_opt_state


def opt_step(w, g, st, lr, weight_decay=0.0, decay_after=False):
    """``torch.optim.Adam(lr, weight_decay)``: the decay is L2 into the gradient, ``g + weight_decay w``."""
    if weight_decay and not decay_after:
        g = {k: (g[k] + F32(weight_decay) * w[k]).astype(w[k].dtype) for k in w}
    before = {k: v.copy() for k, v in w.items()} if decay_after else None
    mf_numpy.opt_step(w, g, st, "adam", lr)
    if decay_after:
        for k in w:
            w[k] -= F32(lr * weight_decay) * before[k]


def train_step(w, st, x, eps, beta, activation, likelihood, lr, weight_decay=0.0):
    loss, ll, kld, g, _ = vaecf_grads(w, x, eps, beta, activation, likelihood)
    opt_step(w, g, st, lr, weight_decay)
    return loss, ll, kld
