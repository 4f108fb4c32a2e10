"""Caser (Tang and Wang, WSDM 2018) restated in plain torch ops with autograd, in any dtype: the specification that
csrc/caser.hip is held to (there is no counterpart in the reference).  No tests here.

Ids: items are 1 .. n_items and 0 is padding; users are 0 .. n_users - 1.  Weights are a dict of numpy arrays under the
``state_dict()`` names (``shapes``).  Forward on ``seq [B, L]``, ``users [B]``:

    E       = item_embeddings[seq]                                     [B, L, d]   (row 0 is zero and takes no gradient)
    out_v   = conv_v.bias[c] + sum_l conv_v.weight[c, l] E[b, l, j]    flattened [n_v, d] row-major, NO activation
    pre_h   = conv_h.{h-1}.bias[f] + sum_{i<h} <conv_h.{h-1}.weight[f, i, :], E[b, t + i, :]>,  t = 0 .. L - h
    out_h   = max_t ac_conv(pre_h)                                     [B, n_h] per height h = 1 .. L
    o       = drop([out_v | out_h]);  z = ac_fc(fc1(o));  x = [z | user_embeddings[users]]
    score   = <x, W2[item]> + b2[item]
    loss    = mean over real pos of softplus(-score) + mean over real neg of softplus(score)   (0 = no item; a mean over
              nothing is 0)
    grads   = autograd + l2 * w on EVERY element (Adam's weight_decay); the l2 term is not part of the loss

``defect=`` switches ONE of these off or over (``DEFECTS``); tests/test_caser_host.py shows that the fixtures of
tests/caser_edges.py see each of them."""
import numpy as np
import torch
import torch.nn.functional as Fn

DEFECTS = ("no_conv_v_bias", "act_on_out_v", "mean_pool", "last_window_dropped", "h_before_v", "out_v_transposed",
           "user_first", "no_b2", "one_mean", "zero_target_counted", "pad_row_gets_grad", "no_l2", "l2_touched_rows",
           "no_dropout_scale")
ACT = {"relu": torch.relu, "tanh": torch.tanh, "sigm": torch.sigmoid, "iden": lambda v: v}
TABLES = ("user_embeddings.weight", "item_embeddings.weight", "W2.weight", "b2.weight")


def shapes(U, I, d, L, n_v, n_h):
    out = {"user_embeddings.weight": (U, d), "item_embeddings.weight": (I + 1, d), "conv_v.weight": (n_v, 1, L, 1),
           "conv_v.bias": (n_v,)}
    for i in range(L):
        out[f"conv_h.{i}.weight"] = (n_h, 1, i + 1, d)
        out[f"conv_h.{i}.bias"] = (n_h,)
    out.update({"fc1.weight": (d, n_v * d + n_h * L), "fc1.bias": (d,), "W2.weight": (I + 1, 2 * d),
                "b2.weight": (I + 1, 1)})
    return out


def n_params(U, I, d, L, n_v, n_h):
    return sum(int(np.prod(s)) for s in shapes(U, I, d, L, n_v, n_h).values())


def tensors(w, dtype, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in w.items()}


def seq_len(wt):
    return wt["conv_v.weight"].shape[2]


def features(wt, seq, users, ac_conv="relu", ac_fc="relu", keep=None, p=0.0, defect=None):
    """``(x [B, 2d], pre, fc_pre)``: ``pre[h - 1] [B, n_h, L - h + 1]`` the horizontal pre-activations, ``fc_pre [B, d]``
    fc1's."""
    seq, users = torch.as_tensor(np.asarray(seq)), torch.as_tensor(np.asarray(users))
    table = wt["item_embeddings.weight"]
    if defect != "pad_row_gets_grad":
        table = torch.cat([torch.zeros_like(table[:1]), table[1:]])
    E = table[seq]
    B, L, d = E.shape
    act_c, act_f = ACT[ac_conv], ACT[ac_fc]
    out_v = torch.einsum("cl,blj->bcj", wt["conv_v.weight"][:, 0, :, 0], E)
    if defect != "no_conv_v_bias":
        out_v = out_v + wt["conv_v.bias"][None, :, None]
    if defect == "act_on_out_v":
        out_v = act_c(out_v)
    if defect == "out_v_transposed":
        out_v = out_v.transpose(1, 2)
    out_v = out_v.reshape(B, -1)
    pooled, pre_all = [], []
    for h in range(1, L + 1):
        win = E.unfold(1, h, 1)                                              # [B, L - h + 1, d, h]
        pre = torch.einsum("btki,fik->bft", win, wt[f"conv_h.{h - 1}.weight"][:, 0]) + wt[f"conv_h.{h - 1}.bias"][None, :, None]
        pre_all.append(pre)
        a = act_c(pre)
        if defect == "last_window_dropped" and a.shape[2] > 1:
            a = a[:, :, :-1]
        pooled.append(a.mean(2) if defect == "mean_pool" else a.max(2).values)
    out_h = torch.cat(pooled, 1)
    o = torch.cat([out_h, out_v] if defect == "h_before_v" else [out_v, out_h], 1)
    if keep is not None:
        k = torch.as_tensor(np.asarray(keep)).reshape(o.shape).to(o.dtype)
        o = o * k if defect == "no_dropout_scale" else o * k * (1.0 / (1.0 - p))
    fc_pre = o @ wt["fc1.weight"].T + wt["fc1.bias"]
    z = act_f(fc_pre)
    u = wt["user_embeddings.weight"][users]
    return torch.cat([u, z] if defect == "user_first" else [z, u], 1), pre_all, fc_pre


def scores_of(wt, x, items, defect=None):
    items = torch.as_tensor(np.asarray(items))
    s = torch.einsum("bj,bkj->bk", x, wt["W2.weight"][items])
    return s if defect == "no_b2" else s + wt["b2.weight"][items][..., 0]


def loss_fn(wt, seq, users, pos, neg, ac_conv="relu", ac_fc="relu", keep=None, p=0.0, defect=None):
    x, _, _ = features(wt, seq, users, ac_conv, ac_fc, keep, p, defect)
    pos, neg = torch.as_tensor(np.asarray(pos)), torch.as_tensor(np.asarray(neg))
    lp = Fn.softplus(-scores_of(wt, x, pos, defect))
    ln = Fn.softplus(scores_of(wt, x, neg, defect))
    mp, mn = (pos != 0).to(x.dtype), (neg != 0).to(x.dtype)
    if defect == "zero_target_counted":
        mp, mn = torch.ones_like(mp), torch.ones_like(mn)
    sp, sn, cp, cn = (lp * mp).sum(), (ln * mn).sum(), mp.sum(), mn.sum()
    if defect == "one_mean":
        return (sp + sn) / torch.clamp(cp + cn, min=1.0)
    return sp / torch.clamp(cp, min=1.0) + sn / torch.clamp(cn, min=1.0)


def grads(w, seq, users, pos, neg, ac_conv="relu", ac_fc="relu", l2=0.0, keep=None, p=0.0, dtype=torch.float64,
          defect=None):
    """``(loss, {name: gradient with the l2 term})`` as a float and numpy arrays."""
    wt = tensors(w, dtype, True)
    loss = loss_fn(wt, seq, users, pos, neg, ac_conv, ac_fc, keep, p, defect)
    loss.backward()
    out = {}
    for k, t in wt.items():
        g = torch.zeros_like(t) if t.grad is None else t.grad.clone()
        if defect == "l2_touched_rows" and k in TABLES:
            ids = np.asarray(users) if k == "user_embeddings.weight" else np.concatenate(
                [np.asarray(a).reshape(-1) for a in ((seq,) if k == "item_embeddings.weight" else (pos, neg))])
            rows = torch.zeros(t.shape[0], dtype=torch.bool)
            rows[torch.as_tensor(np.unique(ids))] = True
            g = g + l2 * t.detach() * rows[:, None].to(t.dtype)
        elif defect != "no_l2":
            g = g + l2 * t.detach()
        out[k] = g.numpy()
    return float(loss.detach()), out


def query(w, seq, users, ac_conv="relu", ac_fc="relu", dtype=torch.float64):
    with torch.no_grad():
        return features(tensors(w, dtype), seq, users, ac_conv, ac_fc)[0].numpy()


def next_item_scores(w, seq, users, ac_conv="relu", ac_fc="relu", dtype=torch.float64):
    """Eval-mode scores of the items ``1 .. n_items`` for every row: ``[B, n_items]``."""
    with torch.no_grad():
        wt = tensors(w, dtype)
        x = features(wt, seq, users, ac_conv, ac_fc)[0]
        return (x @ wt["W2.weight"][1:].T + wt["b2.weight"][1:, 0]).numpy()


# ---- torch.optim.Adam's arithmetic on numpy fp32, for the chained-step test.  The gradients above already hold the
# l2 * w term, which is all that Adam(weight_decay=l2) does before its update. --------------------------------------------
def new_opt_state(w):
    return {"step": 0, "exp_avg": {k: np.zeros_like(v, dtype=np.float32) for k, v in w.items()},
            "exp_avg_sq": {k: np.zeros_like(v, dtype=np.float32) for k, v in w.items()}}


def adam_step(w, g, st, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    st["step"] += 1
    f = np.float32
    for k in w:
        gk = np.asarray(g[k], dtype=f).reshape(w[k].shape)
        m, v = st["exp_avg"][k], st["exp_avg_sq"][k]
        m += f(1 - beta1) * (gk - m)
        v *= f(beta2)
        v += f(1 - beta2) * gk * gk
        step_size = f(lr / (1 - beta1 ** st["step"]))
        denom = np.sqrt(v) / f(np.sqrt(1 - beta2 ** st["step"])) + f(eps)
        w[k] = (w[k] - step_size * m / denom).astype(f)
