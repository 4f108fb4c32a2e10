"""BERT4Rec restated in plain torch ops on the CPU with autograd (``F.layer_norm``, ``F.gelu``, explicit attention,
``F.cross_entropy``), in float32 or float64: what csrc/bert4rec.hip is held to.  The model has no counterpart in the
reference; include/hiprec.h states it.

``grads(w, seq, labels, heads, keep, p, dtype, defect)`` takes the weight dict keyed like ``state_dict()``, explicit keep
masks (``1 + 3 * blocks`` uint8 arrays: embedding ``[B * T, D]``, per block probabilities ``[B * H, T, T]``, dropout1,
dropout2 ``[B * T, D]``) and returns ``(loss, {name: gradient})``.

``DEFECTS`` names ways of getting the model wrong; tests/test_bert4rec_host.py shows that the fixtures of
tests/bert4rec_edges.py see every one of them.
"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-8
DEFECTS = ("causal", "pad_keys_open", "mask_token_is_a_class", "pad_is_a_class", "no_out_bias", "tanh_gelu",
           "mean_over_all_positions", "pre_ln", "head_without_layernorm", "sqrt_d_scale")


def shapes(I, T, D, nb, Fd):
    """``{name: shape}`` in ``state_dict()`` order."""
    s = {"item_emb.weight": (I + 2, D), "pos_emb.weight": (T, D), "emb_layernorm.weight": (D,), "emb_layernorm.bias": (D,)}
    for b in range(nb):
        s.update({f"attention_layers.{b}.in_proj_weight": (3 * D, D), f"attention_layers.{b}.in_proj_bias": (3 * D,),
                  f"attention_layers.{b}.out_proj.weight": (D, D), f"attention_layers.{b}.out_proj.bias": (D,)})
    for b in range(nb):
        s.update({f"attention_layernorms.{b}.weight": (D,), f"attention_layernorms.{b}.bias": (D,)})
    for b in range(nb):
        s.update({f"forward_layers.{b}.fc1.weight": (Fd, D), f"forward_layers.{b}.fc1.bias": (Fd,),
                  f"forward_layers.{b}.fc2.weight": (D, Fd), f"forward_layers.{b}.fc2.bias": (D,)})
    for b in range(nb):
        s.update({f"forward_layernorms.{b}.weight": (D,), f"forward_layernorms.{b}.bias": (D,)})
    s.update({"head.dense.weight": (D, D), "head.dense.bias": (D,), "head.layernorm.weight": (D,),
              "head.layernorm.bias": (D,), "out_bias": (I + 1,)})
    return s


def keys(nb):
    return tuple(shapes(1, 1, 16, nb, 1))


def n_blocks(w):
    return sum(1 for k in w if k.endswith("in_proj_weight"))


def tensors(w, dtype, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in w.items()}


def _ln(x, w, name):
    return F.layer_norm(x, (x.shape[-1],), w[name + ".weight"], w[name + ".bias"], EPS)


def _drop(x, keep, i, p):
    if keep is None or p == 0.0:
        return x
    k = torch.as_tensor(np.asarray(keep[i]).reshape(tuple(x.shape)), dtype=x.dtype)
    return x * k / (1.0 - p)


def _gelu(x, defect):
    return F.gelu(x, approximate="tanh") if defect == "tanh_gelu" else F.gelu(x)


def forward(w, seq, heads, keep=None, p=0.0, defect=None):
    """``w``: torch tensors; ``seq [B, T]`` int64 numpy.  The last block's output ``[B, T, D]``."""
    seq_t = torch.as_tensor(np.asarray(seq), dtype=torch.int64)
    B, T = seq_t.shape
    D = w["pos_emb.weight"].shape[1]
    hd = D // heads
    e = w["item_emb.weight"][seq_t]
    if defect == "sqrt_d_scale":
        e = e * float(np.sqrt(D))
    x = _ln(e + w["pos_emb.weight"][:T][None], w, "emb_layernorm")
    x = _drop(x.reshape(B * T, D), keep, 0, p).reshape(B, T, D)
    closed = (seq_t == 0)[:, None, None, :].expand(B, heads, T, T)
    if defect == "pad_keys_open":
        closed = torch.zeros_like(closed)
    if defect == "causal":
        closed = closed | torch.triu(torch.ones(T, T, dtype=torch.bool), 1)[None, None]
    for k in range(n_blocks(w)):
        a, f = f"attention_layers.{k}.", f"forward_layers.{k}."

        def mha(inp):
            qkv = inp @ w[a + "in_proj_weight"].T + w[a + "in_proj_bias"]
            q, kk, v = (t.reshape(B, T, heads, hd).transpose(1, 2) for t in qkv.split(D, dim=-1))
            s = (q @ kk.transpose(-1, -2)) / float(np.sqrt(hd))
            s = s.masked_fill(closed, float("-inf"))
            mx = s.amax(-1, keepdim=True)
            mx = torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))
            ex = torch.exp(s - mx).masked_fill(closed, 0.0)
            den = ex.sum(-1, keepdim=True)
            pr = ex / torch.where(den > 0, den, torch.ones_like(den))     # a row with no open key: all zero
            pr = _drop(pr.reshape(B * heads, T, T), keep, 1 + 3 * k, p).reshape(B, heads, T, T)
            o = (pr @ v).transpose(1, 2).reshape(B, T, D)
            out = o @ w[a + "out_proj.weight"].T + w[a + "out_proj.bias"]
            return _drop(out.reshape(B * T, D), keep, 2 + 3 * k, p).reshape(B, T, D)

        def ffn(inp):
            hdn = _gelu(inp @ w[f + "fc1.weight"].T + w[f + "fc1.bias"], defect)
            out = hdn @ w[f + "fc2.weight"].T + w[f + "fc2.bias"]
            return _drop(out.reshape(B * T, D), keep, 3 + 3 * k, p).reshape(B, T, D)

        if defect == "pre_ln":
            x = x + mha(_ln(x, w, f"attention_layernorms.{k}"))
            x = x + ffn(_ln(x, w, f"forward_layernorms.{k}"))
        else:
            x = _ln(x + mha(x), w, f"attention_layernorms.{k}")
            x = _ln(x + ffn(x), w, f"forward_layernorms.{k}")
    return x


def head(w, rows, defect=None):
    h = _gelu(rows @ w["head.dense.weight"].T + w["head.dense.bias"], defect)
    return h if defect == "head_without_layernorm" else _ln(h, w, "head.layernorm")


def loss_fn(w, seq, labels, heads, keep=None, p=0.0, defect=None):
    labels_t = torch.as_tensor(np.asarray(labels), dtype=torch.int64).reshape(-1)
    feats = forward(w, seq, heads, keep, p, defect)
    D = feats.shape[-1]
    I = w["item_emb.weight"].shape[0] - 2
    at = torch.nonzero(labels_t).reshape(-1)
    if at.numel() == 0:
        return feats.sum() * 0.0
    h = head(w, feats.reshape(-1, D)[at], defect)
    lo, hi, bias = 1, I + 1, w["out_bias"][1:]
    if defect == "mask_token_is_a_class":
        hi, bias = I + 2, torch.cat([bias, torch.zeros(1, dtype=bias.dtype)])
    if defect == "pad_is_a_class":
        lo, bias = 0, w["out_bias"]
    logits = h @ w["item_emb.weight"][lo:hi].T
    if defect != "no_out_bias":
        logits = logits + bias
    total = F.cross_entropy(logits, labels_t[at] - lo, reduction="sum")
    return total / (labels_t.numel() if defect == "mean_over_all_positions" else at.numel())


def grads(w, seq, labels, heads, keep=None, p=0.0, dtype=torch.float64, defect=None):
    """``(loss, {name: gradient as numpy})``; a parameter the loss does not reach gets zeros."""
    wt = tensors(w, dtype, requires_grad=True)
    loss = loss_fn(wt, seq, labels, heads, keep, p, defect)
    loss.backward()
    return float(loss.detach()), {k: (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.numpy()) for k, v in wt.items()}


def feats(w, seq, heads, dtype=torch.float64):
    with torch.no_grad():
        return forward(tensors(w, dtype), seq, heads).numpy()


def head_rows(w, rows, dtype=torch.float64):
    with torch.no_grad():
        return head(tensors(w, dtype), torch.as_tensor(np.asarray(rows), dtype=dtype)).numpy()


def next_item_scores(w, seqs, heads, dtype=torch.float64):
    """``[n, n_items]``: ``head(feature of the last position) E[1 : n_items + 1]^T + out_bias[1:]``."""
    with torch.no_grad():
        wt = tensors(w, dtype)
        I = wt["item_emb.weight"].shape[0] - 2
        h = head(wt, forward(wt, seqs, heads)[:, -1, :])
        return (h @ wt["item_emb.weight"][1:I + 1].T + wt["out_bias"][1:]).numpy()


# ---- optimizers for the chained-step tests (torch.optim's arithmetic on numpy fp32) ------------------------------------
def new_opt_state(w, opt):
    st = {"step": 0}
    if opt == "adam":
        st["exp_avg"] = {k: np.zeros_like(v, dtype=np.float32) for k, v in w.items()}
        st["exp_avg_sq"] = {k: np.zeros_like(v, dtype=np.float32) for k, v in w.items()}
    return st


def opt_step(w, g, st, opt, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    st["step"] += 1
    f = np.float32
    for k in w:
        gk = np.asarray(g[k], dtype=f).reshape(w[k].shape)
        if opt == "sgd":
            w[k] = (w[k] - f(lr) * gk).astype(f)
            continue
        m, v = st["exp_avg"][k], st["exp_avg_sq"][k]
        m += f(1 - beta1) * (gk - m)
        v *= f(beta2)
        v += f(1 - beta2) * gk * gk
        step_size = f(lr / (1 - beta1 ** st["step"]))
        denom = np.sqrt(v) / f(np.sqrt(1 - beta2 ** st["step"])) + f(eps)
        w[k] = (w[k] - step_size * m / denom).astype(f)
