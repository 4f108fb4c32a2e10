"""GRU4Rec (Hidasi et al., ICLR 2016; Hidasi and Karatzoglou, CIKM 2018) restated in plain torch ops with autograd, in any
dtype: the specification that csrc/gru4rec.hip is held to (there is no counterpart in the reference).  No tests here.

Ids are ``0 .. n_items - 1``.  Weights are a dict of numpy arrays under the ``state_dict()`` names (``shapes``).  A model
is described by ``cfg``: ``layers`` (hidden sizes), ``D`` (width of ``E``; 0: constrained, the input rows are ``Wy``'s),
``loss`` (``"bpr-max"`` / ``"cross-entropy"``), ``bpreg elu logq alpha`` (loss parameters; ``alpha`` is ``sample_alpha``),
``pe ph`` (dropout rates), ``p`` (every item's share of the training events, or None).  One step on
``batch = (in_items [B], targets [B], reset [B], samples [S])`` from ``state`` (a list of ``[B, H_l]`` arrays):

    x       = drop_e(Wy[in_items] or E[in_items])
    h_prev  = state_l, 0 where reset; a constant of the step
    r, z    = sigmoid(W_i. x + b_i. + W_h. h_prev + b_h.);  n = tanh(W_in x + b_in + r (W_hn h_prev + b_hn))
    h       = (1 - z) n + z h_prev;  out = drop_h(h) is what the next layer reads AND the new state
    R[i, j] = <h_last[i], Wy[cand[j]]> + By[cand[j]],  cand = [targets | samples]; row i's positive is column i
    cross-entropy:  R' = R - shift,  L = - sum_i log(softmax(R'[i, :])[i] + 1e-24)
                    shift[j] = logq log(p[cand[j]]) for targets, logq log(p[cand[j]] ** alpha) for samples
    bpr-max:        R' = elu(R, elu) if elu > 0;  s[i, :] = softmax of R'[i, :] over j != i
                    L = sum_i (-log(sum_{j != i} sigmoid(R'[i,i] - R'[i,j]) s[i,j] + 1e-24) + bpreg sum_{j != i} R'[i,j]^2 s[i,j])

``defect=`` switches ONE of these off or over (``DEFECTS``); tests/test_gru4rec_host.py shows that the fixtures of
tests/gru4rec_edges.py see each of them."""
import numpy as np
import torch
import torch.nn.functional as Fn

DEFECTS = ("state_not_reset", "state_before_dropout", "own_column_in_softmax", "softmax_detached", "no_elu_on_target",
           "bpreg_unweighted", "no_By", "no_shift", "shift_on_bprmax", "mean_loss", "repeats_not_summed", "bhn_outside",
           "gate_order", "no_embed_dropout")
TABLES = ("Wy.weight", "By.weight", "E.weight")


def in_width(cfg):
    return cfg["D"] or cfg["layers"][-1]


def shapes(n_items, layers, D):
    out = {"Wy.weight": (n_items, layers[-1]), "By.weight": (n_items, 1)}
    if D:
        out["E.weight"] = (n_items, D)
    for i, H in enumerate(layers):
        fan_in = layers[i - 1] if i else (D or layers[-1])
        out.update({f"G.{i}.weight_ih": (3 * H, fan_in), f"G.{i}.weight_hh": (3 * H, H), f"G.{i}.bias_ih": (3 * H,),
                    f"G.{i}.bias_hh": (3 * H,)})
    return out


def n_params(n_items, layers, D):
    return sum(int(np.prod(s)) for s in shapes(n_items, layers, D).values())


def tensors(w, dtype, requires_grad=False):
    return {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=requires_grad) for k, v in w.items()}


class _GatherLastWins(torch.autograd.Function):
    """``table[idx]`` whose backward ASSIGNS the rows' gradients: of a repeated id only one contribution survives."""

    @staticmethod
    def forward(ctx, table, idx):
        ctx.save_for_backward(idx)
        ctx.shape = table.shape
        return table[idx]

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        out = g.new_zeros(ctx.shape)
        out[idx] = g
        return out, None


def _ids(a):
    return torch.as_tensor(np.asarray(a, dtype=np.int64))


def forward_step(wt, cfg, in_items, reset, state, keeps=None, defect=None):
    """``(h_last [B, H], new_state)``; ``keeps``: None (eval mode) or ``[embed, hidden_0, ...]`` arrays (None entries: no
    mask)."""
    dtype = wt["Wy.weight"].dtype
    in_items = _ids(in_items)
    B = in_items.numel()
    x = (wt["E.weight"] if cfg["D"] else wt["Wy.weight"])[in_items]
    if keeps is not None and keeps[0] is not None and defect != "no_embed_dropout":
        x = x * torch.as_tensor(np.asarray(keeps[0])).reshape(x.shape).to(dtype) * (1.0 / (1.0 - cfg["pe"]))
    live = torch.ones(B, dtype=dtype) if reset is None else 1.0 - (torch.as_tensor(np.asarray(reset)) != 0).to(dtype)
    new_state = []
    for i, H in enumerate(cfg["layers"]):
        hp = torch.as_tensor(np.asarray(state[i])).to(dtype).detach()
        if defect != "state_not_reset":
            hp = hp * live[:, None]
        gi = x @ wt[f"G.{i}.weight_ih"].T + wt[f"G.{i}.bias_ih"]
        gh = hp @ wt[f"G.{i}.weight_hh"].T
        bh = wt[f"G.{i}.bias_hh"]
        ir, iz, i_n = gi.split(H, 1)
        hr, hz, hn = gh.split(H, 1)
        br, bz, bn = bh.split(H)
        if defect == "gate_order":      # z | r | n
            ir, iz, hr, hz, br, bz = iz, ir, hz, hr, bz, br
        r = torch.sigmoid(ir + hr + br)
        z = torch.sigmoid(iz + hz + bz)
        n = torch.tanh(i_n + r * hn + bn) if defect == "bhn_outside" else torch.tanh(i_n + r * (hn + bn))
        h = (1.0 - z) * n + z * hp
        out = h
        if keeps is not None and keeps[1 + i] is not None:
            out = h * torch.as_tensor(np.asarray(keeps[1 + i])).reshape(h.shape).to(dtype) * (1.0 / (1.0 - cfg["ph"]))
        new_state.append((h if defect == "state_before_dropout" else out).detach())
        x = out
    return x, new_state


def shift_of(cfg, targets, samples, dtype):
    p = torch.as_tensor(np.asarray(cfg["p"], dtype=np.float64))
    return cfg["logq"] * torch.cat([torch.log(p[targets]), torch.log(p[samples] ** cfg["alpha"])]).to(dtype)


def score_block(wt, cfg, h, targets, samples, defect=None):
    """``R [B, B + S]`` before any shift or ELU."""
    cand = torch.cat([_ids(targets), _ids(samples)])
    if defect == "repeats_not_summed":
        O, b = _GatherLastWins.apply(wt["Wy.weight"], cand), _GatherLastWins.apply(wt["By.weight"], cand)[:, 0]
    else:
        O, b = wt["Wy.weight"][cand], wt["By.weight"][cand][:, 0]
    R = h @ O.T
    return R if defect == "no_By" else R + b[None, :]


def loss_of(R, cfg, targets, samples, defect=None):
    B, N = R.shape
    if N < 2:
        raise ValueError("a row needs a negative: B + S >= 2")
    targets, samples = _ids(targets), _ids(samples)
    shifted = cfg["loss"] == "cross-entropy" or defect == "shift_on_bprmax"
    if shifted and cfg["logq"] != 0.0 and cfg["p"] is not None and defect != "no_shift":
        R = R - shift_of(cfg, targets, samples, R.dtype)[None, :]
    if cfg["loss"] == "cross-entropy":
        L = -torch.log(torch.softmax(R, 1).diagonal() + 1e-24).sum()
    else:
        eye = torch.eye(B, N, dtype=torch.bool)
        Rp = R
        if cfg["elu"] > 0:
            Rp = Fn.elu(R, cfg["elu"])
            if defect == "no_elu_on_target":
                Rp = torch.where(eye, R, Rp)
        s = torch.softmax(Rp if defect == "own_column_in_softmax" else Rp.masked_fill(eye, -float("inf")), 1)
        if defect == "softmax_detached":
            s = s.detach()
        off = (~eye).to(R.dtype)
        pos = Rp.diagonal()[:, None]
        A = (torch.sigmoid(pos - Rp) * s * off).sum(1)
        reg = (Rp * Rp * off).sum(1) if defect == "bpreg_unweighted" else (Rp * Rp * s * off).sum(1)
        L = (-torch.log(A + 1e-24) + cfg["bpreg"] * reg).sum()
    return L / B if defect == "mean_loss" else L


def grads(w, cfg, batch, state, keeps=None, dtype=torch.float64, defect=None):
    """``(loss, {name: gradient}, new_state)`` as a float, numpy arrays and a list of numpy arrays."""
    in_items, targets, reset, samples = batch
    wt = tensors(w, dtype, True)
    h, new_state = forward_step(wt, cfg, in_items, reset, state, keeps, defect)
    loss = loss_of(score_block(wt, cfg, h, targets, samples, defect), cfg, targets, samples, defect)
    loss.backward()
    out = {k: (torch.zeros_like(t) if t.grad is None else t.grad).numpy() for k, t in wt.items()}
    return float(loss.detach()), out, [s.numpy() for s in new_state]


def scores_R(w, cfg, batch, state, keeps=None, dtype=torch.float64):
    """The raw score block of a step (what the ELU margin of the fixtures is measured on)."""
    in_items, targets, reset, samples = batch
    with torch.no_grad():
        wt = tensors(w, dtype)
        h, _ = forward_step(wt, cfg, in_items, reset, state, keeps)
        return score_block(wt, cfg, h, targets, samples).numpy()


def step_state(w, cfg, in_items, reset, state, keeps=None, dtype=torch.float64):
    """``(h_last, new_state)`` of one step without a loss (``keeps=None``: the eval step)."""
    with torch.no_grad():
        h, new_state = forward_step(tensors(w, dtype), cfg, in_items, reset, state, keeps)
    return h.numpy(), [s.numpy() for s in new_state]


def zero_state(cfg, B, dtype=np.float64):
    return [np.zeros((B, H), dtype=dtype) for H in cfg["layers"]]


def next_item_scores(w, cfg, profiles, dtype=torch.float64):
    """Eval-mode scores of every item as the event after each profile (a ragged list): ``[n, n_items]``."""
    out = []
    with torch.no_grad():
        wt = tensors(w, dtype)
        for prof in profiles:
            state = zero_state(cfg, 1)
            for item in prof:
                h, state = forward_step(wt, cfg, [item], None, state)
            out.append((h @ wt["Wy.weight"].T + wt["By.weight"][:, 0])[0].numpy())
    return np.stack(out)


# ---- torch.optim.Adam's arithmetic on numpy fp32, for the chained-step test -----------------------------------------------
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
