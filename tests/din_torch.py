"""DIN (Zhou et al., KDD 2018) in plain torch ops with autograd, in float64 or float32, in the naive concatenated form: the
specification csrc/din.hip is held to (there is no counterpart in the reference).  No tests here.

``CASES`` are the shapes of tests/test_din_gpu.py, each named for the kernel edge it is there for.  The fused unit gives a
wave a tile of 16 positions and stages the history in chunks of 64 / 32 / 16 (the smallest that holds the sequence, 64 at
most); a forward workgroup takes 4 candidates of one sequence; the backward runs at most 256 workgroups, each with a slab of
weight partials, and pads the unit's widths to multiples of 16.  Every fixture has a full row (0), a row of one item (1), an
all-padding row (the last), a dead candidate, an item repeated inside row 0 (``T >= 2``) and an item that is both in row 0's
history and its candidate."""
import numpy as np
import torch
import torch.nn.functional as F

N_ITEMS = 60

CASES = {
    "t1_c1": dict(T=1, C=1, D=16, B=5, att=[8, 4], dnn=[8]),                                   # one position, one candidate
    "tile_plus_one": dict(T=17, C=2, D=16, B=4, att=[36, 20], dnn=[12, 8], att_act="prelu", dnn_act="prelu"),  # 16 + 1
    "chunk_plus_one": dict(T=65, C=3, D=32, B=4, att=[16, 16], dnn=[12]),                       # 64 + 1: two chunks
    "long": dict(T=256, C=2, D=16, B=4, att=[20, 12], dnn=[8], att_act="prelu"),                # the longest sequence
    "widest_unit": dict(T=5, C=2, D=16, B=4, att=[128, 128], dnn=[8], att_act="prelu"),         # 8 x 8 weight tiles
    "d128": dict(T=6, C=2, D=128, B=4, att=[36, 20], dnn=[24], dnn_act="prelu"),                # the widest rows
    # every width at its limit: LDS holds a backward chunk of 32 only (two chunks) and att.1.weight is read through L2
    "lds_bound": dict(T=40, C=2, D=128, B=4, att=[128, 128], dnn=[8]),
    "slice_plus_one": dict(T=4, C=5, D=16, B=4, att=[8, 8], dnn=[20, 12, 8]),                   # 4 + 1 candidates, 3 layers
    "slab_plus_one": dict(T=3, C=2, D=16, B=257, att=[8, 8], dnn=[8]),                          # 256 + 1 sequences
    "published": dict(T=50, C=4, D=64, B=6, att=[80, 40], dnn=[200, 80], seed=3),               # the published widths
}


def _act(x, alpha, kind):
    return torch.where(x > 0, x, alpha * x) if kind == "prelu" else torch.sigmoid(x)


def attention(e, q, mask, w, kind):
    """``e [B, T, D]``, ``q [B, C, D]``, ``mask [B, T]`` bool: ``(pooled [B, C, D], a [B, C, T])``."""
    B, T, D = e.shape
    C = q.shape[1]
    qe, ee = q[:, :, None, :].expand(B, C, T, D), e[:, None, :, :].expand(B, C, T, D)
    x = torch.cat([qe, ee, qe - ee, qe * ee], -1)
    h = _act(x @ w["att.0.weight"].T + w["att.0.bias"], w["att.0.alpha"], kind)
    h = _act(h @ w["att.1.weight"].T + w["att.1.bias"], w["att.1.alpha"], kind)
    a = (h @ w["att.2.weight"].T + w["att.2.bias"])[..., 0] / D ** 0.5 * mask[:, None, :].to(e.dtype)
    return torch.einsum("bct,btd->bcd", a, e), a


def logits(w, cfg, seq, cand, running=None, train=True):
    """Logits ``[B, C]`` (0 in dead slots).  ``running``: ``{dnn.l.running_mean / running_var}`` tensors, moved in place when
    training, read in eval."""
    E = w["item_emb.weight"]
    q = E[cand]
    pooled, _ = attention(E[seq], q, seq != 0, w, cfg.get("att_activation", "sigmoid"))
    live = (cand != 0).reshape(-1)
    y = torch.cat([pooled, q, pooled * q], -1).reshape(live.numel(), -1)[live]
    for l in range(len(cfg["dnn_hidden"])):
        y = y @ w[f"dnn.{l}.weight"].T + w[f"dnn.{l}.bias"]
        alpha = w[f"dnn.{l}.alpha"]
        if cfg.get("dnn_activation", "dice") == "prelu":
            y = torch.where(y > 0, y, alpha * y)
        elif y.shape[0]:
            rm, rv = (running[f"dnn.{l}.{n}"] for n in ("running_mean", "running_var")) if running else (None, None)
            p = torch.sigmoid(F.batch_norm(y, rm, rv, None, None, train, 0.1, 1e-8))      # BatchNorm1d(affine=False)
            y = p * y + (1 - p) * alpha * y
    out = torch.zeros(live.numel(), dtype=y.dtype, device=y.device)
    out[live] = (y @ w["out.weight"].T + w["out.bias"])[:, 0]
    return out.view(cand.shape), live


def grads(w_np, cfg, batch, dtype=torch.float64, running=None):
    """``(loss, {name: gradient}, logits [B, C])`` as numpy arrays of ``dtype``; ``running`` (numpy, float32) is updated in
    place as ``BatchNorm1d`` in training mode does."""
    w = {n: torch.tensor(v, dtype=dtype, requires_grad=True) for n, v in w_np.items()}
    seq, cand, label = (torch.as_tensor(np.asarray(a)) for a in batch)
    run = {n: torch.tensor(v, dtype=dtype) for n, v in running.items()} if running else None
    z, live = logits(w, cfg, seq, cand, run, True)
    terms = F.binary_cross_entropy_with_logits(z, label.to(dtype), reduction="none").reshape(-1)
    loss = terms[live].sum() / max(int(live.sum()), 1)
    loss.backward()
    if running:
        for n in running:
            running[n][...] = run[n].numpy()
    g = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).numpy() for n, p in w.items()}
    return float(loss.detach()), g, z.detach().numpy()


def predict(w_np, cfg, seq, cand, running, dtype=torch.float64):
    """Eval-mode logits: Dice reads the running buffers."""
    w = {n: torch.tensor(v, dtype=dtype) for n, v in w_np.items()}
    run = {n: torch.tensor(v, dtype=dtype) for n, v in running.items()} if running else None
    return logits(w, cfg, torch.as_tensor(seq), torch.as_tensor(cand), run, False)[0].numpy()


def make(case, n_cand=None):
    """Seeded fixture of a case: ``(cfg, w, batch, running)``: float32 numpy weights in state_dict() order, ``batch = (seq
    [B, T], cand [B, C], label [B, C])`` and Dice's buffers (an empty dict under ``prelu``)."""
    c = CASES[case]
    # `seed`: the draw under which float32 autograd stays within 1e-5 of float64 for every gradient at its scale (the first
    # draw of `published` leaves d att.2.bias, a sum that cancels, at 1.01e-5)
    rng = np.random.default_rng(sum(map(ord, case)) + c.get("seed", 0))
    T, D, B, I = c["T"], c["D"], c["B"], N_ITEMS
    C = n_cand or c["C"]
    (h1, h2), dnn = c["att"], c["dnn"]
    cfg = {"n_items": I, "emb_dim": D, "maxlen": T, "att_hidden": [h1, h2], "dnn_hidden": list(dnn), "batch_size": B,
           "att_activation": c.get("att_act", "sigmoid"), "dnn_activation": c.get("dnn_act", "dice")}
    shapes = [("att.0", h1, 4 * D), ("att.1", h2, h1), ("att.2", 1, h2)]
    shapes += [(f"dnn.{l}", n, ([3 * D] + list(dnn))[l]) for l, n in enumerate(dnn)] + [("out", 1, dnn[-1])]
    w = {"item_emb.weight": rng.normal(0, 0.5, (I + 1, D))}
    w["item_emb.weight"][0] = 0
    for name, n_out, n_in in shapes:
        w[name + ".weight"] = rng.uniform(-1, 1, (n_out, n_in)) * (3.0 / n_in) ** 0.5
        w[name + ".bias"] = rng.normal(0, 0.1, n_out)
        if name not in ("att.2", "out"):
            w[name + ".alpha"] = rng.uniform(0.1, 0.4, n_out)
    w = {n: v.astype(np.float32) for n, v in w.items()}
    lens = rng.integers(1, T + 1, B)
    lens[0], lens[1], lens[-1] = T, 1, 0
    seq = np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(lens):
        seq[b, T - n:] = rng.integers(1, I + 1, n)
    if T >= 2:
        seq[0, -2] = seq[0, -1]
    cand = rng.integers(1, I + 1, (B, C))
    cand[0, 0] = seq[0, -1]
    cand[2, -1] = 0
    label = (rng.random((B, C)) < 0.5).astype(np.float32)
    running = {}
    if cfg["dnn_activation"] == "dice":
        for l, n in enumerate(dnn):
            running[f"dnn.{l}.running_mean"] = rng.normal(0, 0.1, n).astype(np.float32)
            running[f"dnn.{l}.running_var"] = rng.uniform(0.5, 1.5, n).astype(np.float32)
    return cfg, w, (seq, cand, label), running
