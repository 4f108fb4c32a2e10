"""DIEN (Zhou et al., AAAI 2019) in plain torch ops with autograd, in float64 or float32, a Python loop over the positions: the
specification csrc/dien.hip is held to (there is no counterpart in the reference).  No tests here.

``CASES`` are the shapes of tests/test_dien_gpu.py, each named for the kernel edge it is there for.  A recurrence workgroup
owns 16 rows (sequences in the extractor, (sequence, candidate) pairs in the evolution layer); a sequence whose candidates
straddle two tiles leaves one partial per tile; ``weight_hh`` is LDS-resident up to ``D = 96``; the weight-gradient GEMMs are
cut into K-slices of at least 256 rows; the auxiliary kernels run at most 8 counting blocks of 256 positions and 512 blocks
of 4 waves (2048 positions each way).  Every fixture has a full row (0), a row of one item (1), an all-padding row (the
last), a dead candidate, an item that is in row 0's history and also its candidate, and a ``neg_seq`` with a zero at a live
position (one dropped auxiliary term)."""
import numpy as np
import torch
import torch.nn.functional as F

N_ITEMS = 60

CASES = {
    "t1_c1": dict(T=1, C=1, D=16, B=5, dnn=[8]),                                  # one position, one candidate, no aux term
    "tile_plus_one": dict(T=5, C=3, D=16, B=6, dnn=[12, 8], dnn_act="prelu"),     # 18 rows: sequence 5 straddles two tiles
    "cand_plus_one": dict(T=4, C=17, D=16, B=3, dnn=[8]),                         # more candidates than a tile holds
    "long": dict(T=256, C=2, D=16, B=3, dnn=[8]),                                 # the longest sequence
    "d128_tail": dict(T=6, C=2, D=128, B=4, dnn=[24], dnn_act="prelu"),           # weight_hh's tail rows come through L2
    "d112": dict(T=5, C=3, D=112, B=4, dnn=[12]),                                 # a width that is no multiple of 32
    "grid_plus_one": dict(T=3, C=2, D=16, B=683, dnn=[8]),                        # 2048 + 1 positions; 6 full K-slices
    "published": dict(T=50, C=4, D=32, B=6, dnn=[200, 80]),                       # the published tower, Dice
}


def recurrence(x, mask, w_ih, w_hh, bias, g=None):
    """``x [R, T, D]``, ``mask [R, T]`` bool, ``g [R, T]`` (``None``: 1): the states after every position ``[R, T, D]``."""
    R, T, D = x.shape
    gi = x @ w_ih.T + bias
    h, out = x.new_zeros(R, D), []
    for t in range(T):
        gh = h @ w_hh.T
        r = torch.sigmoid(gi[:, t, :D] + gh[:, :D])
        u = torch.sigmoid(gi[:, t, D:2 * D] + gh[:, D:2 * D])
        n = torch.tanh(gi[:, t, 2 * D:] + r * gh[:, 2 * D:])
        gu = u if g is None else g[:, t, None] * u
        h = torch.where(mask[:, t, None], (1 - gu) * h + gu * n, h)
        out.append(h)
    return torch.stack(out, 1)


def evolve(h1, q, mask, w):
    """``h1 [B, T, D]``, ``q [B, C, D]``, ``mask [B, T]`` bool: ``(hT [B, C, D], a [B, C, T])``."""
    B, T, D = h1.shape
    C = q.shape[1]
    m = mask[:, None, :].expand(B, C, T)
    s = torch.einsum("btd,bcd->bct", h1, q @ w["att.weight"].T)
    top = s.masked_fill(~m, -float("inf")).max(-1, keepdim=True).values
    top = torch.where(torch.isinf(top), torch.zeros_like(top), top)
    e = torch.where(m, torch.exp(torch.where(m, s, top) - top), torch.zeros_like(s))
    a = e / e.sum(-1, keepdim=True).clamp_min(torch.finfo(s.dtype).tiny)
    x = h1[:, None].expand(B, C, T, D).reshape(B * C, T, D)
    hs = recurrence(x, m.reshape(B * C, T), w["evolve.weight_ih"], w["evolve.weight_hh"], w["evolve.bias"], a.reshape(B * C, T))
    return hs[:, -1].view(B, C, D), a


def forward(w, cfg, seq, neg, cand, running=None, train=True):
    """``(logits [B, C] (0 in dead slots), live [B C], L_aux)``."""
    E = w["item_emb.weight"]
    q = E[cand]
    h1 = recurrence(E[seq], seq != 0, w["extractor.weight_ih"], w["extractor.weight_hh"], w["extractor.bias"])
    hT, _ = evolve(h1, q, seq != 0, w)
    live = (cand != 0).reshape(-1)
    y = torch.cat([hT, q, hT * q], -1).reshape(live.numel(), -1)[live]
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
    aux = E.new_zeros(())
    if neg is not None and seq.shape[1] > 1:
        on = (seq[:, :-1] != 0) & (seq[:, 1:] != 0) & (neg[:, 1:] != 0)
        terms = F.softplus(-(h1[:, :-1] * E[seq[:, 1:]]).sum(-1)) + F.softplus((h1[:, :-1] * E[neg[:, 1:]]).sum(-1))
        aux = terms[on].sum() / max(int(on.sum()), 1)
    return out.view(cand.shape), live, aux


def grads(w_np, cfg, batch, dtype=torch.float64, running=None):
    """``(loss, {name: gradient}, logits [B, C])`` as numpy arrays of ``dtype``; ``running`` (numpy, float32) is updated in
    place as ``BatchNorm1d`` in training mode does."""
    w = {n: torch.tensor(v, dtype=dtype, requires_grad=True) for n, v in w_np.items()}
    seq, neg, cand, label = (torch.as_tensor(np.asarray(a)) for a in batch)
    run = {n: torch.tensor(v, dtype=dtype) for n, v in running.items()} if running else None
    z, live, aux = forward(w, cfg, seq, neg, cand, run, True)
    terms = F.binary_cross_entropy_with_logits(z, label.to(dtype), reduction="none").reshape(-1)
    loss = terms[live].sum() / max(int(live.sum()), 1) + cfg.get("aux_weight", 1.0) * aux
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
    return forward(w, cfg, torch.as_tensor(seq), None, torch.as_tensor(cand), run, False)[0].numpy()


def make(case, n_cand=None):
    """Seeded fixture of a case: ``(cfg, w, batch, running)``: float32 numpy weights in state_dict() order, ``batch = (seq
    [B, T], neg_seq [B, T], cand [B, C], label [B, C])`` and Dice's buffers (an empty dict under ``prelu``)."""
    c = CASES[case]
    # `seed`: a draw under which float32 autograd stays within 1e-5 of float64 for every gradient at its scale
    rng = np.random.default_rng(sum(map(ord, case)) + c.get("seed", 0))
    T, D, B, I = c["T"], c["D"], c["B"], N_ITEMS
    C = n_cand or c["C"]
    dnn = c["dnn"]
    cfg = {"n_items": I, "emb_dim": D, "maxlen": T, "dnn_hidden": list(dnn), "batch_size": B, "aux_weight": 0.7,
           "dnn_activation": c.get("dnn_act", "dice")}
    w = {"item_emb.weight": rng.normal(0, 0.5, (I + 1, D))}
    w["item_emb.weight"][0] = 0
    for name in ("extractor", "evolve"):
        if name == "evolve":
            w["att.weight"] = rng.uniform(-1, 1, (D, D)) * (3.0 / D) ** 0.5
        for part in ("weight_ih", "weight_hh"):
            w[f"{name}.{part}"] = rng.uniform(-1, 1, (3 * D, D)) * (3.0 / D) ** 0.5
        w[f"{name}.bias"] = rng.normal(0, 0.1, 3 * D)
    for l, (n_out, n_in) in enumerate(zip(list(dnn) + [1], [3 * D] + list(dnn))):
        name = f"dnn.{l}" if l < len(dnn) else "out"
        w[name + ".weight"] = rng.uniform(-1, 1, (n_out, n_in)) * (3.0 / n_in) ** 0.5
        w[name + ".bias"] = rng.normal(0, 0.1, n_out)
        if name != "out":
            w[name + ".alpha"] = rng.uniform(0.1, 0.4, n_out)
    w = {n: v.astype(np.float32) for n, v in w.items()}
    lens = rng.integers(1, T + 1, B)
    lens[0], lens[1], lens[-1] = T, 1, 0
    seq = np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(lens):
        seq[b, T - n:] = rng.integers(1, I + 1, n)
    neg = rng.integers(1, I, (B, T))
    neg = np.where(seq != 0, neg + (neg >= seq), 0)
    neg[0, -1] = 0
    cand = rng.integers(1, I + 1, (B, C))
    cand[0, 0] = seq[0, -1]
    cand[1 if C > 1 else 2, -1] = 0
    label = (rng.random((B, C)) < 0.5).astype(np.float32)
    running = {}
    if cfg["dnn_activation"] == "dice":
        for l, n in enumerate(dnn):
            running[f"dnn.{l}.running_mean"] = rng.normal(0, 0.1, n).astype(np.float32)
            running[f"dnn.{l}.running_var"] = rng.uniform(0.5, 1.5, n).astype(np.float32)
    return cfg, w, (seq, neg, cand, label), running
