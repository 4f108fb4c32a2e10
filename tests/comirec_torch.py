"""ComiRec-DR (Cen et al., KDD 2020: ``bilinear_type 2``, ``hard_readout``, no ReLU layer) in plain torch ops with autograd, in
float64 or float32: the specification csrc/comirec.hip is held to (there is no counterpart in the reference).  No tests here.

``CASES`` are the shapes of tests/test_comirec_gpu.py, each named for the kernel edge it is there for: the projection gives a
workgroup 32 sequences and 64 of the ``K D`` columns; the routing deals the positions to ``256 // (K D)`` thread groups and
updates the logits of 16 positions per trip; the backward walks the rows that chose one interest in slabs of 32."""
import numpy as np
import torch

N_ITEMS = 60
MARGIN = 1e-3

CASES = {
    "t1": dict(T=1, K=1, D=16, B=2, R=1, S=3),                    # one position, one interest, one iteration
    "k3_d48": dict(T=5, K=3, D=48, B=4, R=4, S=9, probs=True),    # K no power of two, K D = 144: one column pass, idle threads
    "proj_tile_plus_one": dict(T=3, K=2, D=16, B=33, R=3, S=5),   # one sequence beyond the projection's tile of 32
    "slab_plus_one": dict(T=2, K=1, D=16, B=34, R=3, S=5),        # 33 labelled rows in ONE list: one beyond a backward slab
    "chunk_plus_one": dict(T=17, K=1, D=16, B=3, R=3, S=4),       # 16 position groups, 16 positions per trip: one beyond both
    "published": dict(T=20, K=4, D=64, B=5, R=3, S=70, hit=True),  # the published shape; samples[0] is row 0's target
    "wide": dict(T=4, K=8, D=128, B=3, R=3, S=6),                 # K D = 1024: four column passes, every D / 16 tile
    "long": dict(T=256, K=2, D=16, B=3, R=3, S=6),                # the longest sequence
}


def route(e, W, mask, R):
    """``e [B, T, D]``, ``W [T, K, D, D]``, ``mask [B, T]`` bool: ``(v [B, K, D], c [B, K, T])`` of the last iteration.
    ``uh`` is a constant in every iteration but the last."""
    uh = torch.einsum("tkij,btj->bkti", W, e)
    uh_c = uh.detach()
    b = uh.new_zeros(uh.shape[:3])
    for r in range(R):
        c = torch.softmax(b, 1) * mask[:, None, :].to(uh.dtype)
        s = (c[..., None] * (uh if r == R - 1 else uh_c)).sum(2)
        n = (s * s).sum(-1, keepdim=True)
        v = s * n / (1 + n) / torch.sqrt(n + 1e-9)
        if r < R - 1:
            b = b + (uh_c * v[:, :, None, :]).sum(-1)
    return v, c


def grads(w_np, cfg, batch, dtype=torch.float64, probs=None):
    """``(loss, {name: gradient}, interests [B, K, D], k* [B] (-1: no label), scores [B, n_items] = max_k <v[k], E[i]>)`` as
    numpy arrays of ``dtype``; ``probs [n_items + 1]``: the sampler's distribution for the logQ shift."""
    w = {n: torch.tensor(v, dtype=dtype, requires_grad=True) for n, v in w_np.items()}
    seq, target, samples = (torch.as_tensor(np.asarray(a)) for a in batch)
    E = w["item_emb.weight"]
    v, _ = route(E[seq], w["routing.weight"], seq != 0, cfg["routing_iters"])
    Et = E[target]
    kstar = (v * Et[:, None, :]).sum(-1).detach().argmax(1)
    readout = v[torch.arange(len(target)), kstar]
    z0, zj = (readout * Et).sum(-1), readout @ E[samples].T
    if probs is not None:
        log_q = torch.log(torch.as_tensor(np.asarray(probs), dtype=dtype))
        log_q[0] = 0.0      # the padding id has no probability and no shift: an unlabelled row's terms stay finite
        z0, zj = z0 - log_q[target], zj - log_q[samples][None, :]
    zj = zj.masked_fill(samples[None, :] == target[:, None], -float("inf"))
    terms = torch.logsumexp(torch.cat([z0[:, None], zj], 1), 1) - z0
    lab = target != 0
    loss = terms[lab].sum() / max(int(lab.sum()), 1)
    loss.backward()
    g = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).numpy() for n, p in w.items()}
    kstar = torch.where(lab, kstar, torch.full_like(kstar, -1)).numpy()
    scores = (v.detach() @ E.detach()[1:].T).amax(1).numpy()
    return float(loss.detach()), g, v.detach().numpy(), kstar, scores


def _draw(case, seed):
    c = CASES[case]
    rng = np.random.default_rng(seed)
    T, K, D, B, S, I = c["T"], c["K"], c["D"], c["B"], c["S"], N_ITEMS
    w = {"item_emb.weight": rng.normal(0, 0.5, (I + 1, D)), "routing.weight": rng.normal(0, D ** -0.5, (T, K, D, D))}
    w["item_emb.weight"][0] = 0
    w = {n: v.astype(np.float32) for n, v in w.items()}
    lens = rng.integers(1, T + 1, B)
    lens[0], lens[-1] = T, 0          # row 0 is full, the last row all padding and unlabelled
    if B > 2:
        lens[1] = 1                   # (with T = 1 row 0 is the row of one item as well)
    seq = np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(lens):
        seq[b, T - n:] = rng.integers(1, I + 1, n)
    target, samples = rng.integers(1, I + 1, B), rng.integers(1, I + 1, S)
    target[lens == 0] = 0
    if c.get("hit"):
        samples[0] = target[0]
    probs = None
    if c.get("probs"):
        probs = rng.uniform(0.2, 1.0, I + 1)
        probs[0] = 0.0
        probs /= probs.sum()
    cfg = {"n_items": I, "emb_dim": D, "maxlen": T, "num_interest": K, "routing_iters": c["R"], "batch_size": B}
    return cfg, w, (seq, target, samples), probs


def make(case):
    """Seeded fixture of a case: ``(cfg, w, batch, probs)`` with float32 numpy weights in state_dict() order and ``batch =
    (seq [B, T], target [B], samples [S])``.  Hard readout is an argmax, so the seed is redrawn until, in float64, every
    labelled row's best interest score leads the second best by ``MARGIN`` of its magnitude; no row is ever left out."""
    for seed in range(sum(map(ord, case)), sum(map(ord, case)) + 64):
        cfg, w, batch, probs = _draw(case, seed)
        E = torch.tensor(w["item_emb.weight"], dtype=torch.float64)
        seq, target = torch.as_tensor(batch[0]), torch.as_tensor(batch[1])
        v, _ = route(E[seq], torch.tensor(w["routing.weight"], dtype=torch.float64), seq != 0, cfg["routing_iters"])
        top = (v * E[target][:, None, :]).sum(-1)[target != 0].sort(1, descending=True).values
        if top.shape[1] == 1 or bool((top[:, 0] - top[:, 1] >= MARGIN * top[:, 0].abs()).all()):
            return cfg, w, batch, probs
    raise AssertionError(f"{case}: no seed separates the best interest from the second best")
