"""HSTU (Zhai et al., ICML 2024) as this project states it, in plain torch ops with autograd, in float64 or float32: the
specification csrc/hstu.hip is held to (there is no counterpart in the reference).  No tests here.

``CASES`` are the shapes of tests/test_hstu_gpu.py, each named for the edge it is there for: the attention kernels own 32
queries (or 32 keys) per workgroup and walk the keys in chunks of 64; the bias gradients are folded over the
``B * H * ceil(T / 32)`` workgroup slabs in ``FOLD_SEGS`` segments."""
import math

import numpy as np
import torch
import torch.nn.functional as F

FOLD_SEGS = 64
EPS = 1e-6
LOG_BASE = 0.301
GAPS = (0, 1, 2, 3, 11, 12, 1000, 10**6)

# T, D, H, dqk, dv; optional B (4), nb (2), maxlen (T), num_buckets (32), rel_bias
CASES = {
    # one key per row.  Two heads: with one, LN_noaffine(a * v) does not depend on a, the true bias gradients are ~ 0 and
    # float32 cannot hold them to 1e-5 of their scale (7e-5 in the restatement itself)
    "t1": dict(T=1, D=16, H=2, dqk=16, dv=16),
    "below_tile": dict(T=31, D=32, H=2, dqk=16, dv=16),
    "tile_exact_dqk_ne_dv": dict(T=32, D=32, H=1, dqk=32, dv=16),
    "tile_plus_one": dict(T=33, D=48, H=2, dqk=16, dv=32),
    "chunk_exact_few_buckets": dict(T=64, D=64, H=4, dqk=16, dv=16, num_buckets=8),      # the clamp at 8 is hit often
    "chunk_plus_one_wide": dict(T=65, D=64, H=1, dqk=64, dv=64),
    "short_of_maxlen": dict(T=200, D=64, H=2, dqk=32, dv=32, maxlen=256),                # N != T: the 1 / N, the offset
    "max_len_heads8": dict(T=256, D=128, H=8, dqk=16, dv=16, nb=1),
    "pos_only": dict(T=40, D=32, H=2, dqk=16, dv=32, rel_bias="pos"),
    # 67 slabs over 64 segments: segments of two slabs, the last of one, the rest empty
    "fold_seams": dict(T=8, D=16, H=1, dqk=16, dv=16, B=FOLD_SEGS + 3),
}
# for the attention stage alone, which does not go through the gated norm: the issue's T = 1 shape with ONE head
STAGE_ONLY = {"t1_one_head": dict(T=1, D=16, H=1, dqk=16, dv=16)}
N_ITEMS = 50


def make(case):
    """Seeded fixture of a case: ``(cfg, w, batch)`` with float32 numpy weights in state_dict() order and ``batch =
    (u, seq, time_seq, pos, neg)``, each ``[B, T]`` (no ``time_seq`` with ``rel_bias="pos"``).  Row 0 is full, row 1 holds
    one item, row 2 is all padding and unlabelled, the others have random lengths.  Weights are drawn far larger than the
    init; time stamps are non-decreasing with gaps from ``GAPS``."""
    c = CASES.get(case) or STAGE_ONLY[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    T, D, H, dq, dv, I = c["T"], c["D"], c["H"], c["dqk"], c["dv"], N_ITEMS
    B, nb, N, nbk, rel = c.get("B", 4), c.get("nb", 2), c.get("maxlen", T), c.get("num_buckets", 32), c.get("rel_bias", "pos_time")
    ln = lambda p: {p + ".weight": rng.uniform(0.5, 1.5, D), p + ".bias": rng.normal(0, 0.3, D)}      # noqa: E731
    w = {"item_emb.weight": rng.normal(0, 0.3, (I + 1, D)), "pos_emb.weight": rng.normal(0, 1.0, (N, D))}
    w["item_emb.weight"][0] = 0
    for b in range(nb):
        p = f"blocks.{b}."
        w.update(ln(p + "norm"))
        w[p + "uvqk"] = rng.normal(0, 1 / np.sqrt(D), (D, 2 * H * (dv + dq)))
        w[p + "pos_w"] = rng.normal(0, 0.5, 2 * N - 1)
        if rel == "pos_time":
            w[p + "ts_w"] = rng.normal(0, 0.5, nbk + 1)
        w[p + "o.weight"], w[p + "o.bias"] = rng.normal(0, 1 / np.sqrt(H * dv), (D, H * dv)), rng.normal(0, 0.1, D)
    w.update(ln("last_norm"))
    w = {n: v.astype(np.float32) for n, v in w.items()}
    lens = rng.integers(1, T + 1, B)
    lens[:3] = T, 1, 0
    seq, ts = np.zeros((B, T), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(lens):
        seq[b, T - n:] = rng.integers(1, I + 1, n)
        ts[b, T - n:] = 1_600_000_000 + np.cumsum(rng.choice(GAPS, n))
    pos = np.where(seq != 0, rng.integers(1, I + 1, (B, T)), 0)
    neg = np.where(seq != 0, rng.integers(1, I + 1, (B, T)), 0)
    cfg = {"n_users": B, "n_items": I, "emb_dim": D, "maxlen": N, "num_blocks": nb, "num_heads": H, "attention_dim": dq,
           "linear_dim": dv, "num_buckets": nbk, "rel_bias": rel, "dropout_rate": 0.0, "batch_size": B, "l2_emb": 1e-3}
    u = np.arange(B)
    return cfg, w, ((u, seq, ts, pos, neg) if rel == "pos_time" else (u, seq, pos, neg))


def buckets(ts, num_buckets):
    """``[B, T, T]`` int64 from time stamps ``[B, T]``: the published formula itself, in float64."""
    te = torch.cat([ts[:, 1:], ts[:, -1:]], 1)
    d = (te[:, :, None] - ts[:, None, :]).abs().clamp(min=1).double()
    return torch.clamp(torch.floor(torch.log(d) / LOG_BASE), max=num_buckets).long()


def attention(act, pos_w, ts_w, seq, bkt, H, dq, dv, N):
    """``AV [B, T, H dv]`` from ``act [B, T, 2 H dv + 2 H dq]`` = u | v | q | k (``ts_w`` / ``bkt`` None: no time term)."""
    B, T, _ = act.shape
    _, v, q, k = act.split([H * dv, H * dv, H * dq, H * dq], -1)
    S = torch.einsum("bihd,bjhd->bhij", q.reshape(B, T, H, dq), k.reshape(B, T, H, dq))
    t = torch.arange(T)
    S = S + pos_w[N - 1 + t[None, :] - t[:, None]]
    if ts_w is not None:
        S = S + ts_w[bkt][:, None]
    valid = seq != 0
    mask = (t[None, :] <= t[:, None])[None] & valid[:, :, None] & valid[:, None, :]
    A = F.silu(S) / N * mask[:, None].to(S.dtype)
    return torch.einsum("bhij,bjhd->bihd", A, v.reshape(B, T, H, dv)).reshape(B, T, H * dv)


def forward(w, cfg, seq, ts, keep=None, ks=1.0):
    """``f [B, T, D]`` from torch weights ``w`` on ``seq`` / ``ts [B, T = maxlen]``; ``keep``: None or the 1 + blocks masks."""
    D, H, dq, dv, N = cfg["emb_dim"], cfg["num_heads"], cfg["attention_dim"], cfg["linear_dim"], cfg["maxlen"]
    timed = cfg["rel_bias"] == "pos_time"
    drop = lambda v, i: v if keep is None else v * keep[i].to(v.dtype) * ks      # noqa: E731
    valid = (seq != 0).to(w["pos_emb.weight"].dtype)[..., None]
    bkt = buckets(ts, cfg["num_buckets"]) if timed else None
    x = drop(w["item_emb.weight"][seq] * math.sqrt(D) + w["pos_emb.weight"][None, :seq.shape[1]], 0) * valid
    for b in range(cfg["num_blocks"]):
        p = f"blocks.{b}."
        act = F.silu(F.layer_norm(x, (D,), w[p + "norm.weight"], w[p + "norm.bias"], EPS) @ w[p + "uvqk"])
        av = attention(act, w[p + "pos_w"], w[p + "ts_w"] if timed else None, seq, bkt, H, dq, dv, N)
        y = drop(F.layer_norm(av, (H * dv,), None, None, EPS) * act[..., :H * dv], 1 + b)
        x = (x + F.linear(y, w[p + "o.weight"], w[p + "o.bias"])) * valid
    return F.layer_norm(x, (D,), w["last_norm.weight"], w["last_norm.bias"], EPS)


def grads(w_np, cfg, batch, dtype=torch.float64, keep=None, ks=1.0):
    """``(loss, {name: gradient}, f [B, maxlen, D], scores [B, n_items] of the last position)`` as numpy arrays of
    ``dtype``; the batch is left-padded to ``maxlen`` first, as the engine does."""
    w = {n: torch.tensor(v, dtype=dtype, requires_grad=True) for n, v in w_np.items()}
    arrays = [torch.as_tensor(np.asarray(a)) for a in batch[1:]]
    seq, pos, neg = (F.pad(a, (cfg["maxlen"] - a.shape[1], 0)) for a in (arrays[0], arrays[-2], arrays[-1]))
    ts = F.pad(arrays[1], (cfg["maxlen"] - arrays[1].shape[1], 0)) if len(arrays) == 4 else None
    if keep is not None:
        keep = [torch.as_tensor(np.asarray(k)).reshape(seq.shape + (-1,)) for k in keep]
    f = forward(w, cfg, seq, ts, keep, ks)
    E = w["item_emb.weight"]
    lab = pos != 0
    terms = F.softplus(-(f * E[pos]).sum(-1)) + F.softplus((f * E[neg]).sum(-1))
    loss = terms[lab].sum() / max(int(lab.sum()), 1) + cfg.get("l2_emb", 0.0) * E.norm()
    loss.backward()
    g = {n: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for n, v in w.items()}
    return float(loss.detach()), g, f.detach().numpy(), (f[:, -1] @ E[1:].T).detach().numpy()
