"""ETA (Chen et al., 2021) in plain torch ops with autograd, in float64 or float32: the specification csrc/eta.hip is held to
(there is no counterpart in the reference).  No tests here.

``CASES`` are the whole-step shapes of tests/test_eta_gpu.py, ``RETRIEVE_CASES`` / ``ATTENTION_CASES`` those of the two stage
entries, each named for the kernel edge it is there for: chunks of 64 positions, 32 hash bits a word, four candidates scanned
at a time, a sequence's codes in LDS unless they do not fit (``D`` 128 with 128 bits at ``T`` 4096), two slots a lane at ``k``
128, a second K-slice of the weight-gradient GEMMs from 512 compact rows on.  Every whole-step fixture has a full row (0), a
row of one item (1), an all-padding row (the last), a dead candidate, a repeated item and a candidate from its own history."""
import numpy as np
import torch
import torch.nn.functional as F

N_ITEMS = 60

CASES = {
    "chunk_plus_one": dict(T=65, C=5, D=16, B=4, m=32, k=5, H=1, dnn=[8], dnn_act="prelu"),   # 64 + 1, a fifth candidate
    "k_above_live": dict(T=20, C=2, D=32, B=4, m=96, k=24, H=8, dnn=[12, 8]),                 # every live position is taken
    "slices": dict(T=8, C=8, D=16, B=65, m=64, k=8, H=2, dnn=[8]),                # 520 compact rows and pairs: two K-slices each
    "published": dict(T=1024, C=4, D=64, B=3, m=64, k=48, H=4, dnn=[200, 80]),                # the published sizes
}
RETRIEVE_CASES = {
    "t1": dict(T=1, C=1, D=16, B=3, m=32, k=1),
    "chunk_plus_one": dict(T=65, C=5, D=16, B=3, m=32, k=7),
    "k_at_live": dict(T=40, C=3, D=32, B=4, m=96, k=16),                  # row 0 has 16 live positions, row 1 five
    "long_in_lds": dict(T=4096, C=2, D=16, B=2, m=64, k=128),
    "long_in_workspace": dict(T=4096, C=2, D=128, B=2, m=128, k=48),      # four words, the widest rows
}
ATTENTION_CASES = {
    "h1_k1": dict(T=9, C=2, D=16, B=3, H=1, k=1),
    "heads_max_k17": dict(T=40, C=3, D=16, B=3, H=4, k=17),
    "d128_k128": dict(T=200, C=2, D=128, B=2, H=32, k=128),
    "slices": dict(T=16, C=2, D=16, B=33, H=2, k=8),                      # 528 compact rows: two K-slices
}


def pack(bits):
    """``[..., m]`` bool -> ``[..., m / 32]`` int32: bit ``j`` in word ``j / 32`` at position ``j % 32``."""
    b = bits.reshape(*bits.shape[:-1], -1, 32).to(torch.int64)
    words = (b << torch.arange(32)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def select(bits_e, bits_q, live, k):
    """``sel [B, C, k]`` int32: the ``k`` live positions with the smallest (Hamming distance, -t), ascending, -1 behind."""
    B, T, _ = bits_e.shape
    ham = (bits_q[:, :, None, :] != bits_e[:, None, :, :]).sum(-1)
    key = ham * T + (T - 1 - torch.arange(T))
    key = torch.where(live[:, None, :], key, torch.full_like(key, 1 << 40))
    val, at = key.sort(-1)
    at = torch.where(val < (1 << 40), at, torch.full_like(at, T))[..., :k].sort(-1)[0]
    at = F.pad(at, (0, k - at.shape[-1]), value=T)
    return torch.where(at < T, at, torch.full_like(at, -1)).to(torch.int32)


def retrieve(e, q, live, hash_w, k):
    """``(codes_e, codes_q, sel)`` of explicit rows, in the dtype of ``e``."""
    be, bq = e @ hash_w.T >= 0, q @ hash_w.T >= 0
    return pack(be), pack(bq), select(be, bq, live, k)


def attention(e, q, sel, w, H):
    """``e [B, T, D]``, ``q [B, C, D]``, ``sel [B, C, k]``: ``v [B, C, D]``."""
    B, C, k = sel.shape
    D = e.shape[-1]
    Qp, Kp, Vp = (x @ w[f"att.{p}.weight"].T + w[f"att.{p}.bias"] for p, x in (("q", q), ("k", e), ("v", e)))
    on = sel >= 0
    at = (torch.arange(B)[:, None, None], sel.clamp(min=0).long())
    Kg, Vg = Kp[at].view(B, C, k, H, D // H), Vp[at].view(B, C, k, H, D // H)
    s = (Qp.view(B, C, 1, H, D // H) * Kg).sum(-1) / (D // H) ** 0.5
    p = torch.softmax(s.masked_fill(~on[..., None], -1e30), 2) * on[..., None].to(e.dtype)
    return (p[..., None] * Vg).sum(2).reshape(B, C, D) @ w["att.o.weight"].T + w["att.o.bias"]


def logits(w, cfg, seq, cand, running=None, train=True):
    """``(logits [B, C] (0 in dead slots), live, sel, bits of the distinct items)``."""
    E = w["item_emb.weight"]
    q, e = E[cand], E[seq]
    with torch.no_grad():
        be, bq = e @ w["hash.weight"].T >= 0, q @ w["hash.weight"].T >= 0
        sel = select(be, bq, seq != 0, cfg["top_k"])
        sel[cand == 0] = -1
    v = attention(e, q, sel, w, cfg["num_heads"])
    live = (cand != 0).reshape(-1)
    y = torch.cat([v, q, v * q], -1).reshape(live.numel(), -1)[live]
    for l in range(len(cfg["dnn_hidden"])):
        y = y @ w[f"dnn.{l}.weight"].T + w[f"dnn.{l}.bias"]
        alpha = w[f"dnn.{l}.alpha"]
        if cfg["dnn_activation"] == "prelu":
            y = torch.where(y > 0, y, alpha * y)
        elif y.shape[0]:
            rm, rv = (running[f"dnn.{l}.{n}"] for n in ("running_mean", "running_var")) if running else (None, None)
            p = torch.sigmoid(F.batch_norm(y, rm, rv, None, None, train, 0.1, 1e-8))      # BatchNorm1d(affine=False)
            y = p * y + (1 - p) * alpha * y
    out = torch.zeros(live.numel(), dtype=y.dtype)
    out[live] = (y @ w["out.weight"].T + w["out.bias"])[:, 0]
    return out.view(cand.shape), live, sel


def grads(w_np, cfg, batch, dtype=torch.float64, running=None):
    """``(loss, {name: gradient}, logits [B, C], sel)`` as numpy; ``running`` moves in place; ``hash.weight`` is left out."""
    w = {n: torch.tensor(v, dtype=dtype, requires_grad=n != "hash.weight") for n, v in w_np.items()}
    seq, cand, label = (torch.as_tensor(np.asarray(a)) for a in batch)
    run = {n: torch.tensor(v, dtype=dtype) for n, v in running.items()} if running else None
    z, live, sel = logits(w, cfg, seq, cand, run, True)
    terms = F.binary_cross_entropy_with_logits(z, label.to(dtype), reduction="none").reshape(-1)
    loss = terms[live].sum() / max(int(live.sum()), 1)
    loss.backward()
    if running:
        for n in running:
            running[n][...] = run[n].numpy()
    g = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).numpy() for n, p in w.items() if n != "hash.weight"}
    return float(loss.detach()), g, z.detach().numpy(), sel.numpy()


def predict(w_np, cfg, seq, cand, running, dtype=torch.float64):
    """Eval-mode logits: Dice reads the running buffers."""
    w = {n: torch.tensor(v, dtype=dtype) for n, v in w_np.items()}
    run = {n: torch.tensor(v, dtype=dtype) for n, v in running.items()} if running else None
    return logits(w, cfg, torch.as_tensor(seq), torch.as_tensor(cand), run, False)[0].numpy()


def config(c):
    return {"n_items": N_ITEMS, "emb_dim": c["D"], "maxlen": c["T"], "hash_bits": c.get("m", 32), "top_k": c["k"],
            "num_heads": c.get("H", 1), "dnn_hidden": list(c.get("dnn", [8])), "batch_size": c["B"],
            "dnn_activation": c.get("dnn_act", "dice")}


def weights(cfg, rng):
    """Seeded float32 weights in state_dict() order, ``hash.weight`` last."""
    D, dnn = cfg["emb_dim"], cfg["dnn_hidden"]
    shapes = [(f"att.{p}", D, D) for p in "qkvo"]
    shapes += [(f"dnn.{l}", n, ([3 * D] + dnn)[l]) for l, n in enumerate(dnn)] + [("out", 1, dnn[-1])]
    w = {"item_emb.weight": rng.normal(0, 0.5, (cfg["n_items"] + 1, D))}
    w["item_emb.weight"][0] = 0
    for name, n_out, n_in in shapes:
        w[name + ".weight"] = rng.uniform(-1, 1, (n_out, n_in)) * (3.0 / n_in) ** 0.5
        w[name + ".bias"] = rng.normal(0, 0.1, n_out)
        if name.startswith("dnn"):
            w[name + ".alpha"] = rng.uniform(0.1, 0.4, n_out)
    w["hash.weight"] = rng.normal(0, 1, (cfg["hash_bits"], D))
    return {n: v.astype(np.float32) for n, v in w.items()}


def make(case, n_cand=None):
    """Seeded fixture of a whole-step case: ``(cfg, w, batch, running)``.  Asserts that no projection of an item onto a hash
    vector lies within 1e-5 of zero and that float32 and float64 give the same code bits: a condition on the inputs."""
    c = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)) + c.get("seed", 0))
    T, B, I = c["T"], c["B"], N_ITEMS
    C = n_cand or c["C"]
    cfg = config(c)
    w = weights(cfg, rng)
    proj = [torch.tensor(w["item_emb.weight"][1:], dtype=t) @ torch.tensor(w["hash.weight"], dtype=t).T
            for t in (torch.float32, torch.float64)]
    assert float(proj[1].abs().min()) > 1e-5 and torch.equal(proj[0] >= 0, proj[1] >= 0), f"{case}: draw another seed"
    lens = rng.integers(1, T + 1, B)
    lens[0], lens[1], lens[-1] = T, 1, 0
    seq = np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(lens):
        seq[b, T - n:] = rng.integers(1, I + 1, n)
    seq[0, -2] = seq[0, -1]
    cand = rng.integers(1, I + 1, (B, C))
    cand[0, 0] = seq[0, -1]
    cand[2, -1] = 0
    label = (rng.random((B, C)) < 0.5).astype(np.float32)
    running = {}
    if cfg["dnn_activation"] == "dice":
        for l, n in enumerate(cfg["dnn_hidden"]):
            running[f"dnn.{l}.running_mean"] = rng.normal(0, 0.1, n).astype(np.float32)
            running[f"dnn.{l}.running_var"] = rng.uniform(0.5, 1.5, n).astype(np.float32)
    return cfg, w, (seq, cand, label), running


def make_retrieve(case):
    """Dyadic fixture ``(cfg, hash_w, e, q, mask)``: ``e``, ``q`` multiples of 2^-6 in [-2, 2], ``hash_w`` of 2^-4 in (-4, 4),
    so every projection is exact in float32, zeros included.  History rows come from a pool of 12 (ties at every threshold),
    half of the candidates too (distance 0); the mask has holes, row 0 is all live, the last row all dead."""
    c = RETRIEVE_CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    T, C, D, B = c["T"], c["C"], c["D"], c["B"]
    pool = rng.integers(-128, 129, (12, D)) / 64.0
    pool[0] = 0      # projections of exactly zero
    e = pool[rng.integers(0, 12, (B, T))]
    q = np.where(rng.random((B, C, 1)) < 0.5, pool[rng.integers(0, 12, (B, C))], rng.integers(-128, 129, (B, C, D)) / 64.0)
    hash_w = rng.integers(-63, 64, (c["m"], D)) / 16.0
    mask = rng.random((B, T)) < 0.7
    mask[0], mask[-1] = True, False
    if case == "k_at_live":
        mask[0, 16:], mask[1], mask[1, ::8] = False, False, True
    f = lambda a: torch.tensor(a, dtype=torch.float32)      # noqa: E731
    return config(c), f(hash_w), f(e), f(q), torch.tensor(mask)


def make_attention(case):
    """``(cfg, w, e, q, sel, dv)`` with an explicit valid ``sel`` that is not the retrieval's: pair (0, 0) is full, (0, 1)
    shares its positions, (1, 0) has none, the others hold a random number of random positions."""
    c = ATTENTION_CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    T, C, D, B, k = c["T"], c["C"], c["D"], c["B"], c["k"]
    cfg = config(c)
    w = weights(cfg, rng)
    sel = np.full((B, C, k), -1, dtype=np.int32)
    for b in range(B):
        for j in range(C):
            n = min(k, T) if (b, j) == (0, 0) else 0 if (b, j) == (1, 0) else int(rng.integers(0, min(k, T) + 1))
            sel[b, j, :n] = np.sort(rng.choice(T, n, replace=False))
    if case == "slices":      # two disjoint full rows a sequence: 512 live compact rows, past the first K-slice of 264
        sel[2:, 0], sel[2:, 1] = np.arange(0, T, 2), np.arange(1, T, 2)
    sel[0, 1] = sel[0, 0]
    sel[0, 1, max(1, k // 2):] = -1
    e, q, dv = (torch.tensor(rng.normal(0, 0.5, s)) for s in ((B, T, D), (B, C, D), (B, C, D)))
    return cfg, w, e, q, torch.tensor(sel), dv
