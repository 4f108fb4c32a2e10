"""Mamba4Rec (Liu et al., 2024) in plain torch ops with a Python loop over the positions and autograd, in float64 or
float32: the specification csrc/mamba4rec.hip is held to (there is no counterpart in the reference).  No tests here.

``CASES`` are the shapes of tests/test_mamba4rec_gpu.py, each named for the edge it is there for: a lane of the scan holds
``ceil(T / 64)`` positions, a workgroup 16 channels, a staged chunk 16 states, and at most ``PARTS`` workgroups per channel
slab walk the batch for the gradients that are summed over it."""
import numpy as np
import torch
import torch.nn.functional as F

PARTS = 128
EPS = 1e-12

CASES = {
    "t1": dict(T=1, D=16, expand=1, N=1, Kc=2, R="auto", B=2, nb=2),       # one lane, one step, one state; conv sees padding
    "below_conv": dict(T=3, D=16, expand=2, N=5, Kc=4, R="auto", B=3, nb=2),      # window wider than the sequence, odd N
    "lanes_exact": dict(T=64, D=32, expand=2, N=16, Kc=4, R=3, B=3, nb=2),        # k = 1, every lane used, odd dt_rank
    "lanes_plus_one": dict(T=65, D=48, expand=2, N=8, Kc=3, R="auto", B=3, nb=2),     # k = 2, last lane half-filled, Di 96
    "default": dict(T=50, D=64, expand=2, N=32, Kc=4, R="auto", B=5, nb=2),       # the published shape
    "max": dict(T=256, D=128, expand=2, N=64, Kc=4, R="auto", B=2, nb=1),         # k = 4, Di 256, no residual
    # B = 2 PARTS + 3: workgroups 0 .. 2 walk three sequences, the others two; row 1 is all padding and unlabelled
    "batch_seams": dict(T=8, D=16, expand=1, N=4, Kc=2, R="auto", B=2 * PARTS + 3, nb=2),
}
N_ITEMS = 50


def make(case):
    """Seeded fixture of a case: ``(cfg, w, batch)`` with float32 numpy weights in state_dict() order and
    ``batch = (u, seq [B, T], pos [B], neg [B])``.  Row 0 is full, row 1 is the shortest (all padding and unlabelled in
    ``batch_seams``, one item elsewhere), the others have random lengths.  Weights are drawn far larger than the init;
    ``A_log`` and ``dt_proj.bias`` are spread so that ``delta |A|`` runs from about 1e-3 (channel 1) to about 10 (channel 0)."""
    c = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    T, D, B, nb, N, Kc, I = c["T"], c["D"], c["B"], c["nb"], c["N"], c["Kc"], N_ITEMS
    Di, H, R = c["expand"] * D, 4 * D, -(-D // 16) if c["R"] == "auto" else c["R"]
    ln = lambda p: {p + ".weight": rng.uniform(0.5, 1.5, D), p + ".bias": rng.normal(0, 0.3, D)}      # noqa: E731
    w = {"item_emb.weight": rng.normal(0, 0.5, (I + 1, D)), **ln("emb_norm")}
    w["item_emb.weight"][0] = 0
    for b in range(nb):
        p, m = f"layers.{b}.", f"layers.{b}.mamba."
        w[m + "in_proj.weight"] = rng.normal(0, 1 / np.sqrt(D), (2 * Di, D))
        w[m + "conv1d.weight"], w[m + "conv1d.bias"] = rng.normal(0, 0.5, (Di, 1, Kc)), rng.normal(0, 0.1, Di)
        w[m + "x_proj.weight"] = rng.normal(0, 1 / np.sqrt(Di), (R + 2 * N, Di))
        w[m + "dt_proj.weight"] = rng.uniform(-R ** -0.5, R ** -0.5, (Di, R))
        w[m + "dt_proj.bias"], w[m + "A_log"] = rng.uniform(-6, 2, Di), rng.uniform(-1, 2, (Di, N))
        w[m + "dt_proj.bias"][:2], w[m + "A_log"][:2] = (2.0, -6.0), ((1.6,), (-1.0,))
        w[m + "D"] = rng.normal(1, 0.3, Di)
        w[m + "out_proj.weight"] = rng.normal(0, 1 / np.sqrt(Di), (D, Di))
        w.update(ln(p + "norm1"))
        w[p + "fc1.weight"], w[p + "fc1.bias"] = rng.normal(0, 1 / np.sqrt(D), (H, D)), rng.normal(0, 0.1, H)
        w[p + "fc2.weight"], w[p + "fc2.bias"] = rng.normal(0, 1 / np.sqrt(H), (D, H)), rng.normal(0, 0.1, D)
        w.update(ln(p + "norm2"))
    w = {n: v.astype(np.float32) for n, v in w.items()}
    lens = rng.integers(1, T + 1, B)
    lens[0], lens[1] = T, 0 if case == "batch_seams" else 1
    seq = np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(lens):
        seq[b, T - n:] = rng.integers(1, I + 1, n)
    pos, neg = rng.integers(1, I + 1, B), rng.integers(1, I + 1, B)
    pos[lens == 0] = 0
    cfg = {"n_users": B, "n_items": I, "emb_dim": D, "maxlen": T, "num_blocks": nb, "dropout_rate": 0.0, "batch_size": B,
           "d_state": N, "d_conv": Kc, "expand": c["expand"], "dt_rank": c["R"]}
    return cfg, w, (np.arange(B), seq, pos, neg)


def selective_scan(u, dt_pre, z, A, Bm, Cm, Dp, m):
    """u, dt_pre, z [B, T, Di], A [Di, N], Bm, Cm [B, T, N], Dp [Di], m [B, T] 0/1: state and output are 0 where m is."""
    delta, h, ys = F.softplus(dt_pre), u.new_zeros(u.shape[0], u.shape[2], A.shape[1]), []
    for t in range(u.shape[1]):
        h = (torch.exp(delta[:, t, :, None] * A) * h + (delta[:, t] * u[:, t])[..., None] * Bm[:, t, None]) * m[:, t, None, None]
        ys.append(((h * Cm[:, t, None]).sum(-1) + Dp * u[:, t]) * m[:, t, None])
    return torch.stack(ys, 1) * F.silu(z)


def mamba(x, w, p, m):
    """The Mamba block on x [B, T, D] (already zero at padding) with the parameters ``w[p + ...]``."""
    Di, Kc = w[p + "conv1d.weight"].shape[0], w[p + "conv1d.weight"].shape[2]
    R, N, T = w[p + "dt_proj.weight"].shape[1], w[p + "A_log"].shape[1], x.shape[1]
    xi, z = (x @ w[p + "in_proj.weight"].T).split(Di, -1)
    u = F.silu(F.conv1d(xi.transpose(1, 2), w[p + "conv1d.weight"], w[p + "conv1d.bias"], padding=Kc - 1, groups=Di)[..., :T])
    u = u.transpose(1, 2)
    dt, Bm, Cm = (u @ w[p + "x_proj.weight"].T).split([R, N, N], -1)
    dt_pre = dt @ w[p + "dt_proj.weight"].T + w[p + "dt_proj.bias"]
    y = selective_scan(u, dt_pre, z, -torch.exp(w[p + "A_log"]), Bm, Cm, w[p + "D"], m)
    return y @ w[p + "out_proj.weight"].T


def forward(w, cfg, seq, keep=None, ks=1.0):
    """``x`` [B, T, D] of the last layer from torch weights ``w``; ``keep``: None or the 1 + 3 layers masks."""
    D, nb = cfg["emb_dim"], cfg["num_blocks"]
    drop = lambda v, i: v if keep is None else v * keep[i].to(v.dtype) * ks      # noqa: E731
    ln = lambda v, p: F.layer_norm(v, (D,), w[p + ".weight"], w[p + ".bias"], EPS)      # noqa: E731
    m = (seq != 0).to(w["item_emb.weight"].dtype)
    x = ln(drop(F.embedding(seq, w["item_emb.weight"], padding_idx=0), 0), "emb_norm")
    for b in range(nb):
        p = f"layers.{b}."
        h = drop(mamba(x * m[..., None], w, p + "mamba.", m), 1 + 3 * b)
        h = ln(h + x if nb > 1 else h, p + "norm1")
        z = drop(F.gelu(F.linear(h, w[p + "fc1.weight"], w[p + "fc1.bias"])), 2 + 3 * b)
        x = ln(h + drop(F.linear(z, w[p + "fc2.weight"], w[p + "fc2.bias"]), 3 + 3 * b), p + "norm2")
    return x


def grads(w_np, cfg, batch, dtype=torch.float64, keep=None, ks=1.0):
    """``(loss, {name: gradient}, f [B, D], scores [B, n_items])`` as numpy arrays of ``dtype``."""
    w = {n: torch.tensor(v, dtype=dtype, requires_grad=True) for n, v in w_np.items()}
    seq, pos, neg = (torch.as_tensor(np.asarray(a)) for a in batch[1:])
    if keep is not None:
        keep = [torch.as_tensor(np.asarray(k)).reshape(seq.shape + (-1,)) for k in keep]
    f = forward(w, cfg, seq, keep, ks)[:, -1]
    E = w["item_emb.weight"]
    lab = pos != 0
    terms = F.softplus(-(f * E[pos]).sum(-1)) + F.softplus((f * E[neg]).sum(-1))
    loss = terms[lab].sum() / max(int(lab.sum()), 1)
    loss.backward()
    g = {n: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for n, v in w.items()}
    return float(loss.detach()), g, f.detach().numpy(), (f @ E[1:].T).detach().numpy()
