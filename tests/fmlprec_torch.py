"""FMLP-Rec (Zhou et al., WWW 2022) in plain torch ops with ``torch.fft`` and autograd, in float64 or float32: the
specification csrc/fmlprec.hip is held to (there is no counterpart in the reference).  No tests here.

``CASES`` are the shapes of tests/test_fmlprec_gpu.py, each named for the edge it is there for: the filter kernels work in
tiles of 16 frequencies / 16 positions / 16 channels, and at most ``PARTS`` workgroups per channel slab walk the batch for
the filter's weight gradient."""
import numpy as np
import torch
import torch.nn.functional as F

PARTS = 64
EPS = 1e-12

# T, D, B, blocks
CASES = {
    "t1": dict(T=1, D=16, B=2, nb=2),                    # F = 1, DC only
    "t2": dict(T=2, D=16, B=3, nb=2),                    # DC + Nyquist only: every imaginary weight is inert
    "odd_below_tile": dict(T=15, D=16, B=3, nb=2),       # no Nyquist bin, one partial tile
    "tile_exact": dict(T=16, D=32, B=4, nb=2),           # F = 9
    "tile_plus_one": dict(T=17, D=48, B=3, nb=2),        # odd, F = 9, three channel slabs
    "default_len": dict(T=50, D=64, B=5, nb=2),          # F = 26, not a multiple of 4
    "max_len_d128": dict(T=256, D=128, B=2, nb=1),       # F = 129, one past a tile, every slab
    # B = 2 PARTS + 3: workgroups 0 .. 2 walk three sequences, the others two; row 1 is all padding and unlabelled
    "dw_seams": dict(T=8, D=16, B=2 * PARTS + 3, nb=2),
}
N_ITEMS = 50


def make(case):
    """Seeded fixture of a case: ``(cfg, w, batch)`` with float32 numpy weights in state_dict() order and
    ``batch = (u, seq [B, T], pos [B], neg [B])``.  Row 0 is full, row 1 is the shortest (all padding and unlabelled in
    ``dw_seams``, one item elsewhere), the others have random lengths.  Weights are drawn far larger than the init."""
    c = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    T, D, B, nb, H, I = c["T"], c["D"], c["B"], c["nb"], 4 * c["D"], N_ITEMS
    ln = lambda p: {p + ".weight": rng.uniform(0.5, 1.5, D), p + ".bias": rng.normal(0, 0.3, D)}      # noqa: E731
    w = {"item_emb.weight": rng.normal(0, 0.5, (I + 1, D)), "pos_emb.weight": rng.normal(0, 0.5, (T, D)), **ln("emb_norm")}
    w["item_emb.weight"][0] = 0
    for b in range(nb):
        p = f"blocks.{b}."
        w[p + "filter.complex_weight"] = rng.normal(0, 0.3, (T // 2 + 1, D, 2))
        w.update(ln(p + "norm1"))
        w[p + "fc1.weight"], w[p + "fc1.bias"] = rng.normal(0, 1 / np.sqrt(D), (H, D)), rng.normal(0, 0.1, H)
        w[p + "fc2.weight"], w[p + "fc2.bias"] = rng.normal(0, 1 / np.sqrt(H), (D, H)), rng.normal(0, 0.1, D)
        w.update(ln(p + "norm2"))
    w = {n: v.astype(np.float32) for n, v in w.items()}
    lens = rng.integers(1, T + 1, B)
    lens[0], lens[1] = T, 0 if case == "dw_seams" else 1
    seq = np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(lens):
        seq[b, T - n:] = rng.integers(1, I + 1, n)
    pos, neg = rng.integers(1, I + 1, B), rng.integers(1, I + 1, B)
    pos[lens == 0] = 0
    cfg = {"n_users": B, "n_items": I, "emb_dim": D, "maxlen": T, "num_blocks": nb, "dropout_rate": 0.0, "batch_size": B}
    return cfg, w, (np.arange(B), seq, pos, neg)


def filter_layer(x, weight):
    """x [B, T, D], weight [T // 2 + 1, D, 2]: the learnable filter along the positions."""
    spectrum = torch.fft.rfft(x, dim=1, norm="ortho") * torch.view_as_complex(weight)[None]
    return torch.fft.irfft(spectrum, n=x.shape[1], dim=1, norm="ortho")


def forward(w, cfg, seq, keep=None, ks=1.0):
    """``x`` [B, T, D] of the last block from torch weights ``w``; ``keep``: None or the 1 + 2 blocks masks [B, T, D]."""
    D = cfg["emb_dim"]
    drop = lambda v, i: v if keep is None else v * keep[i].to(v.dtype) * ks      # noqa: E731
    ln = lambda v, p: F.layer_norm(v, (D,), w[p + ".weight"], w[p + ".bias"], EPS)      # noqa: E731
    x = F.embedding(seq, w["item_emb.weight"], padding_idx=0) + w["pos_emb.weight"][None]
    x = drop(ln(x, "emb_norm"), 0)
    for b in range(cfg["num_blocks"]):
        p = f"blocks.{b}."
        h = ln(x + drop(filter_layer(x, w[p + "filter.complex_weight"]), 1 + 2 * b), p + "norm1")
        z = F.linear(F.gelu(F.linear(h, w[p + "fc1.weight"], w[p + "fc1.bias"])), w[p + "fc2.weight"], w[p + "fc2.bias"])
        x = ln(h + drop(z, 2 + 2 * b), p + "norm2")
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
