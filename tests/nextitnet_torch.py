"""NextItNet (Yuan et al., WSDM 2019) in plain torch ops with autograd, in float64 or float32: the specification
csrc/nextitnet.hip is held to (there is no counterpart in the reference).  No tests here.

``CASES`` are the shapes of tests/test_nextitnet_gpu.py, each named for the edge it is there for; the tile sizes are
csrc/nextitnet.hpp's (time tile 32, weight-gradient row tile 32 in at most 32 slabs, cross-entropy tile 32 x 64 in at most
16 catalogue splits)."""
import numpy as np
import torch
import torch.nn.functional as F

TIME_TILE, WGRAD_ROWS, MAX_SLABS = 32, 32, 32

# D, k, T, dilations, block_num, B, n_items, loss_positions
CASES = {
    "t1_k1_b1": dict(D=16, k=1, T=1, dilations=[1], block_num=1, B=1, n_items=63, loss="all"),
    "tile_minus_one_k2": dict(D=48, k=2, T=TIME_TILE - 1, dilations=[1, 4], block_num=1, B=3, n_items=64, loss="all"),
    "tile_exact_k4_last": dict(D=16, k=4, T=TIME_TILE, dilations=[1], block_num=2, B=4, n_items=65, loss="last"),
    "tile_plus_one_d128": dict(D=128, k=3, T=TIME_TILE + 1, dilations=[1, 4], block_num=1, B=2, n_items=65, loss="all"),
    # T = 40, k = 3, d = 9: conv2 reaches (k-1) 2d = 36 rows back, from the second time tile across the seam into the first
    "reach_across_seam": dict(D=16, k=3, T=40, dilations=[9], block_num=1, B=3, n_items=63, loss="all"),
    # 2d = 16 >= T = 12: only the current tap of conv2 (and of conv1's far taps at d = 8) contributes
    "reach_beyond_t": dict(D=16, k=3, T=12, dilations=[8], block_num=1, B=3, n_items=64, loss="last"),
    # B T = 33 * 33 = 1089 rows = 35 row tiles: more than 32 slabs (slabs 0 .. 2 walk two tiles) and a last tile of 1 row;
    # 1100 items are 18 item tiles, which the row-side kernels cut into 9 splits of 2
    "slab_seam_and_splits": dict(D=16, k=2, T=33, dilations=[1], block_num=1, B=33, n_items=1100, loss="all"),
}


def make(case):
    """Seeded fixture of a case: ``(cfg, w, batch)`` with float32 numpy weights in state_dict() order and
    ``batch = (u, seq, pos, neg)``.  Sequences have mixed real lengths: row 0 is full and, from B = 3 on, row 1 is all
    padding.  The conv biases are drawn well away from 0 so that LayerNorm (eps 1e-8) never sees a near-constant row."""
    c = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    D, k, T, B, I = c["D"], c["k"], c["T"], c["B"], c["n_items"]
    R = len(c["dilations"]) * c["block_num"]
    w = {"item_emb.weight": rng.normal(0, 0.5, (I + 1, D))}
    w["item_emb.weight"][0] = 0
    for r in range(R):
        for n in ("1", "2"):
            w[f"blocks.{r}.conv{n}.weight"] = rng.normal(0, 1.0 / np.sqrt(D * k), (D, D, 1, k))
            w[f"blocks.{r}.conv{n}.bias"] = rng.normal(0, 0.5, D)
            w[f"blocks.{r}.ln{n}.weight"] = rng.uniform(0.5, 1.5, D)
            w[f"blocks.{r}.ln{n}.bias"] = rng.normal(0, 0.3, D)
    w["final_layer.weight"] = rng.normal(0, 1.0 / np.sqrt(D), (D, D))
    w["final_layer.bias"] = rng.normal(0, 0.1, D)
    w = {n: v.astype(np.float32) for n, v in w.items()}
    lens = rng.integers(1, T + 1, B)
    lens[0] = T
    if B >= 3:
        lens[1] = 0
    seq, pos = np.zeros((B, T), dtype=np.int64), np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(lens):
        walk = rng.integers(1, I + 1, n + 1)
        seq[b, T - n:], pos[b, T - n:] = walk[:-1], walk[1:]
    cfg = {"n_items": I, "emb_dim": D, "kernel_size": k, "dilations": c["dilations"], "block_num": c["block_num"],
           "maxlen": T, "loss_positions": c["loss"]}
    return cfg, w, (np.arange(B), seq, pos, np.zeros((B, T), dtype=np.int64))


def _conv(x, weight, bias, dil):
    """x [B, T, D] -> the causal convolution at dilation ``dil``: left zero padding of (k - 1) dil rows."""
    k = weight.shape[-1]
    xp = F.pad(x.transpose(1, 2).unsqueeze(2), ((k - 1) * dil, 0))      # [B, D, 1, T + (k - 1) dil]
    return F.conv2d(xp, weight, bias, dilation=(1, dil)).squeeze(2).transpose(1, 2)


def forward(w, cfg, seq):
    """``f`` [B, T, D] from torch weights ``w`` (a dict by state_dict() name)."""
    D = cfg["emb_dim"]
    x = F.embedding(seq, w["item_emb.weight"], padding_idx=0)      # row 0 receives no gradient
    for r, d in enumerate(list(cfg["dilations"]) * cfg["block_num"]):
        p = f"blocks.{r}."
        h = F.relu(F.layer_norm(_conv(x, w[p + "conv1.weight"], w[p + "conv1.bias"], d), (D,), w[p + "ln1.weight"],
                                w[p + "ln1.bias"], 1e-8))
        x = F.relu(F.layer_norm(_conv(h, w[p + "conv2.weight"], w[p + "conv2.bias"], 2 * d), (D,), w[p + "ln2.weight"],
                                w[p + "ln2.bias"], 1e-8)) + x
    return F.linear(x, w["final_layer.weight"], w["final_layer.bias"])


def grads(w_np, cfg, batch, dtype=torch.float64):
    """``(loss, {name: gradient}, f_last [B, D], scores_last [B, n_items])`` as numpy arrays of ``dtype``."""
    w = {n: torch.tensor(v, dtype=dtype, requires_grad=True) for n, v in w_np.items()}
    seq, pos = torch.as_tensor(batch[1]), torch.as_tensor(batch[2])
    f = forward(w, cfg, seq)
    scores = f @ w["item_emb.weight"][1:].T
    if cfg["loss_positions"] == "last":
        lab = torch.zeros_like(pos, dtype=torch.bool)
        lab[:, -1] = pos[:, -1] != 0
    else:
        lab = pos != 0
    n_lab = int(lab.sum())
    loss = -(F.log_softmax(scores[lab], dim=-1).gather(1, pos[lab][:, None] - 1)).sum() / max(n_lab, 1)
    loss.backward()
    g = {n: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for n, v in w.items()}
    return float(loss.detach()), g, f[:, -1].detach().numpy(), scores[:, -1].detach().numpy()
