"""Fixtures of the Caser tests, shared by tests/test_caser_host.py (which shows on the CPU that they see every defect of
``caser_torch.DEFECTS`` and cover what this table claims) and the GPU tests (which run csrc/caser.hip on those very
inputs).  No tests here.

| name          | what it is there for                                                                               |
|---------------|----------------------------------------------------------------------------------------------------|
| l1            | L 1, T 1, N 1, d 1, n_v 1, n_h 1, B 3: one window, nothing to choose                               |
| defaults      | L 5, T 3, N 3, d 50, n_v 4, n_h 16, B 7: d and the 280-wide fc1 input are ragged against every tile |
| limits        | L 10, T 16, N 64, d 128, n_v 16, n_h 64, B 2: every limit at once, heights processed in turn       |
| padding       | leading padding of every length 0 .. L (the last is all padding: out_h = ac_conv(bias)); pos and   |
|               | neg rows with some 0; one row with no real target                                                  |
| one_row       | B 1                                                                                                |
| tile_edges_B  | B one under, at and one over the batch tile of each kernel (``TILE_BATCHES``): the 8 sequences of  |
|               | a convolution workgroup, the 4 waves of a loss block, the 64 rows below which the folds have one   |
|               | slab, and slabs of 255 / 256 / 257 rows around the 256-row LDS chunk of the d conv_h kernel        |
| repeats       | one item as input, positive and negative of many rows, one user in several rows: every row-atomic  |
|               | path must sum                                                                                      |
| acts_ts       | ac_conv tanh, ac_fc sigm                                                                           |
| acts_iden     | iden / iden                                                                                        |
| dropout       | p = 0.5 with an explicit keep mask (``f["keep"]``)                                                 |
| slabs         | B 140: three slabs of 47, 47, 46 rows in the convolution folds, 128 + 12 rows in fc1's bias sum    |

Weights are at unit scale (every pre-activation is O(1), so no term vanishes) and ``l2`` is 0.01 everywhere.  The large
batches draw their sequences from six items and L = 2, so that they hold few DISTINCT sequences.

Every fixture meets ``margins_ok`` in float64: for every (row, height, filter) the best and the second-best window
differ by more than ``MARGIN`` = 1e-3 of the largest |pre| of the fixture (exact ties between all-padding windows are
exempt: the gradient is the same either way), and with relu every pooled pre and every fc1 pre-activation is further than
that from 0 -- otherwise fp32 and fp64 may legitimately take different branches.  ``fixture`` re-seeds the horizontal
filters and fc1 units that miss it until it holds; the bound is never loosened."""
import functools

import numpy as np
import torch

import caser_torch as ct

MARGIN = 1e-3
L2 = 0.01
# csrc/caser.hpp (kCaserSeqTile, kCaserSlabRows, kCaserMaxSlabs, kCaserChunk) and csrc/common.hpp (kWavesPerBlock)
SEQ_TILE, SLAB_ROWS, MAX_SLABS, CHUNK, LOSS_WAVES = 8, 64, 16, 256, 4
LIMITS = {"d": 128, "L": 10, "n_v": 16, "n_h": 64, "T": 16, "N": 64}      # kCaserMax*
TILE_BATCHES = tuple(sorted({t + o for t in (LOSS_WAVES, SEQ_TILE, SLAB_ROWS) for o in (-1, 0, 1)} |
                            {MAX_SLABS * (CHUNK - 1), MAX_SLABS * CHUNK, MAX_SLABS * CHUNK + 1}))
SMALL = dict(L=2, T=1, N=1, d=3, n_v=1, n_h=2, U=5, I=6)

# name -> dims; B, U, I and the rest
SPECS = {
    "l1": dict(L=1, T=1, N=1, d=1, n_v=1, n_h=1, B=3, U=4, I=5),
    "defaults": dict(L=5, T=3, N=3, d=50, n_v=4, n_h=16, B=7, U=9, I=40),
    "limits": dict(L=10, T=16, N=64, d=128, n_v=16, n_h=64, B=2, U=3, I=200),
    "padding": dict(L=4, T=2, N=3, d=6, n_v=2, n_h=3, B=6, U=7, I=12),
    "one_row": dict(L=3, T=2, N=2, d=5, n_v=2, n_h=3, B=1, U=2, I=9),
    "repeats": dict(L=3, T=2, N=3, d=7, n_v=2, n_h=4, B=12, U=5, I=8),
    "acts_ts": dict(L=4, T=2, N=2, d=9, n_v=3, n_h=5, B=5, U=6, I=15, ac_conv="tanh", ac_fc="sigm"),
    "acts_iden": dict(L=4, T=2, N=2, d=9, n_v=3, n_h=5, B=5, U=6, I=15, ac_conv="iden", ac_fc="iden"),
    "dropout": dict(L=5, T=3, N=3, d=20, n_v=3, n_h=6, B=9, U=9, I=30, p=0.5),
    "slabs": dict(L=2, T=2, N=2, d=5, n_v=2, n_h=3, B=140, U=11, I=6),
}
SPECS.update({f"tile_edges_{B}": dict(SMALL, B=B) for B in TILE_BATCHES})
NAMES = tuple(SPECS)
# the fixtures the defect scan runs on (float64 on the CPU: the large ones add nothing there)
SCAN = ("l1", "defaults", "padding", "one_row", "repeats", "acts_ts", "acts_iden", "dropout")


def slabs_of(B):
    """(number of slabs, rows per slab) of the fixed-order folds, as csrc/caser.hip cuts a batch."""
    n = min(MAX_SLABS, -(-B // SLAB_ROWS))
    return n, -(-B // n)


def _weights(rng, s):
    d, L, n_v, n_h = s["d"], s["L"], s["n_v"], s["n_h"]
    w = {}
    for k, shape in ct.shapes(s["U"], s["I"], d, L, n_v, n_h).items():
        if k.endswith("bias") or k == "b2.weight":
            scale = 0.5
        elif k == "conv_v.weight":
            scale = 1.0 / np.sqrt(L)
        elif k.startswith("conv_h"):
            scale = 1.0 / np.sqrt(shape[2] * d)
        elif k == "fc1.weight":
            scale = 1.0 / np.sqrt(shape[1])
        elif k == "W2.weight":
            scale = 1.0 / np.sqrt(2 * d)
        else:
            scale = 1.0
        w[k] = (rng.standard_normal(shape) * scale).astype(np.float32)
    w["item_embeddings.weight"][0] = 0.0
    return w


def _build(name, seed):
    s = dict(SPECS[name])
    s.setdefault("ac_conv", "relu")
    s.setdefault("ac_fc", "relu")
    s.setdefault("p", 0.0)
    rng = np.random.default_rng(seed)
    B, L, T, N, U, I = (s[k] for k in ("B", "L", "T", "N", "U", "I"))
    f = dict(s, name=name, l2=L2, w=_weights(rng, s), keep=None)
    f["users"] = rng.integers(0, U - 1, B)            # the last user is in no batch: an untouched table row
    # L DISTINCT items per row: two equal items make two equal windows, a tie that no draw of the filters resolves
    f["seq"] = np.argsort(rng.random((B, I)), axis=1)[:, :L] + 1
    f["pos"] = rng.integers(1, I + 1, (B, T))
    f["neg"] = rng.integers(1, I + 1, (B, N))
    if name == "padding":
        for b in range(L + 1):
            f["seq"][b, :b] = 0                       # b leading pads; row L is all padding
        f["pos"][1, 0] = f["pos"][2, 1] = 0
        f["neg"][0, 1] = f["neg"][3, 0] = f["neg"][3, 2] = 0
        f["pos"][L + 1] = 0                           # the last row has no real target at all
        f["neg"][L + 1] = 0
    if name == "repeats":
        for b in range(B):                            # item 3 as input, positive and negative of many rows
            row, col = f["seq"][b], 1 - b % 2
            row[row == 3] = row[col]                  # keeps the row's items distinct
            row[col] = 3
        f["pos"][::2, 0] = 3
        f["pos"][1::2, 1] = 3
        f["neg"][::3, 0] = 3
        f["neg"][1::3, 2] = 3
        f["users"][:] = [0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2]
    if s["p"]:
        keep = (rng.random((B, s["n_v"] * s["d"] + s["n_h"] * L)) >= s["p"]).astype(np.uint8)
        f["keep"] = keep
    return f


def _margin_tables(f):
    """Per horizontal filter ``(h, f)`` the smallest gap between the best and the second-best window and (under relu)
    the smallest |pooled pre| over the rows, per fc1 unit the smallest |pre-activation| (under relu), and the largest
    |pre|: float64.  All-padding windows of one (row, height) count as ONE candidate: they tie exactly and the gradient
    does not depend on which of them wins."""
    with torch.no_grad():
        wt = ct.tensors(f["w"], torch.float64)
        _, pre, fc_pre = ct.features(wt, f["seq"], f["users"], f["ac_conv"], f["ac_fc"], f["keep"], f["p"])
    seq = np.asarray(f["seq"])
    _, first = np.unique(seq, axis=0, return_index=True)        # a row's windows depend on its sequence alone
    gap = np.full((f["L"], f["n_h"]), np.inf)
    zero = np.full((f["L"], f["n_h"]), np.inf)
    top = 0.0
    for h, p in enumerate(pre, start=1):
        p = p.numpy()
        top = max(top, float(np.abs(p).max()))
        for b in first:
            pad = np.array([not seq[b, t:t + h].any() for t in range(p.shape[2])])
            cols = [t for t in range(p.shape[2]) if not pad[t]] + ([int(np.flatnonzero(pad)[0])] if pad.any() else [])
            v = np.sort(p[b][:, cols], axis=1)
            if v.shape[1] > 1:
                gap[h - 1] = np.minimum(gap[h - 1], v[:, -1] - v[:, -2])
            if f["ac_conv"] == "relu":
                zero[h - 1] = np.minimum(zero[h - 1], np.abs(v[:, -1]))
    fc = np.abs(fc_pre.numpy()).min(0) if f["ac_fc"] == "relu" else np.full(f["d"], np.inf)
    return gap, zero, fc, top


def margins(f):
    """``(smallest gap, smallest distance from 0 under relu, largest |pre|)`` of the fixture."""
    gap, zero, fc, top = _margin_tables(f)
    return float(gap.min()), float(min(zero.min(), fc.min())), top


def margins_ok(f):
    gap, zero, top = margins(f)
    return gap > MARGIN * top and zero > MARGIN * top


def _reseed_until_margins(f, rng):
    """Draw the horizontal filters and the fc1 units that miss the margins again (same distributions) until none does."""
    w = f["w"]
    for _ in range(200):
        gap, zero, fc, top = _margin_tables(f)
        bad_f = np.argwhere((gap <= 2 * MARGIN * top) | (zero <= 2 * MARGIN * top))      # twice: top moves with the draws
        bad_u = np.flatnonzero(fc <= 2 * MARGIN * top)
        if not bad_f.size and not bad_u.size:
            return
        for i, k in bad_f:
            shape = w[f"conv_h.{i}.weight"].shape
            w[f"conv_h.{i}.weight"][k] = rng.standard_normal(shape[1:]) / np.sqrt(shape[2] * f["d"])
            w[f"conv_h.{i}.bias"][k] = rng.standard_normal() * 0.5
        for j in bad_u:
            w["fc1.weight"][j] = rng.standard_normal(w["fc1.weight"].shape[1]) / np.sqrt(w["fc1.weight"].shape[1])
            w["fc1.bias"][j] = rng.standard_normal() * 0.5
    raise AssertionError(f"{f['name']}: the margins do not hold after 200 rounds of re-seeding")


@functools.lru_cache(maxsize=None)
def fixture(name):
    """The fixture ``name`` from its own seed, its offending filters / fc1 units re-seeded until ``margins_ok``."""
    seed = 1000 * (NAMES.index(name) + 1)
    f = _build(name, seed)
    _reseed_until_margins(f, np.random.default_rng(seed + 500))
    f["seed"] = seed
    return f


def batch_of(f):
    return f["users"], f["seq"], f["pos"], f["neg"]


def keep_of(f):
    return None if f["keep"] is None else [f["keep"]]


@functools.lru_cache(maxsize=None)
def reference(name):
    """``(loss64, grads64, loss32, grads32)`` of the restatement; computed once, shared, never changed."""
    f = fixture(name)
    args = (f["w"], f["seq"], f["users"], f["pos"], f["neg"], f["ac_conv"], f["ac_fc"], f["l2"], f["keep"], f["p"])
    l64, g64 = ct.grads(*args, dtype=torch.float64)
    l32, g32 = ct.grads(*args, dtype=torch.float32)
    return l64, g64, l32, g32
