"""The fixtures of the BERT4Rec tests: the smallest shapes at which each path of csrc/bert4rec.hip can go wrong.

Weights are not the 0.02 initialisation: unit-scale tables, LayerNorm weights ``1 + 0.3 N(0, 1)``, biases
``0.2 N(0, 1)``, matrices uniform over ``+-1 / sqrt(fan_in)`` (as ``test_sasrec_gpu.synthetic``), so that no term
vanishes below the tolerance.

What each fixture is there for (``T`` crosses the 64-key chunk, ``n_items`` the 64-item tile, ``n_lab`` the 32-row
tile of the cross-entropy):

=============  ===  ===  ==  ===  ===  =====  =====  ==========================================================
name             T    D   H    F    I  n_lab  batch  also
=============  ===  ===  ==  ===  ===  =====  =====  ==========================================================
t1               1   16   1    1    1      3      4  one class: the loss is exactly 0; last sequence all padding
one_seq          5  128   8   40   63      1      1  a batch of one; its only label is its last position
t64             64   64   2  512   64     31      2  exact key chunk and item tile; last sequence all padding
t65             65   64   1   40   65     32      2  ragged chunk, one item over; a sequence with ONE real key
t200           200   64   2   40  130     33      2  the default length, several item tiles, two blocks
no_labels        5   16   1   40   63      0      2  nothing to predict
bias_spread      5   32   2   40  130      2      2  out_bias spread >> scores; a label at the row maximum and
                                                      one far below it
catalogue       20   32   2   40 2200     70      4  35 item tiles (the last holds 24 items) under 3 row tiles: 12
                                                      splits of 3 tiles, the last of 2 -- every cross-entropy block
                                                      streams several item tiles (running max / sum, the label
                                                      picked on the way past, dh summed over tiles)
slabs           65   64   1   40  650     33      9  B T = 585 > 512: every weight gradient in two batch slabs of
                                                      304 and 281 rows, folded in slab order
=============  ===  ===  ==  ===  ===  =====  =====  ==========================================================
"""
import functools

import numpy as np
import torch

import bert4rec_torch as bt

NAMES = ("t1", "one_seq", "t64", "t65", "t200", "no_labels", "bias_spread", "catalogue", "slabs")
#        T, D, H, F, I, n_lab, B, blocks
SHAPES = {"t1": (1, 16, 1, 1, 1, 3, 4, 1), "one_seq": (5, 128, 8, 40, 63, 1, 1, 1),
          "t64": (64, 64, 2, 512, 64, 31, 2, 1), "t65": (65, 64, 1, 40, 65, 32, 2, 1),
          "t200": (200, 64, 2, 40, 130, 33, 2, 2), "no_labels": (5, 16, 1, 40, 63, 0, 2, 1),
          "bias_spread": (5, 32, 2, 40, 130, 2, 2, 1), "catalogue": (20, 32, 2, 40, 2200, 70, 4, 1),
          "slabs": (65, 64, 1, 40, 650, 33, 9, 1)}


def weights(I, T, D, nb, Fd, rng):
    w = {}
    for k, shape in bt.shapes(I, T, D, nb, Fd).items():
        if k in ("item_emb.weight", "pos_emb.weight"):
            w[k] = rng.standard_normal(shape)
        elif "layernorm" in k and k.endswith("weight"):
            w[k] = 1.0 + 0.3 * rng.standard_normal(shape)
        elif k.endswith("bias"):
            w[k] = 0.2 * rng.standard_normal(shape)
        else:
            w[k] = rng.uniform(-1, 1, shape) / np.sqrt(shape[-1])
        w[k] = w[k].astype(np.float32)
    w["item_emb.weight"][0] = 0
    return w


def histories(I, T, B, rng, lengths):
    seq = np.zeros((B, T), dtype=np.int64)
    for b, n in enumerate(lengths):
        if n:
            seq[b, T - n:] = rng.integers(1, I + 1, n)
    return seq


def mask(seq, at, I):
    """``(seq with [MASK] at the flat positions ``at``, labels)``."""
    labels = np.zeros_like(seq)
    s = seq.copy()
    labels.reshape(-1)[at] = s.reshape(-1)[at]
    s.reshape(-1)[at] = I + 1
    return s, labels


@functools.lru_cache(maxsize=None)
def fixture(name):
    """``dict(name, T, D, H, F, I, B, blocks, w, seq, labels)``; built once, never modified by a test."""
    T, D, H, Fd, I, n_lab, B, nb = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    w = weights(I, T, D, nb, Fd, rng)
    if name in ("t1", "t64"):                       # the last sequence is all padding
        lengths = [T] * (B - 1) + [0]
    elif name == "t65":                             # the second sequence has a single real key
        lengths = [T, 1]
    elif name == "t200":
        lengths = [T, 77]
    else:
        lengths = [T] + [max(1, T - 2)] * (B - 1)
    seq = histories(I, T, B, rng, lengths)
    real = np.flatnonzero(seq.reshape(-1))
    if name == "one_seq":
        at = np.array([T - 1])                      # its only labelled position is its last
    elif name == "t65":
        at = np.sort(np.concatenate([rng.choice(real[:-1], n_lab - 1, replace=False), real[-1:]]))   # ... and is labelled
    elif name == "bias_spread":
        at = np.array([1, T + T - 1])
    else:
        at = np.sort(rng.choice(real, n_lab, replace=False))
    assert at.size == n_lab
    seq, labels = mask(seq, at, I)
    if name == "bias_spread":
        w["out_bias"] = (30.0 * rng.standard_normal(I + 1)).astype(np.float32)
        w["out_bias"][0] = np.abs(w["out_bias"]).max()      # never read: as a class, padding would win every row
        wt = bt.tensors(w, torch.float64)           # the labelled rows' own logits, from the restatement
        with torch.no_grad():
            h = bt.head(wt, bt.forward(wt, seq, H).reshape(-1, D)[torch.as_tensor(at)])
            logits = (h @ wt["item_emb.weight"][1:I + 1].T + wt["out_bias"][1:]).numpy()
        labels.reshape(-1)[at[0]] = 1 + int(logits[0].argmax())       # the row maximum
        labels.reshape(-1)[at[1]] = 1 + int(logits[1].argmin())       # far below it
        assert np.ptp(w["out_bias"][1:]) > 2 * np.ptp(logits - w["out_bias"][1:])
    return dict(name=name, T=T, D=D, H=H, F=Fd, I=I, B=B, blocks=nb, w=w, seq=seq, labels=labels)


@functools.lru_cache(maxsize=None)
def reference(name):
    """``(loss64, g64, loss32, g32)`` of the restatement on the fixture: computed once, shared, left unchanged."""
    f = fixture(name)
    l64, g64 = bt.grads(f["w"], f["seq"], f["labels"], f["H"], dtype=torch.float64)
    l32, g32 = bt.grads(f["w"], f["seq"], f["labels"], f["H"], dtype=torch.float32)
    return l64, g64, l32, g32


def keep_masks(f, p, seed):
    """Explicit keep masks of the engine's shapes for fixture ``f`` at dropout rate ``p``."""
    rng = np.random.default_rng(seed)
    B, T, D, H = f["B"], f["T"], f["D"], f["H"]
    shapes = [(B * T, D)]
    for _ in range(f["blocks"]):
        shapes += [(B * H, T, T), (B * T, D), (B * T, D)]
    return [(rng.random(s) >= p).astype(np.uint8) for s in shapes]
