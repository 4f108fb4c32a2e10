"""Fixtures of the SASRec tile-edge tests, shared by tests/test_sasrec_edges_host.py (which shows on the CPU that the
inputs can see one misplaced keep byte) and tests/test_sasrec_edges_gpu.py (which runs the kernels on those very inputs).

The weights are ``test_sasrec_gpu.synthetic``'s with two scales chosen, not taken as they come: a unit-normal item table
gives logits of size sqrt(D) (the BCE saturates and a token's gradient vanishes) and keys of size sqrt(D) (the softmax
is sharp and most keep bytes multiply a probability of ~0), so one flipped attention keep byte moves no gradient by more
than the parity tolerance.  ``EMB_SCALE / sqrt(D)`` on the item table and ``QK_SCALE`` on the query / key rows of every
``in_proj_weight`` make every token's logit and every causal probability count."""
import numpy as np

import sasrec_numpy as sn
from helpers import REL, float64_oracle, to64
from test_sasrec_gpu import synthetic

ITEMS = 50
EMB_SCALE, QK_SCALE = 1.0, 0.25
L2 = 0.05

# (D, H, T, B, num_blocks, p)
DROPOUT_SHAPES = [(64, 2, 65, 3, 2, 0.25), (64, 1, 33, 2, 1, 0.5), (48, 3, 96, 2, 2, 0.2), (128, 8, 129, 2, 2, 0.2),
                  (128, 2, 256, 2, 1, 0.1), (16, 1, 64, 3, 3, 0.3)]
# (D, H, T, B, num_blocks)
PLAIN_SHAPES = [(64, 2, 32, 2, 2), (64, 2, 64, 3, 1), (128, 4, 128, 2, 2), (128, 2, 256, 2, 2), (96, 3, 33, 3, 2),
                (16, 1, 129, 2, 3)]
# the seams of the 32-query tile, the 64-key chunk and the key-side kernel's 32-key tile; (None, j) is the last query
SEAMS = [(None, None), (None, 0), (None, 63), (None, 64), (32, 31), (32, 0), (31, 31), (64, 63), (64, 64), (63, 0)]


def mask_shapes(D, H, T, B, nb):
    """What ``SASRecEngine._mask_shapes`` returns (the GPU test asserts it): embedding; per block attention, two FFN."""
    out = [(B * T, D)]
    for _ in range(nb):
        out += [(B * H, T, T), (B * T, D), (B * T, D)]
    return out


def edge_weights_and_batch(D, H, T, B, nb):
    """Sequence 0 full length, the others left-padded, with more than one sequence the last all padding."""
    w, batch = synthetic(ITEMS, D, H, T, B, nb, seed=1000 * nb + D + T, all_padding_row=B > 1)
    w["item_emb.weight"] *= np.float32(EMB_SCALE / np.sqrt(D))
    for b in range(nb):
        w[f"attention_layers.{b}.in_proj_weight"][:2 * D] *= np.float32(QK_SCALE)
    return w, batch


def draw_keep_masks(D, H, T, B, nb, p, seed):
    rng = np.random.default_rng(seed)
    return [(rng.random(s) >= p).astype(np.uint8) for s in mask_shapes(D, H, T, B, nb)]


def dropout_fixture(D, H, T, B, nb, p):
    """``(w, batch, keep)`` of one of DROPOUT_SHAPES."""
    w, batch = edge_weights_and_batch(D, H, T, B, nb)
    return w, batch, draw_keep_masks(D, H, T, B, nb, p, seed=D * T + H)


def seam_positions(T):
    """The (i, j) of SEAMS that exist at length T (inside the sequence and causal), without repeats."""
    out = []
    for i, j in SEAMS:
        i = T - 1 if i is None else i
        j = T - 1 if j is None else j
        if i < T and j <= i and (i, j) not in out:
            out.append((i, j))
    return out


def reference(w, batch, H, l2, keep, p):
    """``(loss64, g64, g32)``: the restatement in fp64 and its fp32 self's gradients."""
    _, g32 = sn.sasrec_grads(w, batch, H, l2, keep, p)
    with float64_oracle(sn):
        loss64, g64 = sn.sasrec_grads(to64(w), batch, H, l2, keep, p)
    return loss64, g64, g32


def tolerances(g32, g64):
    """Per tensor what ``helpers.assert_grads_as_accurate`` allows: REL of the scale + twice the fp32 self's error."""
    return {k: REL * float(np.abs(g64[k]).max()) + 2.0 * float(np.abs(g32[k] - g64[k]).max()) for k in g64}


def flip_margin(w, batch, H, l2, keep, p, g64, tol, mask, index):
    """Flip byte ``index`` of keep mask ``mask``: the largest move of a tensor of the fp64 gradient, in units of that
    tensor's tolerance."""
    flipped = list(keep)
    flipped[mask] = keep[mask].copy()
    flipped[mask][index] ^= 1
    with float64_oracle(sn):
        _, moved = sn.sasrec_grads(to64(w), batch, H, l2, flipped, p)
    return max(float(np.abs(moved[k] - g64[k]).max()) / tol[k] for k in g64)
