"""Fixtures of the TiSASRec tile-edge tests, shared by tests/test_oracle_golden_tisasrec.py (which shows on the CPU that
the inputs can see one misplaced time-mask byte) and tests/test_tisasrec_gpu.py (which runs the kernels on those inputs).

Weight scales are chosen as tests/sasrec_edges.py chooses them, for the same reason: ``EMB_SCALE / sqrt(D)`` on the item
table and ``QK_SCALE`` on ``Q_w`` / ``K_w``, on ``abs_pos_K_emb`` and on ``time_matrix_K_emb`` keep the softmax soft, so
that every causal probability -- and with it every byte of the two ``[B, T, T, D]`` masks -- counts in some gradient."""
import functools

import numpy as np

import tisasrec_numpy as tn
from helpers import REL, float64_oracle, to64

ITEMS = 50
EMB_SCALE, QK_SCALE = 1.0, 0.25
L2 = 0.05

# (D, H, T, B, num_blocks, time_span, p).  Query tile: 32 rows (16 at head width 64); key chunk: 64.
#   (64, 2, 65, 3, 2, 16)   head width 32, three query tiles (the last of one row), a second key chunk of one key, two
#                           blocks: the position and time masks are shared by both
#   (64, 1, 33, 2, 1, 1)    head width 64 (three 16-row tiles, the last of one row), the smallest time_span
#   (48, 3, 32, 3, 2, 16)   head width 16, D no power of two, T exactly one query tile
#   (64, 1, 256, 3, 1, 256) every limit at once: the LDS of one block holds the 257 x 64 slice next to the score rows
#   (32, 1, 129, 3, 1, 256) three key chunks (the last of one key), head width 32 with the largest table
#   (96, 3, 64, 3, 1, 16)   D = 96, T exactly one key chunk
EDGE_SHAPES = [(64, 2, 65, 3, 2, 16, 0.25), (64, 1, 33, 2, 1, 1, 0.5), (48, 3, 32, 3, 2, 16, 0.2),
               (64, 1, 256, 3, 1, 256, 0.1), (32, 1, 129, 3, 1, 256, 0.2), (96, 3, 64, 3, 1, 16, 0.3)]
# the shapes whose single-byte visibility the CPU test measures (two dozen fp64 gradients each: the short ones)
VISIBLE_SHAPES = [EDGE_SHAPES[0], EDGE_SHAPES[1], EDGE_SHAPES[2]]
PATTERN_SHAPE = (64, 2, 65, 3, 1, 16)          # D, H, T, B, blocks, span of the time-matrix pattern cases
# seams of the query tiles (16 or 32 rows) and of the 64-key chunk; (None, j) is the last query
SEAMS = [(None, None), (None, 0), (None, 63), (None, 64), (32, 31), (32, 0), (31, 31), (16, 15), (16, 16), (64, 63),
         (64, 64), (63, 0)]


def mask_shapes(D, H, T, B, nb):
    """What ``TiSASRecEngine._mask_shapes`` returns (the GPU test asserts it)."""
    out = [(B * T, D)] * 3 + [(B, T, T, D)] * 2
    for _ in range(nb):
        out += [(H * B, T, T), (B * T, D), (B * T, D)]
    return out


def synthetic(I, D, H, T, B, nb, span, seed, all_padding_row):
    """Weights, a batch ``(seq, tm, pos, neg)`` and its ``time_seq``: sequence 0 full length, the last one all padding
    (with more than one sequence), the others left-padded; time stamps grow by 0 .. span / 2 per step from a start
    beyond ``span``, so that the matrix holds 0, small intervals and the clamp."""
    rng = np.random.default_rng(seed)
    w = {}
    for k, shape in tn.shapes(I, T, span, D, nb).items():
        if k.endswith("emb.weight"):
            w[k] = rng.standard_normal(shape)
        elif "layernorm" in k and k.endswith("weight"):
            w[k] = 1.0 + 0.3 * rng.standard_normal(shape)
        elif k.endswith("bias"):
            w[k] = 0.2 * rng.standard_normal(shape)
        else:
            w[k] = rng.uniform(-1, 1, shape) / np.sqrt(D)
        w[k] = w[k].astype(np.float32)
    w["item_emb.weight"][0] = 0
    seq, pos, neg, ts = (np.zeros((B, T), dtype=np.int64) for _ in range(4))
    for b in range(B):
        n = T if b == 0 else int(rng.integers(1, T + 1))
        if all_padding_row and b == B - 1:
            continue
        items = rng.integers(1, I + 1, n + 1)
        seq[b, T - n:], pos[b, T - n:] = items[:-1], items[1:]
        neg[b, T - n:] = rng.integers(1, I + 1, n)
        ts[b, T - n:] = span + 1 + np.cumsum(rng.integers(0, span // 2 + 2, n))
    tm = np.minimum(np.abs(ts[:, :, None] - ts[:, None, :]), span).astype(np.int32)
    return w, (seq, tm, pos, neg), ts


def edge_weights_and_batch(D, H, T, B, nb, span):
    w, batch, ts = synthetic(ITEMS, D, H, T, B, nb, span, seed=1000 * nb + D + T + span, all_padding_row=B > 1)
    w["item_emb.weight"] *= np.float32(EMB_SCALE / np.sqrt(D))
    for k in ("abs_pos_K_emb.weight", "time_matrix_K_emb.weight"):
        w[k] *= np.float32(QK_SCALE)
    for b in range(nb):
        for m in ("Q_w", "K_w"):
            w[f"attention_layers.{b}.{m}.weight"] *= np.float32(QK_SCALE)
    return w, batch, ts


def draw_keep_masks(D, H, T, B, nb, p, seed):
    """Random keep bytes; the ATTENTION masks keep the seam positions of sequence 0's last head, so that a time-mask byte
    there is not hidden behind a probability every block happens to drop."""
    rng = np.random.default_rng(seed)
    keep = [(rng.random(s) >= p).astype(np.uint8) for s in mask_shapes(D, H, T, B, nb)]
    for b in range(nb):
        for i, j in seam_positions(T):
            keep[5 + 3 * b][(H - 1) * B, i, j] = 1
    return keep


@functools.lru_cache(maxsize=None)
def edge_fixture(D, H, T, B, nb, span, p):
    """``(w, batch, keep)`` of one of EDGE_SHAPES (``keep`` None at p = 0); computed once, never written to."""
    w, batch, _ = edge_weights_and_batch(D, H, T, B, nb, span)
    return w, batch, (draw_keep_masks(D, H, T, B, nb, p, seed=D * T + H) if p > 0 else None)


def seam_positions(T):
    out = []
    for i, j in SEAMS:
        i = T - 1 if i is None else i
        j = T - 1 if j is None else j
        if i < T and j <= i and (i, j) not in out:
            out.append((i, j))
    return out


def key_bias_floor(cache):
    """Scale floor of a gradient tensor for ``helpers.assert_grads_as_accurate``, from the cache of a restatement run
    (``with_cache=True``).  ``K_w.bias`` shifts every score of a row alike and cancels in the softmax: its exact
    gradient is ZERO (1e-17 in fp64) although it is the sum over all tokens of the rows of dK, which do not vanish.
    An fp32 sum of terms that cancel is off by the rounding of its TERMS, not of its result (helpers.grad_scale_floor
    makes the same point for MF's biases), so that tensor is held to REL of the largest column's sum of |dK|.  Every
    other tensor: no floor."""
    def floor(k):
        if k.endswith("K_w.bias"):
            return float(np.abs(cache["blocks"][int(k.split(".")[1])]["dk"]).sum((0, 1)).max())
        return 0.0
    return floor


def reference(w, batch, H, l2, keep, p):
    """``(loss64, g64, g32, floor)``: the restatement in fp64, its fp32 self's gradients and ``key_bias_floor``."""
    _, g32 = tn.tisasrec_grads(w, batch, H, l2, keep, p)
    with float64_oracle(tn):
        loss64, g64, cache = tn.tisasrec_grads(to64(w), batch, H, l2, keep, p, with_cache=True)
    return loss64, g64, g32, key_bias_floor(cache)


def tolerances(g32, g64, floor):
    """Per tensor what ``helpers.assert_grads_as_accurate`` allows with ``floor``."""
    return {k: REL * max(float(np.abs(g64[k]).max()), floor(k)) + 2.0 * float(np.abs(g32[k] - g64[k]).max())
            for k in g64}


def flip_margin(w, batch, H, l2, keep, p, g64, tol, mask, index):
    """Flip byte ``index`` of keep mask ``mask``: the largest move of a tensor of the fp64 gradient, in units of that
    tensor's tolerance."""
    flipped = list(keep)
    flipped[mask] = keep[mask].copy()
    flipped[mask][index] ^= 1
    with float64_oracle(tn):
        _, moved = tn.tisasrec_grads(to64(w), batch, H, l2, flipped, p)
    return max(float(np.abs(moved[k] - g64[k]).max()) / tol[k] for k in g64)
