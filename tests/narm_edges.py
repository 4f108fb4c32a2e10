"""The synthetic NARM shapes the GPU edge tests run against the fp64 restatement (tests/narm_numpy.py), and the inputs the
host-side visibility checks reuse.  Each shape is ``(I, D, H, L, T, B, (dropout_input, dropout_hidden))``.

Which constant of csrc/narm.hip each value straddles:

* the session tile of the recurrence workgroups, 16 sessions (``kNarmTile``): B = 1 (one row of one tile), 2, 17 (a full
  tile and one row of the next), 70 (four full tiles and a ragged fifth);
* the MFMA's K step of 4 and its 16-wide output tile: W_hh is packed to ``pad4(H)`` inputs and ``pad16(H)`` outputs --
  H = 16 (both exact), 18 (neither), 20 (K exact, tile ragged), 100 (K exact, tile ragged, seven tiles over four
  waves), 112, 128 (the limit, both exact);
* the LDS-residency boundary: the forward keeps all of W_hh in LDS up to H = 108, the backward up to H = 100 -- H = 100
  is the last width that is fully resident both ways, H = 112 keeps 320 of 336 rows forward (the split falls inside the
  n gate) and 296 of 336 backward, H = 128 keeps 272 of 384 forward and 252 of 384 backward;
* the cross-entropy's per-row stride of 256 threads (``kBlock``): I = 2 and 23 (one partial trip), 257 (one element into
  the second trip), 300, 1500 (six trips, the last ragged);
* the wave-per-session attention's two values per lane (H <= 64 / H > 64) and the GEMM's 64 x 64 tiles with a K tile of
  32: D = 12, 32, 128;
* T = 1 (no recurrent weight gradient: h_0 = 0), 2, 33; L = 1, 2, 3 (the stacked layers read the layer below).

Every batch has its lengths in NO particular order, holds a session of length T and (where B > 1) one of length 1, and --
where a session is at least 3 long -- a 0 inside a session's length.
"""
import numpy as np

import narm_numpy as nn_
from helpers import float64_oracle, to64

SHAPES = [
    (2, 12, 16, 1, 1, 1, (0.0, 0.0)),
    (23, 12, 20, 1, 2, 17, (0.0, 0.0)),
    (1500, 32, 100, 2, 33, 17, (0.0, 0.0)),
    (50, 128, 128, 3, 5, 70, (0.0, 0.0)),
    (23, 32, 18, 2, 33, 2, (0.0, 0.0)),
    (300, 12, 100, 1, 2, 70, (0.0, 0.0)),
    (23, 32, 20, 1, 7, 17, (0.25, 0.5)),
    (257, 128, 16, 3, 33, 17, (0.0, 0.0)),
    (60, 32, 112, 1, 9, 33, (0.0, 0.0)),
]
# the one shape whose attention gradients are ONE cancelling dot product (see alpha_floors)
NEEDS_FLOOR = {(2, 12, 16, 1, 1, 1, (0.0, 0.0))}


def shape_id(shape):
    I, D, H, L, T, B, p = shape
    return f"I{I}-D{D}-H{H}-L{L}-T{T}-B{B}" + ("-drop" if any(p) else "")


def synthetic(shape, seed=0):
    """``(weights, (seq, target, lens), keep)`` for a shape; the same seed gives the same inputs everywhere."""
    I, D, H, L, T, B, p = shape
    rng = np.random.default_rng(seed + 1000 * I + H + T)
    w = {}
    for k, s in nn_.shapes(I, D, H, L).items():
        scale = 1.0 if k == "emb.weight" else 1.0 / np.sqrt(H)
        w[k] = (rng.uniform(-1, 1, s) * scale).astype(np.float32)
    w["emb.weight"][0] = 0
    lens = rng.integers(1, T + 1, B)
    full = int(rng.integers(0, B))
    if B > 1:
        lens[(full + 1) % B] = 1
    lens[full] = T
    seq = np.zeros((T, B), dtype=np.int64)
    for b, n in enumerate(lens):
        seq[:n, b] = rng.integers(1, I, n)
    long_ones = np.nonzero(lens >= 3)[0]
    if long_ones.size:
        seq[1, long_ones[0]] = 0
    target = rng.integers(0, I, B)
    keep = None
    if any(p):
        keep = [(rng.random((T, B, D)) >= p[0]).astype(np.uint8).reshape(-1),
                (rng.random((B, 2 * H)) >= p[1]).astype(np.uint8).reshape(-1)]
    return w, (seq, target, lens), keep


def alpha_floors(w, batch, keep, p):
    """Scale floors for ``a_1``, ``a_2`` and ``v_t``, from the terms summed.  Their gradients all go through
    ``d alpha[b, t] = sum_j d c_local[b, j] * gru_out[b, t, j]``: a dot product of H terms of either sign, whose fp32
    rounding error is relative to ``sum_j |terms|``, not to the (cancelled) result.  With many (b, t) positions the
    gradients' own scale is of that size anyway; with ONE position (B = 1, T = 1) the three gradients ARE that one
    cancelled dot product times a factor, and their scale says nothing about the error any summation order makes.  The
    floor is each gradient's formula evaluated in fp64 with ``|d alpha|`` replaced by ``sum_j |terms|`` and every other
    factor by its magnitude."""
    with float64_oracle(nn_):
        _, _, c = nn_.narm_grads(to64(w), batch, keep, p, with_cache=True)
    H = c["H"]
    out, s, mask, hT = np.abs(c["out"]), c["s"], c["mask"], np.abs(c["hT"])
    dabs = (np.abs(c["dcl"])[None] * out).sum(-1)
    dpre = dabs[:, :, None] * np.abs(c["w"]["v_t.weight"][0])[None, None] * s * (1.0 - s)
    return {"v_t.weight": float((dabs[:, :, None] * s).sum((0, 1)).max()),
            "a_1.weight": float((dpre.reshape(-1, H).T @ out.reshape(-1, H)).max()),
            "a_2.weight": float(((dpre * mask).sum(0).T @ hT).max())}


def floor_fn(shape, w, batch, keep):
    if shape not in NEEDS_FLOOR:
        return None
    floors = alpha_floors(w, batch, keep, shape[6])
    return lambda k: floors.get(k, 0.0)
