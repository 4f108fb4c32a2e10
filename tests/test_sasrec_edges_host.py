"""The inputs of tests/test_sasrec_edges_gpu.py can see ONE misplaced dropout keep byte: on the CPU, with the fp64
restatement alone, flipping a single byte at every seam of the attention kernels' tiles (and one byte of the embedding
mask and of each FFN mask) moves at least one gradient tensor by 10x what the GPU test's gradient bound allows.  CPU
only; ``pytest -s`` shows the measured margins."""
import numpy as np
import pytest

import sasrec_edges as se
import sasrec_numpy as sn
from helpers import float64_oracle, to64

MIN_MARGIN = 10.0


def test_seam_positions():
    """Which of the listed (i, j) exist at each length: none is dropped but those outside the sequence."""
    assert se.seam_positions(256) == [(255, 255), (255, 0), (255, 63), (255, 64), (32, 31), (32, 0), (31, 31), (64, 63),
                                      (64, 64), (63, 0)]
    assert se.seam_positions(65) == [(64, 64), (64, 0), (64, 63), (32, 31), (32, 0), (31, 31), (63, 0)]
    assert se.seam_positions(64) == [(63, 63), (63, 0), (32, 31), (32, 0), (31, 31)]
    assert se.seam_positions(33) == [(32, 32), (32, 0), (32, 31), (31, 31)]
    assert [len(se.seam_positions(T)) for T in (96, 129)] == [10, 10]


@pytest.mark.parametrize("D,H,T,B,nb,p", se.DROPOUT_SHAPES)
def test_fixture_layout(D, H, T, B, nb, p):
    """Sequence 0 is full length, the last one all padding, the others left-padded; every mask drops and keeps."""
    w, (seq, pos, neg), keep = se.dropout_fixture(D, H, T, B, nb, p)
    assert (seq[0] != 0).all() and (pos[0] != 0).all()
    assert not seq[B - 1].any() and not pos[B - 1].any()
    real = seq != 0
    assert (real[:, 1:] >= real[:, :-1]).all(), "padding is on the left"
    assert [k.shape for k in keep] == se.mask_shapes(D, H, T, B, nb) and len(keep) == 1 + 3 * nb
    for k in keep:
        assert k.dtype == np.uint8 and abs(float(k.mean()) - (1 - p)) < 0.05
    assert float(np.abs(w["item_emb.weight"][0]).max()) == 0.0


@pytest.mark.parametrize("D,H,T,B,nb,p", se.DROPOUT_SHAPES)
def test_one_flipped_keep_byte_is_visible(D, H, T, B, nb, p):
    w, batch, keep = se.dropout_fixture(D, H, T, B, nb, p)
    _, g64, g32 = se.reference(w, batch, H, se.L2, keep, p)
    tol = se.tolerances(g32, g64)
    with float64_oracle(sn):
        _, cache = sn.sasrec_forward(to64(w), batch[0], H, keep, p)
    margins = {}
    last = T - 1                                   # sequence 0's last token is row T - 1 of [B * T, D]
    margins["embedding", last, 0] = se.flip_margin(w, batch, H, se.L2, keep, p, g64, tol, 0, (last, 0))
    for blk in range(nb):
        for i, j in se.seam_positions(T):          # head H - 1 of sequence 0 is slice H - 1 of [B * H, T, T]
            margins[f"attention {blk}", i, j] = se.flip_margin(w, batch, H, se.L2, keep, p, g64, tol, 1 + 3 * blk,
                                                               (H - 1, i, j))
        alive = int(np.argmax(cache["blocks"][blk]["pre1"][0, last]))
        assert cache["blocks"][blk]["pre1"][0, last, alive] > 0
        margins[f"dropout1 {blk}", last, alive] = se.flip_margin(w, batch, H, se.L2, keep, p, g64, tol, 2 + 3 * blk,
                                                                 (last, alive))
        margins[f"dropout2 {blk}", last, 0] = se.flip_margin(w, batch, H, se.L2, keep, p, g64, tol, 3 + 3 * blk,
                                                             (last, 0))
    for (mask, i, j), m in margins.items():
        print(f"D {D} H {H} T {T}: {mask} byte ({i}, {j}) moves a gradient by {m:.1f} x its tolerance")
    print(f"D {D} H {H} T {T} B {B} blocks {nb} p {p}: smallest margin {min(margins.values()):.1f}")
    blind = {k: round(m, 2) for k, m in margins.items() if m < MIN_MARGIN}
    assert not blind, f"the gradient bound cannot see these bytes at {MIN_MARGIN:g} x: {blind}"
