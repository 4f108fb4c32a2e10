"""GPU parity tests of SASRec (csrc/sasrec.hip) at the tile edges the goldens and ``test_shapes_against_the_restatement``
do not reach: gradients under dropout with explicit keep masks wherever more than one 32-query tile, 64-key chunk or
32-key tile is in play (inputs that tests/test_sasrec_edges_host.py shows to see a single misplaced keep byte), the exact
tile multiples and ``kSasMaxLen`` without dropout, a batch shorter than ``maxlen``, a negative id of 0, one Adam step
under dropout with explicit and with device-drawn masks, and ``predict`` at a ragged length.  The yardsticks are those of
tests/test_sasrec_gpu.py: the fp64 restatement, ``assert_scalar_close`` and ``assert_grads_as_accurate``."""
import functools

import numpy as np
import pytest

import sasrec_edges as se
import sasrec_numpy as sn
from helpers import assert_grads_as_accurate, assert_scalar_close, assert_step_close, assert_tensor_close
from helpers import float64_oracle, to64
from test_oracle_golden_sasrec import sas_band
from test_sasrec_gpu import full_batch, get_weights, make_engine, np_grads

pytestmark = pytest.mark.gpu

STEP_SHAPE = se.DROPOUT_SHAPES[0]         # (64, 2, 65, 3, 2, 0.25): parts 1, 4 and 5 share it
LR = 1e-3


@functools.lru_cache(maxsize=None)
def dropout_case(shape):
    """``(w, batch, keep, loss64, g64, g32)`` of one of DROPOUT_SHAPES, computed once and never written to."""
    D, H, T, B, nb, p = shape
    w, batch, keep = se.dropout_fixture(*shape)
    return (w, batch, keep) + se.reference(w, batch, H, se.L2, keep, p)


def features64(w, seq, H):
    with float64_oracle(sn):
        return sn.sasrec_forward(to64(w), seq, H)[0]


def check_loss_and_grads(loss, grads, loss64, g64, g32, what):
    grads = np_grads(grads)
    print(f"{what}: loss {loss!r} vs exact {loss64!r}")
    for k in g64:
        print(f"  grad {k}: err vs exact {np.abs(grads[k].reshape(g64[k].shape) - g64[k]).max():.3e}, fp32 restatement's "
              f"{np.abs(g32[k] - g64[k]).max():.3e}, scale {np.abs(g64[k]).max():.3e}")
    assert_scalar_close(loss, loss64, what=f"{what}: loss")
    assert_grads_as_accurate(grads, g32, g64, what=f"{what}: grad")
    assert float(np.abs(grads["item_emb.weight"][0]).max()) == 0.0, "a gradient reached the padding row"


@pytest.mark.parametrize("D,H,T,B,nb,p", se.DROPOUT_SHAPES)
def test_dropout_gradients_at_the_tile_edges(hip_device, D, H, T, B, nb, p):
    """Part 1.  (64, 2, 65): head width 32, three query tiles (the last of one row), a second key chunk of one key,
    M = 195; (64, 1, 33): head width 64, a second query tile of one row; (48, 3, 96): head width 16 with H, B > 1, D no
    multiple of 64, T a multiple of 32; (128, 8, 129): three key chunks, a fifth key tile of one row; (128, 2, 256): T at
    kSasMaxLen; (16, 1, 64): the narrowest D, three blocks, T exactly one key chunk.  At the first shape the eval-mode
    features afterwards are the mask-free forward's: the masks do not leak."""
    w, batch, keep, loss64, g64, g32 = dropout_case((D, H, T, B, nb, p))
    eng = make_engine(w, se.ITEMS, D, H, T, nb, p=p, B=B, l2=se.L2)
    assert [tuple(s) for s in eng._mask_shapes(B, T)] == se.mask_shapes(D, H, T, B, nb)
    loss, grads = eng.backward_only(full_batch(batch), keep_masks=keep)
    check_loss_and_grads(loss, grads, loss64, g64, g32, f"D {D} H {H} T {T} B {B} blocks {nb} p {p}")
    if (D, H, T, B, nb, p) == STEP_SHAPE:
        eng.model.eval()
        feats = eng.model.log2feats(batch[0]).cpu().numpy()
        assert_tensor_close(feats, features64(w, batch[0], H), what="log2feats in eval mode")


def check_plain(eng, w, batch, H, what):
    """The assertions of ``test_shapes_against_the_restatement``."""
    loss64, g64, g32 = se.reference(w, batch, H, se.L2, None, 0.0)
    loss, grads = eng.backward_only(full_batch(batch))
    check_loss_and_grads(loss, grads, loss64, g64, g32, what)
    feats = eng.model.log2feats(batch[0]).cpu().numpy()
    assert_tensor_close(feats, features64(w, batch[0], H), what=f"{what}: log2feats")


@pytest.mark.parametrize("D,H,T,B,nb", se.PLAIN_SHAPES)
def test_exact_tile_edges_without_dropout(hip_device, D, H, T, B, nb):
    """Part 3.  T = 32, 64, 128 (exact tile multiples), 33 and 129 (one past), 256 = kSasMaxLen (the LDS score row used
    to its last column); D = 16 and 96 (a wave's two LayerNorm passes not filled evenly); one and three blocks."""
    w, batch = se.edge_weights_and_batch(D, H, T, B, nb)
    eng = make_engine(w, se.ITEMS, D, H, T, nb, l2=se.L2, B=B)
    check_plain(eng, w, batch, H, f"D {D} H {H} T {T} B {B} blocks {nb}")


def test_negative_id_zero_beside_a_real_positive(hip_device):
    """``neg = 0`` where ``pos != 0``: the negative logit is 0 and counts in the loss, no gradient reaches row 0."""
    D, H, T, B, nb = 96, 3, 33, 3, 2
    w, (seq, pos, neg) = se.edge_weights_and_batch(D, H, T, B, nb)
    neg = neg.copy()
    for b, t in ((0, 0), (0, 31), (0, T - 1), (1, T - 1)):
        assert pos[b, t] != 0
        neg[b, t] = 0
    eng = make_engine(w, se.ITEMS, D, H, T, nb, l2=se.L2, B=B)
    check_plain(eng, w, (seq, pos, neg), H, "negative id 0")


def test_sequences_shorter_than_maxlen(hip_device):
    """An engine of maxlen 100 on a batch of length 37: the restatement on ``pos_emb.weight[:37]``, the positional
    gradient's rows 37.. exactly zero; then length 100 (the workspace regrows), then 37 again with the first result."""
    D, H, T, B, nb, maxlen = 64, 2, 37, 3, 2, 100
    w, long_batch = se.edge_weights_and_batch(D, H, maxlen, B, nb)
    _, short_batch = se.edge_weights_and_batch(D, H, T, B, nb)
    assert 0 < (short_batch[0][1] != 0).sum() < T, "the second sequence is left-padded"
    w_short = dict(w)
    w_short["pos_emb.weight"] = w["pos_emb.weight"][:T]
    loss64, g64, g32 = se.reference(w_short, short_batch, H, se.L2, None, 0.0)
    eng = make_engine(w, se.ITEMS, D, H, maxlen, nb, l2=se.L2, B=B)

    def run_short(what):
        loss, grads = eng.backward_only(full_batch(short_batch))
        grads = dict(grads)
        g_pos = grads["pos_emb.weight"].cpu().numpy().reshape(maxlen, D)
        assert float(np.abs(g_pos[T:]).max()) == 0.0, "a gradient reached a positional row the batch does not use"
        grads["pos_emb.weight"] = grads["pos_emb.weight"].reshape(maxlen, D)[:T]
        check_loss_and_grads(loss, grads, loss64, g64, g32, what)
        feats = eng.model.log2feats(short_batch[0]).cpu().numpy()
        assert_tensor_close(feats, features64(w_short, short_batch[0], H), what=f"{what}: log2feats")
        return loss

    first = run_short("length 37 of maxlen 100")
    long64, long_g64, long_g32 = se.reference(w, long_batch, H, se.L2, None, 0.0)
    loss, grads = eng.backward_only(full_batch(long_batch))
    check_loss_and_grads(loss, grads, long64, long_g64, long_g32, "length 100 of maxlen 100")
    again = run_short("length 37 after length 100")
    assert_scalar_close(again, first, what="length 37 again")


def check_adam_step(eng, w0, g32, loss, loss64, what):
    """As ``test_step_matches_reference``: the stepped weights against ``sn.opt_step`` on the restatement's fp32
    gradient, inside ``sas_band``."""
    assert_scalar_close(loss, loss64, what=f"{what}: loss")
    st0 = sn.new_opt_state(w0, "adam")
    band = sas_band(w0, st0, g32, "adam", LR)
    w_ref = {k: v.copy() for k, v in w0.items()}
    sn.opt_step(w_ref, g32, sn.new_opt_state(w0, "adam"), "adam", LR)
    w1 = get_weights(eng)
    for k in w_ref:
        assert_step_close(w0[k], w1[k], w_ref[k], band[k], what=f"{what}: weights {k}")
    assert float(np.abs(w1["item_emb.weight"][0]).max()) == 0.0
    assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"


def test_adam_step_under_dropout_with_explicit_masks(hip_device):
    """Part 4.  One full step at (64, 2, 65, 3, 2, 0.25), Adam, l2_emb 0.05, from a fresh optimizer state."""
    D, H, T, B, nb, p = STEP_SHAPE
    w, batch, keep, loss64, g64, g32 = dropout_case(STEP_SHAPE)
    eng = make_engine(w, se.ITEMS, D, H, T, nb, p=p, B=B, l2=se.L2, optimizer="adam", lr=LR)
    eng.load_optimizer_state(0)
    loss = eng.train_single_batch(full_batch(batch), keep_masks=keep)
    check_adam_step(eng, w, g32, loss, loss64, "explicit masks")


def test_device_drawn_masks_give_the_restatement_gradient(hip_device):
    """Part 4, ``dropout_rng = "device"``: the masks the engine drew are read back and handed to the restatement; the
    loss and gradients of ``backward_only`` and one Adam step are held as with explicit masks."""
    D, H, T, B, nb, p = STEP_SHAPE
    w, batch = se.edge_weights_and_batch(D, H, T, B, nb)
    eng = make_engine(w, se.ITEMS, D, H, T, nb, p=p, B=B, l2=se.L2, optimizer="adam", lr=LR, dropout_rng="device",
                      dropout_seed=5)
    shapes = se.mask_shapes(D, H, T, B, nb)

    def drawn():
        masks = [k.cpu().numpy().reshape(s) for k, s in zip(eng.last_keep_masks, shapes)]
        assert len(masks) == len(shapes)
        for k in masks:
            assert k.dtype == np.uint8 and 0 < k.mean() < 1
        return masks

    loss, grads = eng.backward_only(full_batch(batch))
    keep = drawn()
    loss64, g64, g32 = se.reference(w, batch, H, se.L2, keep, p)
    check_loss_and_grads(loss, grads, loss64, g64, g32, "device masks")
    eng.load_optimizer_state(0)
    loss = eng.train_single_batch(full_batch(batch))
    keep2 = drawn()
    assert not np.array_equal(keep2[1], keep[1]), "two steps drew the same attention mask"
    loss64, _, g32 = se.reference(w, batch, H, se.L2, keep2, p)
    check_adam_step(eng, w, g32, loss, loss64, "device masks")


def test_predict_at_a_ragged_length(hip_device):
    """Part 5.  3 sequences x 20 candidates at (64, 2, 65) against the fp64 forward's last-position features."""
    D, H, T, B, nb, _ = STEP_SHAPE
    w, batch = se.edge_weights_and_batch(D, H, T, B, nb)
    eng = make_engine(w, se.ITEMS, D, H, T, nb, B=B)
    ids = np.random.default_rng(3).permutation(se.ITEMS)[:20] + 1
    with float64_oracle(sn):
        s64 = sn.predict(to64(w), batch[0], ids, H)
    got = eng.model.predict(np.arange(B), batch[0], ids)
    assert tuple(got.shape) == (B, 20)
    assert_tensor_close(got.cpu().numpy(), s64, what="predict")
