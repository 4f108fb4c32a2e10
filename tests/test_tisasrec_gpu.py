"""GPU parity tests of TiSASRec (csrc/tisasrec.hip): forward + loss + backward, the full step and chained steps vs
golden vectors from the real reference's TiSASRecEngine (tests/golden/tisasrec_*.npz); shapes that cross every tile edge
of the attention kernels, with and without dropout, and the time-matrix patterns, against the fp64 restatement; run-to-run
reproducibility; the dropout modes; ``time_matrix=None``; predict / recommend_next; the epoch's contract with the
sampler; the bounds checks; the checkpoint round trip.

``attention_layers.{b}.K_w.bias`` is held through ``tisasrec_edges.key_bias_floor`` (its exact gradient is zero; see
tests/test_oracle_golden_tisasrec.py)."""
import contextlib
import ctypes
import functools
import io

import numpy as np
import pytest
import torch

import tisasrec_edges as te
import tisasrec_numpy as tn
import topk_reference as tk
from helpers import REL, assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_sgd_exact
from helpers import assert_step_close, assert_tensor_close, float64_oracle, load_golden, oracle_trajectory, to64
from test_oracle_golden_tisasrec import CASES, exact_grads, hyper, meta, model_config, tis_band, tis_batch
from test_oracle_golden_tisasrec import tis_keep, tis_opt_state, tis_params, unused_rows

pytestmark = pytest.mark.gpu

TIME_TABLES = ("time_matrix_K_emb.weight", "time_matrix_V_emb.weight")


def make_engine(w, I, D, H, T, nb, span, p=0.0, B=8, l2=0.0, optimizer="adam", lr=1e-3, **extra):
    import beta_recsys_amd as hp

    cfg = model_config(I, D, H, T, nb, span, p, B, l2, optimizer, lr, device="cuda:0")
    cfg["model"].update(extra)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.TiSASRecEngine(cfg)
    if w is not None:
        load_weights(eng, w)
    return eng


def golden_engine(case, g, **extra):
    I, T, D, H, nb, B, _, _, span = meta(g)
    opt, lr, l2, p = hyper(g)
    return make_engine(tis_params(case, g, 0), I, D, H, T, nb, span, p, B, l2, opt, lr, **extra)


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def load_opt_state(eng, st, opt):
    eng.load_optimizer_state(st["step"], st.get("exp_avg"), st.get("exp_avg_sq", st.get("square_avg")))


def np_grads(grads):
    return {k: v.cpu().numpy() for k, v in grads.items()}


def full_batch(batch, time_seq=None):
    """The engine's ``(u, seq, time_seq, time_matrix, pos, neg)`` from the restatement's ``(seq, tm, pos, neg)``."""
    seq, tm, pos, neg = batch
    return np.arange(len(seq)), seq, time_seq, tm, pos, neg


def check_loss_and_grads(loss, grads, loss64, g64, g_other, floor, what, tm=None, span=None):
    grads = np_grads(grads)
    print(f"{what}: loss {loss!r} vs exact {loss64!r}")
    for k in g64:
        print(f"  grad {k}: err vs exact {np.abs(grads[k].reshape(g64[k].shape) - g64[k]).max():.3e}, the other fp32's "
              f"{np.abs(g_other[k] - g64[k]).max():.3e}, scale {max(np.abs(g64[k]).max(), floor(k)):.3e}")
    assert_scalar_close(loss, loss64, what=f"{what}: loss")
    assert_grads_as_accurate(grads, g_other, g64, what=f"{what}: grad", floor_fn=floor)
    assert float(np.abs(grads["item_emb.weight"][0]).max()) == 0.0, "a gradient reached the padding row"
    if tm is not None:
        rows = unused_rows(tm, span)
        for k in TIME_TABLES:
            if rows:
                assert float(np.abs(grads[k][rows]).max()) == 0.0, f"{k}: a gradient reached a row no pair selects"
    return grads


@pytest.mark.parametrize("case", CASES)
def test_step_matches_reference(hip_device, case):
    """Each step from the reference's own weights and optimizer state: the loss, every gradient (as accurate as the
    reference against the fp64 evaluation), the padding row's and the never-indexed time-table rows' gradients exactly
    zero, the stepped weights, the gradient buffer cleared."""
    g = load_golden(case)
    opt, lr, l2, p = hyper(g)
    H, span = meta(g)[3], meta(g)[8]
    eng = golden_engine(case, g)
    for s in range(meta(g)[6]):
        batch, keep = tis_batch(g, s), tis_keep(g, s)
        w0, st0 = tis_params(case, g, s), tis_opt_state(case, g, s)
        load_weights(eng, w0)
        load_opt_state(eng, st0, opt)
        loss, grads = eng.backward_only(full_batch(batch), keep_masks=keep)
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        g_ref = tis_params(case, g, s + 1, "g")
        loss64, g64, floor = exact_grads(w0, batch, H, l2, keep, p)
        assert unused_rows(batch[1], span)
        check_loss_and_grads(loss, grads, loss64, g64, g_ref, floor, f"{case} step {s}", batch[1], span)
        assert float(eng._g_flat.abs().max()) == 0.0
        # the full step
        load_opt_state(eng, st0, opt)
        loss = eng.train_single_batch(full_batch(batch), keep_masks=keep)
        assert_scalar_close(loss, g["losses"][s], what=f"loss (step) {s}")
        band = tis_band(w0, st0, g_ref, opt, lr, floor)
        w1, w_ref = get_weights(eng), tis_params(case, g, s + 1)
        for k in w_ref:
            assert_step_close(w0[k], w1[k], w_ref[k], band[k], what=f"weights {k} step {s}")
        assert float(np.abs(w1["item_emb.weight"][0]).max()) == 0.0
        assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"


@pytest.mark.parametrize("case", CASES)
def test_trajectory_matches_reference(hip_device, case):
    """Three steps chained from w0.  SGD: every element within 1e-5 of the trajectory's update; Adam / RMSprop: every
    element inside the oracle's perturbed-gradient envelope around the reference's end point, zero outliers.  K_w.bias's
    gradient is rounding noise around an exact zero, which Adam / RMSprop turn into steps of size lr in a direction no
    two implementations share: WHICH of its elements drift is chance, so that tensor's envelope is pooled over its
    elements (``assert_on_trajectory(pool=True)``, made for exactly this)."""
    g = load_golden(case)
    opt, lr, l2, p = hyper(g)
    H, steps = meta(g)[3], meta(g)[6]
    eng = golden_engine(case, g)
    w0 = tis_params(case, g, 0)
    batches = [tis_batch(g, s) + (tis_keep(g, s), s) for s in range(steps)]
    for s, b in enumerate(batches):
        loss = eng.train_single_batch(full_batch(b[:4]), keep_masks=b[4])
        print(f"{case} chained step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        if opt == "sgd" or s == 0:
            assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
    ref_end = tis_params(case, g, steps)
    got = get_weights(eng)
    if opt == "sgd":
        floors = [exact_grads(tis_params(case, g, s), b[:4], H, l2, b[4], p)[2] for s, b in enumerate(batches)]
        bias_keys = [k for k in ref_end if k.endswith("K_w.bias")]
        rest = {k: v for k, v in ref_end.items() if k not in bias_keys}
        assert_sgd_exact(got, rest, w0, "final weights")
        for k in bias_keys:        # three steps of lr x (a gradient within REL of its terms' scale)
            tol = steps * lr * REL * max(f(k) for f in floors) + 4 * np.finfo(np.float32).eps * np.abs(ref_end[k]).max()
            assert float(np.abs(got[k] - ref_end[k]).max()) <= tol, k
        return
    floors = [exact_grads(tis_params(case, g, s), b[:4], H, l2, b[4], p)[2] for s, b in enumerate(batches)]
    _, env, upd = oracle_trajectory(
        w0, batches, lambda w, b: tn.tisasrec_grads(w, b[:4], H, l2, b[4], p)[1],
        lambda w, gr, st: tn.opt_step(w, gr, st, opt, lr), lambda w: tn.new_opt_state(w, opt),
        floor_fn=lambda k, b: floors[b[5]](k))
    bias_keys = [k for k in ref_end if k.endswith("K_w.bias")]
    assert_on_trajectory(got, {k: v for k, v in ref_end.items() if k not in bias_keys}, env, upd, f"{case} trajectory")
    assert_on_trajectory(got, {k: ref_end[k] for k in bias_keys}, env, upd, f"{case} trajectory", pool=True)


@functools.lru_cache(maxsize=None)
def edge_case(shape, dropout):
    """``(w, batch, keep, p, loss64, g64, g32, floor)`` of one of EDGE_SHAPES, computed once and never written to."""
    D, H, T, B, nb, span, p = shape
    w, batch, keep = te.edge_fixture(*shape)
    if not dropout:
        keep, p = None, 0.0
    return (w, batch, keep, p) + te.reference(w, batch, H, te.L2, keep, p)


def features64(w, seq, tm, H):
    with float64_oracle(tn):
        return tn.tisasrec_forward(to64(w), seq, tm, H)[0]


@pytest.mark.parametrize("dropout", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("D,H,T,B,nb,span,p", te.EDGE_SHAPES)
def test_tile_edges_against_the_restatement(hip_device, D, H, T, B, nb, span, p, dropout):
    """Every seam of the attention kernels (tisasrec_edges.EDGE_SHAPES says which shape crosses which), head widths 16,
    32 and 64, D = 48 and 96, time_span 1, 16 and 256, one sequence fully real, one left-padded, one all padding, two
    blocks sharing the position and time masks: loss and every gradient against the restatement in fp64, as accurate as
    its fp32 self; without dropout the eval-mode features too (padded query rows included: the restatement attends
    uniformly there, the kernel skips them, and nothing downstream can tell)."""
    w, batch, keep, p_used, loss64, g64, g32, floor = edge_case((D, H, T, B, nb, span, p), dropout)
    eng = make_engine(w, te.ITEMS, D, H, T, nb, span, p=p_used, B=B, l2=te.L2)
    assert [tuple(s) for s in eng._mask_shapes(B, T)] == te.mask_shapes(D, H, T, B, nb)
    loss, grads = eng.backward_only(full_batch(batch), keep_masks=keep)
    check_loss_and_grads(loss, grads, loss64, g64, g32, floor, f"D {D} H {H} T {T} B {B} blocks {nb} span {span} "
                         f"p {p_used}", batch[1], span)
    if not dropout:
        assert (batch[0] == 0).any()
        feats = eng.model.seq2feats(None, batch[0], batch[1]).cpu().numpy()
        assert_tensor_close(feats, features64(w, batch[0], batch[1], H), what="seq2feats")


def test_padded_query_rows_reach_nothing(hip_device):
    """The restatement attends uniformly over all T keys at a padded query row (its output there is not zero); the
    kernel skips such rows.  The features at EVERY position, padded ones included, and every gradient are the
    restatement's all the same: the block's output is multiplied by the timeline mask."""
    case = "tisasrec_adam"
    g = load_golden(case)
    I, T, D, H, nb, B, _, _, span = meta(g)
    _, _, l2, p = hyper(g)
    w, batch = tis_params(case, g, 0), tis_batch(g, 0)
    pad = batch[0] == 0
    assert pad.any() and pad.all(1).sum() == 0 and (pad.sum(1) >= T // 2).any()
    with float64_oracle(tn):
        f64, cache = tn.tisasrec_forward(to64(w), batch[0], batch[1], H)
    for c in cache["blocks"]:
        assert float(np.abs(c["o"][pad]).max()) > 0 and np.allclose(c["prob"][:, 0][pad], 1.0 / T)
    eng = golden_engine(case, g)
    feats = eng.model.seq2feats(None, batch[0], batch[1]).cpu().numpy()
    assert_tensor_close(feats, f64, what="features at every position")
    assert_tensor_close(feats[pad], f64[pad], what="features at the padded positions")
    loss64, g64, floor = exact_grads(w, batch, H, l2, None, p)
    _, g32 = tn.tisasrec_grads(w, batch, H, l2)
    loss, grads = eng.backward_only(full_batch(batch))
    check_loss_and_grads(loss, grads, loss64, g64, g32, floor, "padded query rows", batch[1], span)


def pattern_matrix(name, B, T, span):
    if name == "zeros":                       # what the reference's seq_predict_time passes: one row takes everything
        return np.zeros((B, T, T), dtype=np.int32)
    if name == "all_span":
        return np.full((B, T, T), span, dtype=np.int32)
    rng = np.random.default_rng(17)           # asymmetric, from no time sequence; row 3 of the tables never selected
    tm = rng.integers(0, span + 1, (B, T, T)).astype(np.int32)
    tm[tm == 3] = 4
    assert not np.array_equal(tm, tm.transpose(0, 2, 1)) and (np.diagonal(tm, axis1=1, axis2=2) != 0).any()
    return tm


@pytest.mark.parametrize("dropout", [False, True], ids=["plain", "dropout"])
@pytest.mark.parametrize("pattern", ["zeros", "all_span", "asymmetric"])
def test_time_matrix_patterns(hip_device, pattern, dropout):
    """T = 65 (two key chunks): every pair in ONE table row (the hottest possible bin, rows 1 .. span untouched), every
    pair in the last row, and an arbitrary matrix -- the ABI takes any."""
    D, H, T, B, nb, span = te.PATTERN_SHAPE
    p = 0.25 if dropout else 0.0
    w, (seq, _, pos, neg), keep = te.edge_fixture(D, H, T, B, nb, span, 0.25)
    batch = (seq, pattern_matrix(pattern, B, T, span), pos, neg)
    keep = keep if dropout else None
    loss64, g64, g32, floor = te.reference(w, batch, H, te.L2, keep, p)
    eng = make_engine(w, te.ITEMS, D, H, T, nb, span, p=p, B=B, l2=te.L2)
    loss, grads = eng.backward_only(full_batch(batch), keep_masks=keep)
    grads = check_loss_and_grads(loss, grads, loss64, g64, g32, floor, f"{pattern} p {p}", batch[1], span)
    assert len(unused_rows(batch[1], span)) == {"zeros": span, "all_span": span, "asymmetric": 1}[pattern]
    for k in TIME_TABLES:
        assert float(np.abs(grads[k]).max()) > 0


def test_time_matrix_entries_out_of_range_raise_and_corrupt_nothing(hip_device):
    case = "tisasrec_adam"
    g = load_golden(case)
    span = meta(g)[8]
    eng = golden_engine(case, g)
    good = tis_batch(g, 0)
    before = eng.model.flat.clone()
    for where, value in (((0, 0, 0), span + 1), ((1, 5, 2), -1), ((2, 11, 11), 2 ** 31 - 1), ((4, 3, 9), -2 ** 31)):
        bad = [a.copy() for a in good]
        bad[1][where] = value
        with pytest.raises(IndexError):
            eng.backward_only(full_batch(bad))
        assert torch.equal(eng.model.flat, before), "the weights moved"
        assert float(eng._g_flat.abs().max()) == 0.0, "a partial gradient was kept"
        with pytest.raises(IndexError):
            eng.model.seq2feats(None, bad[0], bad[1])
    for slot, value in ((0, meta(g)[0] + 1), (2, meta(g)[0] + 1), (3, -1)):
        bad = [a.copy() for a in good]
        bad[slot][0, -1] = value
        with pytest.raises(IndexError):
            eng.backward_only(full_batch(bad))
        assert float(eng._g_flat.abs().max()) == 0.0
    bad = [a.copy() for a in good]
    bad[1][3, 7, 2] = span + 9
    with pytest.raises(IndexError):          # as for an item id: the step's error surfaces at its one host sync
        eng.train_single_batch(full_batch(bad))
    assert float(eng._g_flat.abs().max()) == 0.0
    with pytest.raises(ValueError):
        eng.train_single_batch(good)                                     # four entries: not a TiSASRec batch
    with pytest.raises(ValueError):
        eng.train_single_batch(full_batch((good[0], good[1][:, :-1], good[2], good[3])))
    with pytest.raises(ValueError):
        eng.train_single_batch((None, good[0], None, None, good[2], good[3]))       # neither matrix nor time_seq
    load_weights(eng, tis_params(case, g, 0))
    eng.load_optimizer_state(0)
    loss = eng.train_single_batch(full_batch(good))
    assert_scalar_close(loss, g["losses"][0], what="loss after the errors")


def test_gradients_are_reproducible(hip_device):
    """Two ``backward_only`` calls on the same inputs under dropout at (64, 2, 65, 3, 2): three query tiles, B * H = 6.
    Every gradient but item_emb's (row atomics in the loss stage, as SASRec's) is bit-identical."""
    shape = te.EDGE_SHAPES[0]
    D, H, T, B, nb, span, p = shape
    assert B * H >= 6 and T > 32
    w, batch, keep = te.edge_fixture(*shape)
    eng = make_engine(w, te.ITEMS, D, H, T, nb, span, p=p, B=B, l2=te.L2)
    _, first = eng.backward_only(full_batch(batch), keep_masks=keep)
    other = make_engine(w, te.ITEMS, D, H, T, nb, span, p=p, B=B, l2=te.L2)      # its own workspace, too
    for e in (eng, other, eng):
        _, again = e.backward_only(full_batch(batch), keep_masks=keep)
        for k in first:
            if k != "item_emb.weight":
                assert torch.equal(first[k], again[k]), f"{k} differs between two runs"


def test_dropout_modes(hip_device):
    """``"torch_cpu"`` draws the reference's own masks from the fixture's torch seed; explicit masks give the reference's
    losses; ``"device"`` differs between steps and is a function of (seed, step); a wrong count or size raises."""
    case = "tisasrec_rmsprop_drop"
    g = load_golden(case)
    opt, lr, l2, p = hyper(g)
    nb, steps, seed = meta(g)[4], meta(g)[6], meta(g)[7]
    torch.manual_seed(seed)
    eng = golden_engine(case, g)                  # the constructor draws what the reference's constructor drew
    for s in range(steps):
        load_weights(eng, tis_params(case, g, s))
        load_opt_state(eng, tis_opt_state(case, g, s), opt)
        loss = eng.train_single_batch(full_batch(tis_batch(g, s)))
        drawn = [k.cpu().numpy() for k in eng.last_keep_masks]
        assert len(drawn) == 5 + 3 * nb
        assert_scalar_close(loss, g["losses"][s], what=f"torch_cpu loss step {s}")
        for i, (a, b) in enumerate(zip(drawn, tis_keep(g, s))):
            assert np.array_equal(a, b), f"step {s} mask {i} is not the reference's"
    other = golden_engine(case, g)
    loss = other.train_single_batch(full_batch(tis_batch(g, 0)), keep_masks=tis_keep(g, 0))
    assert_scalar_close(loss, g["losses"][0], what="explicit masks")
    with pytest.raises(ValueError):
        other.train_single_batch(full_batch(tis_batch(g, 0)), keep_masks=tis_keep(g, 0)[:-1])
    wrong = list(tis_keep(g, 0))
    wrong[3] = wrong[3][:-1]
    with pytest.raises(ValueError):
        other.train_single_batch(full_batch(tis_batch(g, 0)), keep_masks=wrong)
    runs = []
    for _ in range(2):
        dev = golden_engine(case, g, dropout_rng="device", dropout_seed=5)
        masks = []
        for s in range(2):
            assert np.isfinite(dev.train_single_batch(full_batch(tis_batch(g, s))))
            masks.append([k.clone() for k in dev.last_keep_masks])
        runs.append(masks)
    for i, (a, b) in enumerate(zip(runs[0][0], runs[0][1])):
        assert a.dtype == torch.uint8 and int(a.max()) == 1 and not torch.equal(a, b), f"mask {i}: two steps, one draw"
    for s in range(2):
        for a, b in zip(runs[0][s], runs[1][s]):
            assert torch.equal(a, b), "the device masks are a function of (seed, step)"
    for i in range(len(runs[0][0])):
        for j in range(i):
            if runs[0][0][i].numel() == runs[0][0][j].numel():
                assert not torch.equal(runs[0][0][i], runs[0][0][j]), f"masks {i} and {j} of one step are the same draw"
    different = golden_engine(case, g, dropout_rng="device", dropout_seed=6)
    different.train_single_batch(full_batch(tis_batch(g, 0)))
    assert not torch.equal(different.last_keep_masks[3], runs[0][0][3])
    dev.model.eval()
    dev.backward_only(full_batch(tis_batch(g, 0)))
    assert dev.last_keep_masks is None


def test_time_relation_on_the_device_and_a_batch_without_matrix(hip_device):
    """``hiprec_time_relation`` is numpy's ``min(|t_i - t_j|, span)`` bit for bit, the clamp included; a batch with
    ``time_matrix=None`` gives bit-identical results to one that carries ``data.time_relation(time_seq)``."""
    from beta_recsys_amd import _lib
    from beta_recsys_amd.data import time_relation

    rng = np.random.default_rng(9)
    lib = _lib.load()
    for B, T, span in ((3, 65, 16), (2, 7, 1), (1, 256, 256)):
        ts = rng.integers(0, 4 * span + 3, (B, T))
        ts[0, :T // 2] = 0
        ts[-1, -1] = 2 ** 40                                         # a 64-bit stamp: the difference clamps, no wrap
        dev_ts = torch.from_numpy(ts).cuda()
        out = torch.empty((B, T, T), dtype=torch.int32, device="cuda")
        _lib.check(lib.hiprec_time_relation(_lib.ptr(dev_ts), B, T, span, _lib.ptr(out), _lib.stream_ptr(out.device)))
        want = time_relation(ts, span)
        assert want.max() == span and np.array_equal(out.cpu().numpy(), want)
    case = "tisasrec_rmsprop_drop"
    g = load_golden(case)
    span = meta(g)[8]
    eng = golden_engine(case, g)
    batch, keep, ts = tis_batch(g, 0), tis_keep(g, 0), g["time_seq"][0]
    assert np.array_equal(time_relation(ts, span), batch[1])
    loss_a, grads_a = eng.backward_only(full_batch(batch, ts), keep_masks=keep)
    loss_b, grads_b = eng.backward_only(full_batch((batch[0], None, batch[2], batch[3]), ts), keep_masks=keep)
    assert loss_a == loss_b
    for k in grads_a:
        if k != "item_emb.weight":
            assert torch.equal(grads_a[k], grads_b[k]), k
    eng.model.eval()
    a = eng.model.seq2feats(None, batch[0], batch[1])
    b = eng.model.seq2feats(None, batch[0], None, time_seq=ts)
    assert torch.equal(a, b)
    assert torch.equal(eng.model.predict(None, batch[0], batch[1], [1, 2, 3]),
                       eng.model.predict(None, batch[0], None, [1, 2, 3], time_seq=ts))
    assert torch.equal(eng.recommend_next(batch[0], batch[1], 4)[0], eng.recommend_next(batch[0], None, 4, time_seq=ts)[0])


def test_predict_and_recommend_next(hip_device):
    case = "tisasrec_adam"
    g = load_golden(case)
    I, T, D, H, nb, B, _, _, span = meta(g)
    w = tis_params(case, g, 0)
    eng = golden_engine(case, g)
    seqs, tm = tis_batch(g, 0)[:2]
    ids = np.arange(1, I + 1)
    with float64_oracle(tn):
        s64 = tn.predict(to64(w), seqs, tm, ids, H)
        f64 = tn.tisasrec_forward(to64(w), seqs, tm, H)[0]
    feats = eng.model.seq2feats(np.arange(B), seqs, tm)
    assert_tensor_close(feats.cpu().numpy(), f64, what="seq2feats")
    got = eng.model.predict(np.arange(B), seqs, tm, ids)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, I)
    assert_tensor_close(got.cpu().numpy(), s64, what="predict")
    pl, nl = eng.model(None, seqs, tm, tis_batch(g, 0)[2], tis_batch(g, 0)[3])
    E = w["item_emb.weight"].astype(np.float64)
    assert_tensor_close(pl.cpu().numpy(), (f64 * E[tis_batch(g, 0)[2]]).sum(-1), what="forward: positive logits")
    assert_tensor_close(nl.cpu().numpy(), (f64 * E[tis_batch(g, 0)[3]]).sum(-1), what="forward: negative logits")
    sub = np.array([7, 0, 3, 7])
    with float64_oracle(tn):
        s_sub = tn.predict(to64(w), seqs, tm, sub, H)
    assert_tensor_close(eng.model.predict(None, seqs, tm, sub).cpu().numpy(), s_sub, what="predict on a list with id 0")
    with pytest.raises(IndexError):
        eng.model.predict(None, seqs, tm, [1, I + 1])
    with pytest.raises(ValueError):
        eng.model.predict(None, seqs, tm, [[1, 2]])
    k = 6
    items, scores = eng.recommend_next(seqs, tm, k)
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    assert items.shape == (B, k) and (items >= 1).all() and (items <= I).all()
    tk.check_against_float64(items - 1, scores, s64, None, "recommend_next")
    rows = np.repeat(np.arange(B), T)
    items_s, scores_s = eng.recommend_next(seqs, tm, k, seen=(rows, seqs.reshape(-1)))
    items_s = items_s.cpu().numpy()
    seen = [np.unique(seqs[b][seqs[b] != 0]) - 1 for b in range(B)]
    tk.check_against_float64(items_s - 1, scores_s.cpu().numpy(), s64, seen, "recommend_next with seen")
    for b in range(B):
        assert not set(items_s[b].tolist()) & set(seqs[b].tolist())
    many, _ = eng.recommend_next(seqs[:1], tm[:1], 64)
    many = many.cpu().numpy()[0]
    assert sorted(many[:I].tolist()) == list(range(1, I + 1)) and (many[I:] == -1).all()


class StubSampler:
    def __init__(self, g, with_matrix=True):
        self.g, self.calls, self.with_matrix = g, 0, with_matrix

    def next_batch(self):
        s = self.calls % meta(self.g)[6]
        seq, tm, pos, neg = tis_batch(self.g, s)
        self.calls += 1
        rows = lambda a: tuple(map(tuple, a))   # noqa: E731
        return (tuple(range(len(seq))), rows(seq), rows(self.g["time_seq"][s]), tm if self.with_matrix else None,
                rows(pos), rows(neg))


def test_train_an_epoch_asks_the_sampler_as_the_reference_does(hip_device):
    case = "tisasrec_sgd_h1"
    g = load_golden(case)
    B = meta(g)[5]
    for with_matrix in (True, False):
        eng = golden_engine(case, g)
        eng.num_batch = 3                                     # the fixture's three batches make one epoch
        sampler = StubSampler(g, with_matrix)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            eng.train_an_epoch(sampler, 4)
        assert sampler.calls == 3
        tag, total, epoch_id = eng.writer.scalars[-1]
        assert (tag, epoch_id) == ("model/loss", 4)
        assert_scalar_close(total, float(g["losses"].sum()), 2 * REL, "epoch loss sum")
        assert out.getvalue().strip() == "[Training Epoch 4], Loss {}".format(total)
        got, ref_end = get_weights(eng), tis_params(case, g, 3)
        rest = {k: v for k, v in ref_end.items() if not k.endswith("K_w.bias")}
        assert_sgd_exact(got, rest, tis_params(case, g, 0), "after the epoch")
    full = golden_engine(case, g)
    assert full.num_batch == 64 // B                          # n_users // batch_size, as the reference computes it
    sampler = StubSampler(g)
    with contextlib.redirect_stdout(io.StringIO()):
        full.train_an_epoch(sampler, 0)
    assert sampler.calls == 64 // B


def test_epoch_with_the_time_sequence_sampler(hip_device):
    """``data.TimeSequenceSampler`` feeds ``train_an_epoch`` directly; the loss falls over a few epochs."""
    from beta_recsys_amd.data import TimeSequenceSampler

    rng = np.random.default_rng(2)
    I, D, H, T, nb, span, B = 30, 32, 2, 10, 1, 8, 16
    user_train = {u: [[int((u + 3 * k) % I) + 1, 1 + 2 * k] for k in range(4 + u % 9)] for u in range(1, 65)}
    eng = make_engine(None, I, D, H, T, nb, span, B=B, lr=5e-3)
    sampler = TimeSequenceSampler(user_train, 64, I, B, T, span, seed=int(rng.integers(100)))
    totals = []
    for epoch in range(4):
        with contextlib.redirect_stdout(io.StringIO()):
            eng.train_an_epoch(sampler, epoch)
        totals.append(eng.writer.scalars[-1][1])
    assert np.isfinite(totals).all() and totals[-1] < totals[0]


def test_checkpoint_round_trip(hip_device, tmp_path):
    """Save, load into a fresh engine (weights and optimizer state): the next step's loss and weights are identical."""
    case = "tisasrec_adam"
    g = load_golden(case)
    eng = golden_engine(case, g)
    eng.train_single_batch(full_batch(tis_batch(g, 0)))
    path = str(tmp_path / "tisasrec.pt")
    eng.save_checkpoint(path, optimizer_state=True)
    sd = torch.load(path)
    assert tuple(sd) == tn.keys(meta(g)[4])
    other = golden_engine(case, g)
    with contextlib.redirect_stdout(io.StringIO()):
        other.resume_checkpoint(path, optimizer_state=True)
    assert torch.equal(other.model.flat, eng.model.flat)
    a = eng.train_single_batch(full_batch(tis_batch(g, 1)))
    b = other.train_single_batch(full_batch(tis_batch(g, 1)))
    assert a == b
    assert_tensor_close(other.model.flat.cpu().numpy(), eng.model.flat.cpu().numpy(), 1e-6, "weights after the step")


def test_workspace_holds_no_gathered_tensor(hip_device):
    """A condition, not a measurement: at the reference's default shape the workspace is below B * T * T * D * 4 bytes,
    and a step at that shape's sequence length runs in it."""
    from beta_recsys_amd import _lib

    B, T, D, H, nb, span = 128, 150, 64, 2, 2, 128
    shape = _lib.TisasrecShape(3416, D, H, T, span, nb, 0)
    need = _lib.load().hiprec_tisasrec_workspace_bytes(ctypes.byref(shape), B, T)
    assert 0 < need < B * T * T * D * 4
    eng = make_engine(None, 3416, D, H, T, nb, span, B=B)
    w, batch, _ = te.synthetic(3416, D, H, T, 8, nb, span, seed=1, all_padding_row=True)
    loss = eng.train_single_batch(full_batch(batch))
    assert np.isfinite(loss)
