"""GPU parity tests of NARM (csrc/narm.hip): forward + loss + backward, the full step and chained steps vs golden vectors
from the real reference's NARMEngine (tests/golden/narm_*.npz), the epoch's StepLR rule on the path; synthetic shapes
that straddle every kernel constant (tests/narm_edges.py) against the fp64 restatement; unsorted lengths; the dropout
modes; predict / recommend / recommend_next; the bounds check; the ValueError cases; the checkpoint round trip."""
import contextlib
import io

import numpy as np
import pytest
import torch

import narm_edges as ne
import narm_numpy as nn_
import topk_reference as tk
from helpers import REL, assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_sgd_exact
from helpers import assert_step_close, assert_tensor_close, float64_oracle, load_golden, oracle_trajectory, to64
from test_oracle_golden_narm import CASES, exact_grads, golden_config, hyper, meta, model_config, narm_band, narm_batch
from test_oracle_golden_narm import narm_keep, narm_opt_state, narm_params, step_lr

pytestmark = pytest.mark.gpu


def engine_for(cfg, w=None):
    import beta_recsys_amd as hp

    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.NARMEngine(cfg)
    if w is not None:
        load_weights(eng, w)
    return eng


def golden_engine(case, g, **extra):
    cfg = golden_config(g, device="cuda:0")
    cfg["model"].update(extra)
    return engine_for(cfg, narm_params(case, g, 0))


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def load_opt_state(eng, st):
    eng.load_optimizer_state(st["step"], st.get("exp_avg"), st.get("exp_avg_sq", st.get("square_avg")))


def np_grads(grads):
    return {k: v.cpu().numpy() for k, v in grads.items()}


def report(grads, g_ref, g64):
    for k in g64:
        print(f"  grad {k}: err vs exact {np.abs(grads[k].reshape(g64[k].shape) - g64[k]).max():.3e}, reference's own "
              f"{np.abs(g_ref[k] - g64[k]).max():.3e}, scale {np.abs(g64[k]).max():.3e}")


@pytest.mark.parametrize("case", CASES)
def test_step_matches_reference(hip_device, case):
    """Each step from the reference's own weights and optimizer state: the loss, every gradient (as accurate as the
    reference against the fp64 evaluation), the padding row's gradient and weight exactly zero, the gradient buffer
    cleared after the sweep, the stepped weights inside the band."""
    g = load_golden(case)
    opt, _, _, _, p = hyper(g)
    eng = golden_engine(case, g)
    for s in range(meta(g)[6]):
        batch, keep = narm_batch(g, s), narm_keep(g, s)
        w0, st0 = narm_params(case, g, s), narm_opt_state(case, g, s)
        load_weights(eng, w0)
        load_opt_state(eng, st0)
        loss, grads = eng.backward_only(batch, keep_masks=keep)
        grads = np_grads(grads)
        print(f"{case} step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        g_ref = narm_params(case, g, s + 1, "g")
        _, g64 = exact_grads(w0, batch, keep, p)
        report(grads, g_ref, g64)
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}")
        assert float(np.abs(grads["emb.weight"][0]).max()) == 0.0, "a gradient reached the padding row"
        assert float(eng._g_flat.abs().max()) == 0.0
        # the full step, at the epoch's learning rate
        load_opt_state(eng, st0)
        eng.optimizer.lr = step_lr(g, s)
        loss = eng.train_single_batch(batch, keep_masks=keep)
        assert_scalar_close(loss, g["losses"][s], what=f"loss (step) {s}")
        band = narm_band(w0, st0, g_ref, opt, step_lr(g, s))
        w1, w_ref = get_weights(eng), narm_params(case, g, s + 1)
        for k in w_ref:
            assert_step_close(w0[k], w1[k], w_ref[k], band[k], what=f"weights {k} step {s}")
        assert float(np.abs(w1["emb.weight"][0]).max()) == 0.0
        assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"


@pytest.mark.parametrize("case", CASES)
def test_trajectory_matches_reference(hip_device, case):
    """Three steps chained from w0, each one epoch of one batch through ``train_an_epoch`` (the StepLR rule is on the
    path: narm_adam's third epoch runs at lr / 10).  SGD: every element within 1e-5 of the trajectory's update; Adam /
    RMSprop: every element inside the oracle's perturbed-gradient envelope around the reference's end point."""
    g = load_golden(case)
    opt, _, _, _, p = hyper(g)
    steps = meta(g)[6]
    eng = golden_engine(case, g)
    w0 = narm_params(case, g, 0)
    batches = [narm_batch(g, s) + (narm_keep(g, s), step_lr(g, s)) for s in range(steps)]
    for s, b in enumerate(batches):
        if b[3] is None:
            with contextlib.redirect_stdout(io.StringIO()):
                loss = eng.train_an_epoch([b[:3]], s)
            assert eng.writer.scalars[-1] == ("model/loss", loss, s)
        else:                                   # explicit masks do not travel through a loader
            eng.optimizer.lr = eng.epoch_lr(s)
            loss = eng.train_single_batch(b[:3], keep_masks=b[3])
        assert eng.optimizer.lr == pytest.approx(b[4], rel=1e-12)
        print(f"{case} chained step {s}: loss {loss!r} vs {float(g['losses'][s])!r}, lr {eng.optimizer.lr:g}")
        if opt == "sgd" or s == 0:
            assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
    ref_end = narm_params(case, g, steps)
    if opt == "sgd":
        assert_sgd_exact(get_weights(eng), ref_end, w0, "final weights")
        return
    _, env, upd = oracle_trajectory(
        w0, batches, lambda w, b: nn_.narm_grads(w, b[:3], b[3], p)[1],
        lambda w, gr, st: nn_.opt_step(w, gr, st, opt, batches[st["step"]][4]), lambda w: nn_.new_opt_state(w, opt))
    assert_on_trajectory(get_weights(eng), ref_end, env, upd, f"{case} trajectory")


@pytest.mark.parametrize("shape", ne.SHAPES, ids=ne.shape_id)
def test_shapes_against_the_restatement(hip_device, shape):
    """Loss, gradients and eval-mode scores at the shapes of narm_edges.py against the restatement in fp64, as accurate
    as its fp32 self; lengths in no particular order."""
    I, D, H, L, T, B, p = shape
    w, batch, keep = ne.synthetic(shape)
    eng = engine_for(model_config(I, D, H, L, B, p, device="cuda:0"), w)
    _, g32 = nn_.narm_grads(w, batch, keep, p)
    loss64, g64 = exact_grads(w, batch, keep, p)
    loss, grads = eng.backward_only(batch, keep_masks=keep)
    grads = np_grads(grads)
    print(f"{ne.shape_id(shape)}: loss {loss!r} vs exact {loss64!r}")
    report(grads, g32, g64)
    assert_scalar_close(loss, loss64, what="loss")
    assert_grads_as_accurate(grads, g32, g64, what="grad", floor_fn=ne.floor_fn(shape, w, batch, keep))
    assert float(np.abs(grads["emb.weight"][0]).max()) == 0.0
    eng.model.eval()
    scores = eng.model.forward(batch[0], batch[2]).cpu().numpy()
    with float64_oracle(nn_):
        s64 = nn_.scores(to64(w), batch[0], batch[2])
    assert scores.shape == (B, I) and float(np.abs(scores[:, 0]).max()) == 0.0, "item 0 scores exactly 0"
    assert_tensor_close(scores, s64, what="forward")


def test_unsorted_lengths_give_the_sorted_result_row_for_row(hip_device):
    case = "narm_sgd_l2"
    g = load_golden(case)
    eng = golden_engine(case, g)
    seq, target, lens = narm_batch(g, 0)
    perm = np.array([3, 0, 5, 1, 4, 2])
    loss_a, g_a = eng.backward_only((seq, target, lens))
    loss_b, g_b = eng.backward_only((seq[:, perm], target[perm], lens[perm]))
    assert_scalar_close(loss_b, loss_a, what="loss")
    for k in g_a:
        assert_tensor_close(g_b[k].cpu().numpy(), g_a[k].cpu().numpy(), what=k)
    eng.model.eval()
    a = eng.model.forward(seq, lens).cpu().numpy()
    b = eng.model.forward(seq[:, perm], lens[perm]).cpu().numpy()
    assert_tensor_close(b, a[perm], 1e-6, "a session's scores must not depend on its place in the batch")


def test_torch_cpu_dropout_reproduces_the_reference_masks(hip_device):
    """narm_rmsprop_drop: the default ``dropout_rng = "torch_cpu"`` draws the reference's two masks from the fixture's
    torch seed; explicit masks give the same losses; a wrong number of masks is a ValueError."""
    case = "narm_rmsprop_drop"
    g = load_golden(case)
    steps, seed = meta(g)[6], meta(g)[7]
    torch.manual_seed(seed)
    eng = golden_engine(case, g)                  # the constructor draws what the reference's constructor drew
    for s in range(steps):
        load_weights(eng, narm_params(case, g, s))
        load_opt_state(eng, narm_opt_state(case, g, s))
        loss = eng.train_single_batch(narm_batch(g, s))
        drawn = [k.cpu().numpy() for k in eng.last_keep_masks]
        assert_scalar_close(loss, g["losses"][s], what=f"torch_cpu loss step {s}")
        for i, (a, b) in enumerate(zip(drawn, narm_keep(g, s))):
            assert np.array_equal(a, b), f"step {s} mask {i} is not the reference's"
    other = golden_engine(case, g)
    loss = other.train_single_batch(narm_batch(g, 0), keep_masks=narm_keep(g, 0))
    assert_scalar_close(loss, g["losses"][0], what="explicit masks")
    with pytest.raises(ValueError):
        other.train_single_batch(narm_batch(g, 0), keep_masks=narm_keep(g, 0)[:1])


def test_device_dropout_statistics(hip_device):
    """dropout_rng = "device": each mask's keep rate within 4 sigma of 1 - p, two steps draw different masks, a rate of
    0 draws no mask, eval mode draws none."""
    shape = (60, 32, 64, 1, 20, 64, (0.25, 0.5))
    I, D, H, L, T, B, p = shape
    w, batch, _ = ne.synthetic(shape)
    eng = engine_for(model_config(I, D, H, L, B, p, device="cuda:0", optimizer="adam"), w)
    eng.config["model"].update(dropout_rng="device", dropout_seed=5)
    loss1 = eng.train_single_batch(batch)
    first = [k.clone() for k in eng.last_keep_masks]
    loss2 = eng.train_single_batch(batch)
    second = eng.last_keep_masks
    assert np.isfinite(loss1) and np.isfinite(loss2) and len(first) == 2
    for i, (a, b) in enumerate(zip(first, second)):
        n = a.numel()
        assert n == int(np.prod(eng._mask_shapes(B, T)[i])) and a.dtype == torch.uint8
        sigma = np.sqrt(p[i] * (1 - p[i]) / n)
        for m in (a, b):
            assert abs(float(m.float().mean()) - (1 - p[i])) <= 4 * sigma, f"mask {i}"
        assert not torch.equal(a, b), f"mask {i}: two steps drew the same mask"
    half = engine_for(model_config(I, D, H, L, B, (0.0, 0.5), device="cuda:0"), w)
    half.config["model"].update(dropout_rng="device")
    half.train_single_batch(batch)
    assert half.last_keep_masks[0] is None and half.last_keep_masks[1] is not None
    eng.model.eval()
    load_weights(eng, w)
    loss_eval, _ = eng.backward_only(batch)
    assert eng.last_keep_masks is None
    plain = engine_for(model_config(I, D, H, L, B, device="cuda:0"), w)
    loss_plain, _ = plain.backward_only(batch)
    assert plain.last_keep_masks is None
    assert_scalar_close(loss_eval, loss_plain, what="eval mode")
    bad = engine_for(model_config(I, D, H, L, B, p, device="cuda:0"), w)
    bad.config["model"].update(dropout_rng="nope")
    with pytest.raises(ValueError):
        bad.train_single_batch(batch)


def test_predict_and_recommend(hip_device):
    case = "narm_adam"
    g = load_golden(case)
    I = meta(g)[0]
    w = narm_params(case, g, 0)
    eng = golden_engine(case, g)
    seq, _, lens = narm_batch(g, 0)
    for b in (0, len(lens) - 1):
        profile = seq[:lens[b], b].tolist()
        with float64_oracle(nn_):
            p64 = nn_.predict(to64(w), profile)
        pred = eng.predict(profile)
        assert isinstance(pred, np.ndarray) and pred.shape == (I,) and pred.dtype == np.float32
        assert abs(float(pred.astype(np.float64).sum()) - 1.0) <= 1e-5
        assert_tensor_close(pred, p64, what="predict")
        rec = eng.recommend(profile)
        assert len(rec) == I and all(isinstance(r[0], list) and len(r[0]) == 1 for r in rec)
        items, conf = eng.get_recommendation_list(rec), eng.get_recommendation_confidence_list(rec)
        assert sorted(i[0] for i in items) == list(range(I))
        assert all(a >= b for a, b in zip(conf, conf[1:])), "scores must descend"
        assert conf == [float(pred[i[0]]) for i in items]
    assert not eng.model.training


def test_recommend_next(hip_device):
    """Against tests/topk_reference.py on the fp64 scores: never the padding id, ``seen`` honoured, the caller's order
    restored although the kernel batch is sorted by length; ragged and padded input agree."""
    case = "narm_sgd_l2"
    g = load_golden(case)
    I = meta(g)[0]
    w = narm_params(case, g, 0)
    eng = golden_engine(case, g)
    seq, _, lens = narm_batch(g, 0)
    order = np.array([4, 0, 5, 2, 1, 3])                     # the caller's order: lengths NOT sorted
    profiles = [seq[:lens[b], b].tolist() for b in order]
    with float64_oracle(nn_):
        s64 = nn_.scores(to64(w), seq[:, order], lens[order])[:, 1:]
    k = 6
    items, scores = eng.recommend_next(profiles, k)
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    assert items.shape == (len(order), k) and (items >= 1).all() and (items < I).all()
    tk.check_against_float64(items - 1, scores, s64, None, "recommend_next")
    padded = np.ascontiguousarray(seq[:, order].T)
    items_p, scores_p = eng.recommend_next((padded, lens[order]), k)
    assert np.array_equal(items_p.cpu().numpy(), items) and np.array_equal(scores_p.cpu().numpy(), scores)
    rows = np.concatenate([np.full(len(p), r) for r, p in enumerate(profiles)])
    flat = np.concatenate(profiles)
    items_s, scores_s = eng.recommend_next(profiles, k, seen=(rows, flat))
    items_s = items_s.cpu().numpy()
    seen = [np.unique(np.asarray(p)[np.asarray(p) != 0]) - 1 for p in profiles]
    tk.check_against_float64(items_s - 1, scores_s.cpu().numpy(), s64, seen, "recommend_next with seen")
    for r, p in enumerate(profiles):
        assert not set(items_s[r].tolist()) & set(p)
    many, _ = eng.recommend_next(profiles[:1], 64)
    many = many.cpu().numpy()[0]
    assert sorted(many[:I - 1].tolist()) == list(range(1, I)) and (many[I - 1:] == -1).all()


def test_out_of_range_ids_raise_and_leave_the_engine_usable(hip_device):
    case = "narm_adam"
    g = load_golden(case)
    I = meta(g)[0]
    eng = golden_engine(case, g)
    good = narm_batch(g, 0)
    before = eng.model.flat.clone()
    for slot, at, value in ((0, (0, 0), I), (0, (0, 1), -2), (1, 2, I), (1, 0, -1)):
        bad = [a.copy() for a in good]
        bad[slot][at] = value
        with pytest.raises(IndexError):
            eng.backward_only(tuple(bad))
        assert torch.equal(eng.model.flat, before), "the weights moved"
        assert float(eng._g_flat.abs().max()) == 0.0, "a partial gradient was kept"
    bad = [a.copy() for a in good]
    bad[1][3] = I + 7
    with pytest.raises(IndexError):
        eng.train_single_batch(tuple(bad))
    assert float(eng._g_flat.abs().max()) == 0.0
    with pytest.raises(IndexError):
        eng.model.forward(good[0] * 0 + I, good[2])
    load_weights(eng, narm_params(case, g, 0))
    eng.load_optimizer_state(0)
    loss = eng.train_single_batch(good)
    assert_scalar_close(loss, g["losses"][0], what="loss after the errors")


def test_what_the_reference_cannot_run_is_a_value_error(hip_device):
    case = "narm_adam"
    g = load_golden(case)
    eng = golden_engine(case, g)
    seq, target, lens = narm_batch(g, 0)
    short = lens.copy()
    short[0] -= 1                                            # max(lens) != seq.shape[0]
    zero = lens.copy()
    zero[-1] = 0
    for bad in ((seq, target, short), (seq, target, zero), (seq, target, lens[:-1]), (seq, target[:-1], lens),
                (seq[0], target, lens), (seq, target)):
        with pytest.raises(ValueError):
            eng.train_single_batch(bad)
    with pytest.raises(ValueError):
        eng.model.forward(seq, short)
    with pytest.raises(ValueError):
        eng.recommend_next([[1, 2], []], 3)
    assert_scalar_close(eng.train_single_batch((seq, target, lens)), g["losses"][0], what="loss after the errors")


def test_checkpoint_round_trip(hip_device, tmp_path):
    """Save, load into a fresh engine (weights and optimizer state): the reference's keys, the same next step."""
    case = "narm_adam"
    g = load_golden(case)
    eng = golden_engine(case, g)
    eng.train_single_batch(narm_batch(g, 0))
    path = str(tmp_path / "narm.pt")
    eng.save_checkpoint(path, optimizer_state=True)
    sd = torch.load(path)
    assert tuple(sd) == nn_.keys(meta(g)[4])
    other = golden_engine(case, g)
    with contextlib.redirect_stdout(io.StringIO()):
        other.resume_checkpoint(path, optimizer_state=True)
    assert torch.equal(other.model.flat, eng.model.flat)
    a = eng.train_single_batch(narm_batch(g, 1))
    b = other.train_single_batch(narm_batch(g, 1))
    assert_scalar_close(b, a, 1e-6, "loss after the reload")
    assert_tensor_close(other.model.flat.cpu().numpy(), eng.model.flat.cpu().numpy(), 1e-6, "weights after the step")
