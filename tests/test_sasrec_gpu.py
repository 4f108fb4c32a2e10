"""GPU parity tests of SASRec (csrc/sasrec.hip): forward + loss + backward, the full step and chained steps vs golden
vectors from the real reference's SASRecEngine (tests/golden/sasrec_*.npz); synthetic shapes that cross every tile edge
of the attention kernels against the fp64 restatement; the dropout modes; predict / recommend_next; the epoch's contract
with the sampler; the bounds check; the checkpoint round trip."""
import contextlib
import io

import numpy as np
import pytest
import torch

import sasrec_numpy as sn
import topk_reference as tk
from helpers import REL, assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_sgd_exact
from helpers import assert_step_close, assert_tensor_close, float64_oracle, load_golden, oracle_trajectory, to64
from test_oracle_golden_sasrec import CASES, exact_grads, hyper, meta, model_config, sas_band, sas_batch
from test_oracle_golden_sasrec import sas_keep, sas_opt_state, sas_params

pytestmark = pytest.mark.gpu


def make_engine(w, I, D, H, T, nb, p=0.0, B=8, l2=0.0, optimizer="adam", lr=1e-3, **extra):
    import beta_recsys_amd as hp

    cfg = model_config(I, D, H, T, nb, p, B, l2, optimizer, lr, device="cuda:0")
    cfg["model"].update(extra)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.SASRecEngine(cfg)
    if w is not None:
        load_weights(eng, w)
    return eng


def golden_engine(case, g, **extra):
    I, T, D, H, nb, B, _, _ = meta(g)
    opt, lr, l2, p = hyper(g)
    return make_engine(sas_params(case, g, 0), I, D, H, T, nb, p, B, l2, opt, lr, **extra)


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def load_opt_state(eng, st, opt):
    eng.load_optimizer_state(st["step"], st.get("exp_avg"), st.get("exp_avg_sq", st.get("square_avg")))


def np_grads(grads):
    return {k: v.cpu().numpy() for k, v in grads.items()}


def full_batch(batch):
    return (np.arange(len(batch[0])),) + tuple(batch)


@pytest.mark.parametrize("case", CASES)
def test_step_matches_reference(hip_device, case):
    """Each step from the reference's own weights and optimizer state: the loss, every gradient (as accurate as the
    reference against the fp64 evaluation), the padding row's gradient exactly zero, the stepped weights."""
    g = load_golden(case)
    opt, lr, l2, p = hyper(g)
    H = meta(g)[3]
    eng = golden_engine(case, g)
    for s in range(meta(g)[6]):
        batch, keep = sas_batch(g, s), sas_keep(g, s)
        w0, st0 = sas_params(case, g, s), sas_opt_state(case, g, s)
        load_weights(eng, w0)
        load_opt_state(eng, st0, opt)
        loss, grads = eng.backward_only(full_batch(batch), keep_masks=keep)
        grads = np_grads(grads)
        print(f"{case} step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        g_ref = sas_params(case, g, s + 1, "g")
        _, g64 = exact_grads(w0, batch, H, l2, keep, p)
        for k in g_ref:
            print(f"  grad {k}: err vs exact {np.abs(grads[k].reshape(g64[k].shape) - g64[k]).max():.3e}, reference's "
                  f"own {np.abs(g_ref[k] - g64[k]).max():.3e}, scale {np.abs(g64[k]).max():.3e}")
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}")
        assert float(np.abs(grads["item_emb.weight"][0]).max()) == 0.0, "a gradient reached the padding row"
        assert float(eng._g_flat.abs().max()) == 0.0
        # the full step
        load_opt_state(eng, st0, opt)
        loss = eng.train_single_batch(full_batch(batch), keep_masks=keep)
        assert_scalar_close(loss, g["losses"][s], what=f"loss (step) {s}")
        band = sas_band(w0, st0, g_ref, opt, lr)
        w1, w_ref = get_weights(eng), sas_params(case, g, s + 1)
        for k in w_ref:
            assert_step_close(w0[k], w1[k], w_ref[k], band[k], what=f"weights {k} step {s}")
        assert float(np.abs(w1["item_emb.weight"][0]).max()) == 0.0
        assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"


@pytest.mark.parametrize("case", CASES)
def test_trajectory_matches_reference(hip_device, case):
    """Three steps chained from w0.  SGD: every element within 1e-5 of the trajectory's update; Adam / RMSprop: every
    element inside the oracle's perturbed-gradient envelope around the reference's end point.  Zero outliers."""
    g = load_golden(case)
    opt, lr, l2, p = hyper(g)
    H, steps = meta(g)[3], meta(g)[6]
    eng = golden_engine(case, g)
    w0 = sas_params(case, g, 0)
    batches = [sas_batch(g, s) + (sas_keep(g, s),) for s in range(steps)]
    for s, b in enumerate(batches):
        loss = eng.train_single_batch(full_batch(b[:3]), keep_masks=b[3])
        print(f"{case} chained step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        if opt == "sgd" or s == 0:
            assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
    ref_end = sas_params(case, g, steps)
    if opt == "sgd":
        assert_sgd_exact(get_weights(eng), ref_end, w0, "final weights")
        return
    _, env, upd = oracle_trajectory(
        w0, batches, lambda w, b: sn.sasrec_grads(w, b[:3], H, l2, b[3], p)[1],
        lambda w, gr, st: sn.opt_step(w, gr, st, opt, lr), lambda w: sn.new_opt_state(w, opt))
    assert_on_trajectory(get_weights(eng), ref_end, env, upd, f"{case} trajectory")


def synthetic(I, D, H, T, B, nb, seed, all_padding_row):
    rng = np.random.default_rng(seed)
    w = {}
    for k, shape in sn.shapes(I, T, D, nb).items():
        if k in ("item_emb.weight", "pos_emb.weight"):
            w[k] = rng.standard_normal(shape)
        elif "layernorm" in k and k.endswith("weight"):
            w[k] = 1.0 + 0.3 * rng.standard_normal(shape)
        elif k.endswith("bias"):
            w[k] = 0.2 * rng.standard_normal(shape)
        else:
            w[k] = rng.uniform(-1, 1, shape) / np.sqrt(D)
        w[k] = w[k].astype(np.float32)
    w["item_emb.weight"][0] = 0
    seq, pos, neg = (np.zeros((B, T), dtype=np.int64) for _ in range(3))
    for b in range(B):
        n = T if b == 0 else int(rng.integers(1, T + 1))
        if all_padding_row and b == B - 1:
            continue
        items = rng.integers(1, I + 1, n + 1)
        seq[b, T - n:], pos[b, T - n:] = items[:-1], items[1:]
        neg[b, T - n:] = rng.integers(1, I + 1, n)
    return w, (seq, pos, neg)


@pytest.mark.parametrize("D,H,T,B", [(64, 2, 65, 2), (64, 1, 17, 3), (128, 8, 5, 1), (32, 2, 1, 4), (64, 2, 200, 2)])
def test_shapes_against_the_restatement(hip_device, D, H, T, B):
    """A ragged key tile (T 65), head width 64, head width 16 with a batch of ONE sequence, T = 1 and the default
    length: loss and gradients against the restatement in fp64, as accurate as its fp32 self.  Where the batch has more
    than one sequence, the last one is all padding."""
    I, nb, l2 = 50, 2, 0.05
    w, batch = synthetic(I, D, H, T, B, nb, seed=D + T, all_padding_row=B > 1)
    eng = make_engine(w, I, D, H, T, nb, l2=l2, B=B)
    loss32, g32 = sn.sasrec_grads(w, batch, H, l2)
    loss64, g64 = exact_grads(w, batch, H, l2, None, 0.0)
    loss, grads = eng.backward_only(full_batch(batch))
    grads = np_grads(grads)
    print(f"D {D} H {H} T {T} B {B}: loss {loss!r} vs exact {loss64!r}")
    for k in g64:
        print(f"  grad {k}: err vs exact {np.abs(grads[k].reshape(g64[k].shape) - g64[k]).max():.3e}, fp32 restatement's "
              f"{np.abs(g32[k] - g64[k]).max():.3e}, scale {np.abs(g64[k]).max():.3e}")
    assert_scalar_close(loss, loss64, what="loss")
    assert_grads_as_accurate(grads, g32, g64, what="grad")
    assert float(np.abs(grads["item_emb.weight"][0]).max()) == 0.0
    feats = eng.model.log2feats(batch[0]).cpu().numpy()
    with float64_oracle(sn):
        f64, _ = sn.sasrec_forward(to64(w), batch[0], H)
    assert_tensor_close(feats, f64, what="log2feats")


def test_padded_keys_are_attended_to(hip_device):
    """S3: the reference has no key-padding mask.  On a left-padded batch the loss is the restatement's, which differs
    from the counterfactual WITH such a mask; on fully real sequences the two agree and the kernel with them.  A shift
    of the key third of in_proj_bias moves every score of a row alike: the loss stays where the restatement says."""
    case = "sasrec_adam"
    g = load_golden(case)
    I, T, D, H, nb, B, _, _ = meta(g)
    w = sas_params(case, g, 0)
    eng = make_engine(w, I, D, H, T, nb, B=B)
    batch = sas_batch(g, 0)
    with float64_oracle(sn):
        open_keys = sn.sasrec_loss(to64(w), batch, H, 0.0)
        masked = sn.sasrec_loss(to64(w), batch, H, 0.0, mask_padded_keys=True)
    loss, _ = eng.backward_only(full_batch(batch))
    print(f"left-padded batch: {loss!r}, restatement {open_keys!r}, with a key-padding mask {masked!r}")
    assert abs(masked - open_keys) > 1e-3 * abs(open_keys)
    assert_scalar_close(loss, open_keys, what="left-padded batch")
    real = tuple(a[:1] for a in batch)
    with float64_oracle(sn):
        a = sn.sasrec_loss(to64(w), real, H, 0.0)
        b = sn.sasrec_loss(to64(w), real, H, 0.0, mask_padded_keys=True)
    assert a == b
    loss, _ = eng.backward_only(full_batch(real))
    assert_scalar_close(loss, a, what="fully real batch")
    w2 = {k: v.copy() for k, v in w.items()}
    w2["attention_layers.0.in_proj_bias"][D:2 * D] += 0.5
    load_weights(eng, w2)
    with float64_oracle(sn):
        moved = sn.sasrec_loss(to64(w2), batch, H, 0.0)
    loss, _ = eng.backward_only(full_batch(batch))
    assert_scalar_close(loss, moved, what="moved key bias")
    assert_scalar_close(moved, open_keys, what="a key bias cancels in the softmax")


def test_explicit_masks_equal_the_reference_under_dropout(hip_device):
    """sasrec_rmsprop_drop: with the reference's masks handed in the losses are the reference's; and the default
    ``dropout_rng = "torch_cpu"`` draws those very masks from the fixture's torch seed."""
    case = "sasrec_rmsprop_drop"
    g = load_golden(case)
    opt, lr, l2, p = hyper(g)
    steps, seed = meta(g)[6], meta(g)[7]
    torch.manual_seed(seed)
    eng = golden_engine(case, g)                  # the constructor draws what the reference's constructor drew
    for s in range(steps):
        load_weights(eng, sas_params(case, g, s))
        load_opt_state(eng, sas_opt_state(case, g, s), opt)
        loss = eng.train_single_batch(full_batch(sas_batch(g, s)))
        drawn = [k.cpu().numpy() for k in eng.last_keep_masks]
        assert_scalar_close(loss, g["losses"][s], what=f"torch_cpu loss step {s}")
        for i, (a, b) in enumerate(zip(drawn, sas_keep(g, s))):
            assert np.array_equal(a, b), f"step {s} mask {i} is not the reference's"
    other = golden_engine(case, g)
    for s in range(steps):
        loss = other.train_single_batch(full_batch(sas_batch(g, s)), keep_masks=sas_keep(g, s))
        if s == 0:
            assert_scalar_close(loss, g["losses"][s], what="explicit masks")
    with pytest.raises(ValueError):
        other.train_single_batch(full_batch(sas_batch(g, 0)), keep_masks=sas_keep(g, 0)[:-1])


def test_device_dropout_statistics(hip_device):
    """dropout_rng = "device" at (D 64, H 2, T 50, B 64): the keep rate of each of the 1 + 3 * blocks masks within
    4 sigma of 1 - p, two steps draw different masks, eval mode draws none."""
    I, D, H, T, B, nb, p = 60, 64, 2, 50, 64, 2, 0.2
    w, batch = synthetic(I, D, H, T, B, nb, seed=11, all_padding_row=False)
    eng = make_engine(w, I, D, H, T, nb, p=p, B=B, dropout_rng="device", dropout_seed=5)
    loss1 = eng.train_single_batch(full_batch(batch))
    first = [k.clone() for k in eng.last_keep_masks]
    loss2 = eng.train_single_batch(full_batch(batch))
    second = eng.last_keep_masks
    assert np.isfinite(loss1) and np.isfinite(loss2)
    assert len(first) == 1 + 3 * nb
    shapes = eng._mask_shapes(B, T)
    for i, (a, b) in enumerate(zip(first, second)):
        n = a.numel()
        assert n == int(np.prod(shapes[i])) and a.dtype == torch.uint8
        assert int(a.max()) == 1
        sigma = np.sqrt(p * (1 - p) / n)
        for m in (a, b):
            rate = float(m.float().mean())
            assert abs(rate - (1 - p)) <= 4 * sigma, f"mask {i}: keep rate {rate:.5f}"
        assert not torch.equal(a, b), f"mask {i}: two steps drew the same mask"
    for i in range(len(first)):
        for j in range(i):
            if first[i].numel() == first[j].numel():
                assert not torch.equal(first[i], first[j]), f"masks {i} and {j} of one step are the same draw"
    eng.model.eval()
    load_weights(eng, w)
    loss_eval, _ = eng.backward_only(full_batch(batch))
    assert eng.last_keep_masks is None
    plain = make_engine(w, I, D, H, T, nb, p=0.0, B=B)
    loss_plain, _ = plain.backward_only(full_batch(batch))
    assert plain.last_keep_masks is None
    assert_scalar_close(loss_eval, loss_plain, what="eval mode")


def test_predict_and_recommend_next(hip_device):
    case = "sasrec_adam"
    g = load_golden(case)
    I, T, D, H, nb, B, _, _ = meta(g)
    w = sas_params(case, g, 0)
    eng = golden_engine(case, g)
    seqs = sas_batch(g, 0)[0]
    ids = np.arange(1, I + 1)
    with float64_oracle(sn):
        s64 = sn.predict(to64(w), seqs, ids, H)
    got = eng.model.predict(np.arange(B), seqs, ids)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, I)
    assert_tensor_close(got.cpu().numpy(), s64, what="predict")
    sub = np.array([7, 0, 3, 7])
    with float64_oracle(sn):
        s_sub = sn.predict(to64(w), seqs, sub, H)
    assert_tensor_close(eng.model.predict(None, seqs, sub).cpu().numpy(), s_sub, what="predict on a list with id 0")
    with pytest.raises(IndexError):
        eng.model.predict(None, seqs, [1, I + 1])
    k = 6
    items, scores = eng.recommend_next(seqs, k)
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    assert items.shape == (B, k) and (items >= 1).all() and (items <= I).all()
    tk.check_against_float64(items - 1, scores, s64, None, "recommend_next")
    # seen: (rows, items) in the model's ids -- here every item of the row's own sequence; id 0 entries are ignored
    rows = np.repeat(np.arange(B), T)
    items_s, scores_s = eng.recommend_next(seqs, k, seen=(rows, seqs.reshape(-1)))
    items_s = items_s.cpu().numpy()
    seen = [np.unique(seqs[b][seqs[b] != 0]) - 1 for b in range(B)]
    tk.check_against_float64(items_s - 1, scores_s.cpu().numpy(), s64, seen, "recommend_next with seen")
    for b in range(B):
        assert not set(items_s[b].tolist()) & set(seqs[b].tolist())
    # more than the catalogue holds: the tail is -1 / -inf, never the padding row
    many, _ = eng.recommend_next(seqs[:1], 64)
    many = many.cpu().numpy()[0]
    assert sorted(many[:I].tolist()) == list(range(1, I + 1)) and (many[I:] == -1).all()


class StubSampler:
    def __init__(self, g):
        self.g, self.calls = g, 0

    def next_batch(self):
        seq, pos, neg = sas_batch(self.g, self.calls % meta(self.g)[6])
        self.calls += 1
        return tuple(range(len(seq))), tuple(map(tuple, seq)), tuple(map(tuple, pos)), tuple(map(tuple, neg))


def test_train_an_epoch_asks_the_sampler_as_the_reference_does(hip_device):
    case = "sasrec_sgd_h1"
    g = load_golden(case)
    eng = golden_engine(case, g)
    B = meta(g)[5]
    eng.num_batch = 3                                     # the fixture's three batches make one epoch
    assert golden_engine(case, g).num_batch == 64 // B    # n_users // batch_size, as the reference computes it
    sampler = StubSampler(g)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        eng.train_an_epoch(sampler, 4)
    assert sampler.calls == 3
    tag, total, epoch_id = eng.writer.scalars[-1]
    assert (tag, epoch_id) == ("model/loss", 4)
    assert_scalar_close(total, float(g["losses"].sum()), 2 * REL, "epoch loss sum")
    assert out.getvalue().strip() == "[Training Epoch 4], Loss {}".format(total)
    assert_sgd_exact(get_weights(eng), sas_params(case, g, 3), sas_params(case, g, 0), "after the epoch")
    full = golden_engine(case, g)
    sampler = StubSampler(g)
    with contextlib.redirect_stdout(io.StringIO()):
        full.train_an_epoch(sampler, 0)
    assert sampler.calls == 64 // B


def test_out_of_range_ids_raise_and_leave_the_engine_usable(hip_device):
    case = "sasrec_adam"
    g = load_golden(case)
    I = meta(g)[0]
    eng = golden_engine(case, g)
    good = sas_batch(g, 0)
    before = eng.model.flat.clone()
    for slot, value in ((0, I + 1), (1, I + 1), (2, -1), (0, -3)):
        bad = [a.copy() for a in good]
        bad[slot][0, -1] = value
        with pytest.raises(IndexError):
            eng.backward_only(full_batch(bad))
        assert torch.equal(eng.model.flat, before), "the weights moved"
        assert float(eng._g_flat.abs().max()) == 0.0, "a partial gradient was kept"
    bad = [a.copy() for a in good]
    bad[1][2, 3] = I + 7
    with pytest.raises(IndexError):
        eng.train_single_batch(full_batch(bad))
    assert float(eng._g_flat.abs().max()) == 0.0
    with pytest.raises(IndexError):
        eng.model.log2feats(bad[0] * 0 + I + 1)
    with pytest.raises(ValueError):
        eng.train_single_batch(good)
    with pytest.raises(ValueError):
        eng.train_single_batch(full_batch((good[0], good[1][:, :-1], good[2])))
    with pytest.raises(ValueError):
        eng.model.log2feats(np.ones((2, meta(g)[1] + 1), dtype=np.int64))
    load_weights(eng, sas_params(case, g, 0))
    eng.load_optimizer_state(0)
    loss = eng.train_single_batch(full_batch(good))
    assert_scalar_close(loss, g["losses"][0], what="loss after the errors")


def test_checkpoint_round_trip(hip_device, tmp_path):
    """Save, load into a fresh engine (weights and optimizer state): the next step's loss and weights are identical."""
    case = "sasrec_adam"
    g = load_golden(case)
    eng = golden_engine(case, g)
    eng.train_single_batch(full_batch(sas_batch(g, 0)))
    path = str(tmp_path / "sasrec.pt")
    eng.save_checkpoint(path, optimizer_state=True)
    sd = torch.load(path)
    assert tuple(sd) == sn.keys(meta(g)[4])
    other = golden_engine(case, g)
    with contextlib.redirect_stdout(io.StringIO()):
        other.resume_checkpoint(path, optimizer_state=True)
    assert torch.equal(other.model.flat, eng.model.flat)
    # the forward pass and the loss sum in a fixed order: the same weights give the same loss bit for bit
    a = eng.train_single_batch(full_batch(sas_batch(g, 1)))
    b = other.train_single_batch(full_batch(sas_batch(g, 1)))
    assert a == b
    assert_tensor_close(other.model.flat.cpu().numpy(), eng.model.flat.cpu().numpy(), 1e-6, "weights after the step")
