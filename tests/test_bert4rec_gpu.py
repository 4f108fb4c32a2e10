"""BERT4Rec on the GPU beyond single gradients: device-drawn dropout, chained optimizer steps against the restatement,
``predict`` / ``recommend_next``, the bounds checks, the epoch's contract with the sampler, the checkpoint round trip."""
import contextlib
import io

import numpy as np
import pytest
import torch

import bert4rec_edges as be
import bert4rec_torch as bt
import topk_reference as tk
from helpers import assert_on_trajectory, assert_scalar_close, assert_sgd_exact, assert_tensor_close, oracle_trajectory
from test_bert4rec_edges_gpu import batch_of, load_weights, make_engine

pytestmark = pytest.mark.gpu


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def three_batches(f):
    """Three batches on the fixture's histories: the fixture's own masking and two more draws."""
    rng = np.random.default_rng(9)
    hist = np.where(f["labels"] != 0, f["labels"], f["seq"])
    out = [(f["seq"], f["labels"])]
    real = np.flatnonzero(hist.reshape(-1))
    for _ in range(2):
        out.append(be.mask(hist, np.sort(rng.choice(real, max(1, real.size // 5), replace=False)), f["I"]))
    return out


def test_device_dropout_statistics(hip_device):
    """dropout_rng = "device" (the default) on t200 (B 2, T 200, D 64, H 2, two blocks): the masks hold 25 600 bytes
    ([B * T, D]) or 160 000 ([B * H, T, T]), so four standard deviations of the keep rate are 1.0e-2 / 4.0e-3; two steps
    draw different masks; eval mode draws none."""
    f = be.fixture("t200")
    p = 0.2
    eng = make_engine(f, p=p, dropout_seed=5)
    assert eng.config["model"]["dropout_rng"] == "device"
    loss1 = eng.train_single_batch(batch_of(f))
    first = [k.clone() for k in eng.last_keep_masks]
    loss2 = eng.train_single_batch(batch_of(f))
    second = eng.last_keep_masks
    assert np.isfinite(loss1) and np.isfinite(loss2)
    shapes = eng._mask_shapes(f["B"], f["T"])
    assert len(first) == 1 + 3 * f["blocks"] == len(shapes)
    for i, (a, b) in enumerate(zip(first, second)):
        n = a.numel()
        assert n == int(np.prod(shapes[i])) >= 25600 and a.dtype == torch.uint8 and int(a.max()) == 1
        sigma = np.sqrt(p * (1 - p) / n)
        for m in (a, b):
            rate = float(m.float().mean())
            assert abs(rate - (1 - p)) <= 4 * sigma, f"mask {i}: keep rate {rate:.5f}"
        assert not torch.equal(a, b), f"mask {i}: two steps drew the same mask"
    eng.model.eval()
    load_weights(eng, f["w"])
    loss_eval, _ = eng.backward_only(batch_of(f))
    assert eng.last_keep_masks is None
    assert_scalar_close(loss_eval, be.reference("t200")[0], what="eval mode")


@pytest.mark.parametrize("optimizer,lr", [("sgd", 0.05), ("adam", 1e-3)])
def test_three_chained_steps(hip_device, optimizer, lr):
    """SGD: every element within 1e-5 of the trajectory's update; Adam: every element inside the restatement's
    perturbed-gradient envelope.  Zero outliers."""
    f = be.fixture("t65")
    H = f["H"]
    batches = three_batches(f)
    eng = make_engine(f, optimizer=optimizer, lr=lr)
    for s, (seq, labels) in enumerate(batches):
        loss = eng.train_single_batch((np.arange(f["B"]), seq, labels))
        if s == 0:
            assert_scalar_close(loss, be.reference("t65")[0], what="loss step 0")
    grad_fn = lambda w, b: {k: v.astype(np.float32) for k, v in bt.grads(w, b[0], b[1], H, dtype=torch.float32)[1].items()}  # noqa: E731
    w_ref, env, upd = oracle_trajectory(
        f["w"], batches, grad_fn, lambda w, g, st: bt.opt_step(w, g, st, optimizer, lr),
        lambda w: bt.new_opt_state(w, optimizer), trials=0 if optimizer == "sgd" else 8)
    if optimizer == "sgd":
        assert_sgd_exact(get_weights(eng), w_ref, f["w"], "final weights")
    else:
        assert_on_trajectory(get_weights(eng), w_ref, env, upd, "adam trajectory")
    assert float(np.abs(get_weights(eng)["item_emb.weight"][0]).max()) == 0.0


def test_predict_and_recommend_next(hip_device):
    f = be.fixture("bias_spread")
    I, T, H = f["I"], f["T"], f["H"]
    eng = make_engine(f)
    rng = np.random.default_rng(4)
    hist = [rng.integers(1, I + 1, n).tolist() for n in (3, 1, T - 1, T + 6)]      # the last is longer than maxlen - 1
    q = eng.query_sequences(hist)
    assert q.shape == (4, T) and q[3, :-1].tolist() == hist[3][-(T - 1):]
    s64 = bt.next_item_scores(f["w"], q, H)
    ids = np.arange(1, I + 1)
    got = eng.model.predict(q, ids)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, I)
    assert_tensor_close(got.cpu().numpy(), s64, what="predict")
    for bad in ([0, 1], [1, I + 1]):
        with pytest.raises(IndexError):
            eng.model.predict(q, bad)
    k = 7
    items, scores = eng.recommend_next(hist, k)
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    assert items.shape == (4, k) and (items >= 1).all() and (items <= I).all()
    tk.check_against_float64(items - 1, scores, s64, None, "recommend_next")
    exact_items, _ = tk.exact_topk(s64, None, k)
    assert np.array_equal(items - 1, exact_items), "not the brute-force ranking (ties to the lower id)"
    # the bias decides: without it the first place would differ somewhere
    assert (items[:, 0] - 1 != (s64 - f["w"]["out_bias"][1:]).argmax(1)).any()
    rows = np.concatenate([np.full(len(h), r) for r, h in enumerate(hist)] + [[0]])
    seen_items = np.concatenate(hist + [[0]])                          # a 0 entry is ignored
    items_s, scores_s = eng.recommend_next(hist, k, seen=(rows, seen_items))
    items_s = items_s.cpu().numpy()
    seen = [np.unique(h) - 1 for h in hist]
    tk.check_against_float64(items_s - 1, scores_s.cpu().numpy(), s64, seen, "recommend_next with seen")
    assert np.array_equal(items_s - 1, tk.exact_topk(s64, seen, k)[0])
    for r, h in enumerate(hist):
        assert not set(items_s[r].tolist()) & set(h)
    # more than is left: the tail is -1 / -inf, never 0 or the [MASK] id
    many, many_s = eng.recommend_next(hist[:1], 128, seen=(np.zeros(3, dtype=np.int64), np.array(hist[0])))
    many = many.cpu().numpy()[0]
    left = I - np.unique(hist[0]).size
    assert sorted(many[:left].tolist()) == sorted(set(range(1, I + 1)) - set(hist[0])) and (many[left:] == -1).all()
    assert np.isneginf(many_s.cpu().numpy()[0, left:]).all()
    assert 0 not in many and eng.model.mask_id not in many
    with pytest.raises(ValueError):
        eng.recommend_next([[1, eng.model.mask_id]], 3)
    for bad_seen in (([0], [eng.model.mask_id]), ([0], [-1]), ([4], [1]), ([-1], [1])):
        with pytest.raises(ValueError):
            eng.recommend_next(hist, 3, seen=bad_seen)


def test_out_of_range_ids_raise_and_leave_the_engine_usable(hip_device):
    f = be.fixture("t65")
    I = f["I"]
    eng = make_engine(f)
    before = eng.model.flat.clone()
    users = np.arange(f["B"])
    for slot, at, value in ((0, (0, 3), I + 2), (0, (0, 3), -1), (1, (0, 5), I + 1), (1, (0, 5), -2)):
        bad = [f["seq"].copy(), f["labels"].copy()]
        bad[slot][at] = value
        with pytest.raises(IndexError):
            eng.backward_only((users, bad[0], bad[1]))
        assert torch.equal(eng.model.flat, before), "the weights moved"
        assert float(eng._g_flat.abs().max()) == 0.0, "a partial gradient was kept"
    with pytest.raises(IndexError):
        eng.model.log2feats(f["seq"] * 0 + I + 2)
    with pytest.raises(ValueError):
        eng.train_single_batch((users, f["seq"], f["labels"], f["labels"]))
    with pytest.raises(ValueError):
        eng.train_single_batch((users, f["seq"], f["labels"][:, :-1]))
    with pytest.raises(ValueError):
        eng.model.log2feats(np.ones((2, f["T"] + 1), dtype=np.int64))
    loss, _ = eng.backward_only(batch_of(f))
    assert_scalar_close(loss, be.reference("t65")[0], what="loss after the errors")
    # labels on the device take the torch.nonzero path to the same list
    loss_dev, _ = eng.backward_only((users, f["seq"], torch.from_numpy(f["labels"]).cuda()))
    assert loss_dev == loss


class StubSampler:
    def __init__(self, f):
        self.batches, self.calls = three_batches(f), 0

    def next_batch(self):
        seq, labels = self.batches[self.calls % 3]
        self.calls += 1
        return tuple(range(len(seq))), tuple(map(tuple, seq)), tuple(map(tuple, labels))


def test_train_an_epoch_asks_the_sampler(hip_device):
    f = be.fixture("one_seq")
    eng = make_engine(f, optimizer="sgd", lr=0.05)
    assert eng.num_batch == 64 // f["B"]
    eng.num_batch = 3
    sampler = StubSampler(f)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        eng.train_an_epoch(sampler, 4)
    assert sampler.calls == 3
    tag, total, epoch_id = eng.writer.scalars[-1]
    assert (tag, epoch_id) == ("model/loss", 4) and np.isfinite(total)
    assert out.getvalue().strip() == "[Training Epoch 4], Loss {}".format(total)


def test_checkpoint_round_trip(hip_device, tmp_path):
    """Save, load into a fresh engine (weights and optimizer state): the next step's loss is identical and the weights
    agree bit for bit except the atomically accumulated item rows, which are held to 1e-6."""
    f = be.fixture("t65")
    batches = three_batches(f)
    users = np.arange(f["B"])
    eng = make_engine(f)
    eng.train_single_batch((users,) + batches[0])
    path = str(tmp_path / "bert4rec.pt")
    eng.save_checkpoint(path, optimizer_state=True)
    assert tuple(torch.load(path)) == bt.keys(f["blocks"])
    other = make_engine(f, w={k: np.zeros_like(v) for k, v in f["w"].items()})
    with contextlib.redirect_stdout(io.StringIO()):
        other.resume_checkpoint(path, optimizer_state=True)
    assert torch.equal(other.model.flat, eng.model.flat)
    a = eng.train_single_batch((users,) + batches[1])
    b = other.train_single_batch((users,) + batches[1])
    assert a == b
    wa, wb = get_weights(eng), get_weights(other)
    for k in wa:
        if k == "item_emb.weight":
            assert_tensor_close(wb[k], wa[k], 1e-6, "item_emb after the step")
        else:
            assert np.array_equal(wa[k], wb[k]), f"{k} differs after the round trip"
