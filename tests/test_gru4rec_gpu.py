"""GRU4Rec on the GPU beyond single gradients: chained Adam steps with the state carried and a reset on the way, ``step`` /
``forward`` / ``predict`` / ``recommend_next``, the bounds checks, the dropout masks, the epoch over a
``SessionParallelLoader``."""
import contextlib
import io

import numpy as np
import pytest
import torch

import gru4rec_edges as ge
import gru4rec_torch as gt
import topk_reference as tk
from helpers import REL, assert_on_trajectory, assert_scalar_close, assert_tensor_close, oracle_trajectory
from test_gru4rec_edges_gpu import get_state, load_state, make_engine, run_fixture

pytestmark = pytest.mark.gpu


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def five_steps(f):
    """``(step, in_items, targets, reset, samples)``: the fixture's own step and four more draws of the same shapes; no
    slot restarts after the first step except in step 3, where two do."""
    rng = np.random.default_rng(17)
    out = [(0,) + ge.batch_of(f)]
    for s in range(1, 5):
        reset = np.zeros(f["B"], dtype=np.uint8)
        if s == 3:
            reset[[1, 4]] = 1
        out.append((s, rng.integers(0, f["I"], f["B"]), rng.integers(0, f["I"], f["B"]), reset,
                    rng.integers(0, f["I"], f["S"])))
    return out


@pytest.mark.parametrize("name", ["defaults", "xe"])
def test_five_chained_adam_steps_carry_the_state(hip_device, name):
    """``torch.optim.Adam`` on the restatement's gradients, the state handed from step to step: every element inside the
    envelope of the restatement's own perturbed-gradient runs.  Zero outliers."""
    f = ge.fixture(name)
    cfg, lr = ge.cfg_of(f), 1e-3
    steps = five_steps(f)
    eng = make_engine(f, lr=lr)
    load_state(eng, f["state"])
    for b in steps:
        loss = eng.train_single_batch(b[1:])
        if b[0] == 0:
            assert_scalar_close(loss, ge.reference(name)[0], what="loss step 0")
    carried = {}

    def grad_fn(w, b):
        state = f["state"] if b[0] == 0 else carried["state"]
        _, g, carried["state"] = gt.grads(w, cfg, b[1:], state, None, torch.float32)
        return {k: v.astype(np.float32) for k, v in g.items()}

    w_ref, env, upd = oracle_trajectory(f["w"], steps, grad_fn, lambda w, g, st: gt.adam_step(w, g, st, lr),
                                        gt.new_opt_state)
    assert_on_trajectory(get_weights(eng), w_ref, env, upd, "adam trajectory")


def test_step_forward_predict_and_recommend_next(hip_device):
    f = ge.fixture("stacked")
    I, cfg = f["I"], ge.cfg_of(f)
    eng = make_engine(f)
    eng.model.eval()
    # one eval step from the fixture's state: h_last, the new state, the scores
    load_state(eng, f["state"])
    h = eng.model.step(f["in_items"], f["reset"])
    h64, s64 = gt.step_state(f["w"], cfg, f["in_items"], f["reset"], f["state"])
    assert_tensor_close(h.cpu().numpy(), h64, what="step")
    for l, (got, want) in enumerate(zip(get_state(eng), s64)):
        assert_tensor_close(got, want, what=f"state of layer {l} after the eval step")
    load_state(eng, f["state"])
    scores = eng.model.forward(f["in_items"], f["reset"])
    want = h64 @ f["w"]["Wy.weight"].astype(np.float64).T + f["w"]["By.weight"][:, 0].astype(np.float64)
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (f["B"], I)
    assert_tensor_close(scores.cpu().numpy(), want, what="forward")
    # without a reset argument no slot restarts
    load_state(eng, f["state"])
    assert_tensor_close(eng.model.step(f["in_items"]).cpu().numpy(),
                        gt.step_state(f["w"], cfg, f["in_items"], None, f["state"])[0], what="step without reset")
    # ragged profiles; the carried state is left alone
    rng = np.random.default_rng(4)
    profiles = [rng.integers(0, I, n).tolist() for n in (3, 1, 6, 2)]
    n64 = gt.next_item_scores(f["w"], cfg, profiles)
    load_state(eng, f["state"])
    before = [s.clone() for s in eng.model.state]
    for r, prof in enumerate(profiles):
        got = eng.predict(prof)
        assert got.shape == (I,) and got.dtype == np.float32
        assert_tensor_close(got, n64[r], what=f"predict profile {r}")
    assert all(torch.equal(a, b) for a, b in zip(before, eng.model.state)), "inference moved the carried state"
    k = 7
    gaps = -np.diff(-np.sort(-n64, axis=1), axis=1)
    assert gaps.min() > 4 * REL * np.abs(n64).max(), "the fixture separates its scores"
    items, scores = eng.recommend_next(profiles, k)
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    assert items.shape == (4, k) and (items >= 0).all() and (items < I).all()
    tk.check_against_float64(items, scores, n64, None, "recommend_next")
    assert np.array_equal(items, tk.exact_topk(n64, None, k)[0]), "not the brute-force ranking"
    # the (padded, lengths) form gives the same; what lies behind a length is not read
    T = max(len(p) for p in profiles)
    padded = np.full((4, T), I + 5, dtype=np.int64)
    for r, p in enumerate(profiles):
        padded[r, :len(p)] = p
    items_p, scores_p = eng.recommend_next((padded, [len(p) for p in profiles]), k)
    assert np.array_equal(items_p.cpu().numpy(), items) and np.array_equal(scores_p.cpu().numpy(), scores)
    rows = np.concatenate([np.full(len(p), r) for r, p in enumerate(profiles)])
    seen_items = np.concatenate(profiles)
    items_s, scores_s = eng.recommend_next(profiles, k, seen=(rows, seen_items))
    items_s = items_s.cpu().numpy()
    seen = [np.unique(p) for p in profiles]
    tk.check_against_float64(items_s, scores_s.cpu().numpy(), n64, seen, "recommend_next with seen")
    assert np.array_equal(items_s, tk.exact_topk(n64, seen, k)[0])
    for r, p in enumerate(profiles):
        assert not set(items_s[r].tolist()) & set(p)
    # more than is left: the tail is -1 / -inf
    many, many_s = eng.recommend_next(profiles[:1], I + 4, seen=(np.zeros(3, dtype=np.int64), np.array(profiles[0])))
    many = many.cpu().numpy()[0]
    left = I - len(set(profiles[0]))
    assert sorted(many[:left].tolist()) == sorted(set(range(I)) - set(profiles[0])) and (many[left:] == -1).all()
    assert np.isneginf(many_s.cpu().numpy()[0, left:]).all()
    for bad_seen in (([0], [I]), ([0], [-1]), ([4], [1]), ([-1], [1]), ([0, 1], [1])):
        with pytest.raises(ValueError):
            eng.recommend_next(profiles, 3, seen=bad_seen)
    with pytest.raises(ValueError):
        eng.recommend_next([[1, 2], []], 3)


def test_out_of_range_ids_raise_and_leave_the_engine_usable(hip_device):
    f = ge.fixture("defaults")
    I = f["I"]
    eng = make_engine(f)
    before = eng.model.flat.clone()
    # slot of (in_items, targets, reset, samples), position, value
    for slot, at, value in ((0, 2, I), (0, 2, -1), (1, 0, I), (1, 6, -3), (3, 1, I + 7), (3, 4, -1)):
        bad = [np.array(a).copy() for a in ge.batch_of(f)]
        bad[slot][at] = value
        load_state(eng, f["state"])
        with pytest.raises(IndexError):
            eng.backward_only(tuple(bad))
        assert torch.equal(eng.model.flat, before), "the weights moved"
        assert float(eng._g_flat.abs().max()) == 0.0, "a partial gradient was kept"
    for value in (I, -1):
        ids = f["in_items"].copy()
        ids[3] = value
        with pytest.raises(IndexError):
            eng.model.step(ids)
    in_items, targets, reset, samples = ge.batch_of(f)
    for bad_batch in ((in_items, targets, reset), (in_items, targets[:-1], reset, samples),
                      (in_items, targets, reset[:-1], samples), (in_items[:-1], targets[:-1], reset[:-1], samples)):
        with pytest.raises(ValueError):      # the last: the carried state holds another number of slots
            eng.train_single_batch(bad_batch)
    loss, _ = run_fixture(eng, f)
    assert_scalar_close(loss, ge.reference("defaults")[0], what="loss after the errors")
    load_state(eng, f["state"])
    first = eng.train_single_batch(ge.batch_of(f))
    assert first == loss and not torch.equal(eng.model.flat, before), "the engine trains on"


@pytest.mark.parametrize("rng", ["device", "torch_cpu"])
def test_dropout_masks_have_the_stated_shapes_and_rates(hip_device, rng):
    """One mask [B, in_0] and one [B, H_l] per layer and step; tile_edges_B_129 with layers [3] holds 387 bytes per mask,
    so the two steps' masks are pooled: four standard deviations of the keep rate at 774 draws are 6.6e-2 (p 0.3)."""
    f = ge.fixture("tile_edges_B_129")
    pe, ph = 0.3, 0.3
    eng = make_engine(dict(f, pe=pe, ph=ph), dropout_rng=rng, dropout_seed=5)
    torch.manual_seed(3)
    load_state(eng, f["state"])
    loss1 = eng.train_single_batch(ge.batch_of(f))
    first = [k.clone() for k in eng.last_keep_masks]
    loss2 = eng.train_single_batch(ge.batch_of(f))
    second = eng.last_keep_masks
    assert np.isfinite(loss1) and np.isfinite(loss2)
    assert eng._mask_shapes(f["B"]) == [(f["B"], 3), (f["B"], 3)] and len(first) == len(second) == 2
    for a, b, p in zip(first, second, (pe, ph)):
        n = 2 * f["B"] * 3
        assert a.numel() == b.numel() == n // 2 and a.dtype == torch.uint8 and int(a.max()) == 1
        rate = float(torch.cat([a, b]).float().mean())
        assert abs(rate - (1 - p)) <= 4 * np.sqrt(p * (1 - p) / n), f"keep rate {rate:.5f}"
        assert not torch.equal(a, b), "two steps drew the same mask"
    assert not torch.equal(first[0], first[1]), "the embed and the hidden mask are the same draw"
    if rng == "torch_cpu":
        torch.manual_seed(3)
        again = [torch.empty(f["B"], 3).bernoulli_(1 - p).to(torch.uint8).reshape(-1) for p in (pe, ph)]
        assert all(torch.equal(a, b.cpu()) for a, b in zip(again, first)), "the torch seed does not reproduce the masks"
    # a rate of 0 draws nothing
    only_h = make_engine(dict(f, pe=0.0, ph=ph), dropout_rng=rng)
    load_state(only_h, f["state"])
    only_h.train_single_batch(ge.batch_of(f))
    assert only_h.last_keep_masks[0] is None and only_h.last_keep_masks[1] is not None
    eng.model.eval()
    eng.backward_only(ge.batch_of(f))
    assert eng.last_keep_masks is None
    with pytest.raises(ValueError):
        bad = make_engine(dict(f, pe=pe, ph=ph), dropout_rng="numpy")
        load_state(bad, f["state"])
        bad.train_single_batch(ge.batch_of(f))


def test_train_an_epoch_equals_its_steps_one_by_one(hip_device):
    """Every step of a ``SessionParallelLoader`` epoch from a zero state with one host sync: the mean loss is that of the
    same steps taken one by one, and weights and state agree outside the atomically accumulated tables' rounding."""
    import beta_recsys_amd as hp

    f = ge.fixture("logq")
    rng = np.random.default_rng(2)
    sessions = [rng.integers(0, f["I"], rng.integers(1, 9)).tolist() for _ in range(40)]
    sessions = [s for s in sessions if len(s) >= 2]

    def loader():
        return hp.data.SessionParallelLoader(sessions, f["I"], f["B"], f["S"], f["alpha"], seed=6)

    eng = make_engine(f, optimizer="sgd", lr=0.05)
    load_state(eng, f["state"])                      # the epoch starts from zero whatever was there
    own = loader()
    with contextlib.redirect_stdout(io.StringIO()):
        mean = eng.train_an_epoch(own, 4)
    assert own.device == eng.model.flat.device and len(own) > 4
    assert torch.equal(eng._log_p.cpu(), torch.log(torch.as_tensor(own.item_probs)).float()), "the loader's event shares"
    other = make_engine(f, optimizer="sgd", lr=0.05)
    other.set_item_probs(own.item_probs)
    other.model.reset_state(f["B"])
    steps = list(loader())
    assert len(steps) == len(own) and any(int(s[2].sum()) for s in steps[1:]), "a slot restarts inside the epoch"
    losses = [other.train_single_batch(s) for s in steps]
    assert_scalar_close(mean, float(np.mean(losses)), what="mean epoch loss")
    tag, total, epoch_id = eng.writer.scalars[-1]
    assert (tag, epoch_id) == ("model/loss", 4) and total == mean
    wa, wb = get_weights(eng), get_weights(other)
    for k in wa:
        assert_tensor_close(wa[k], wb[k], 1e-6, f"{k} after the epoch")
    for a, b in zip(get_state(eng), get_state(other)):
        assert_tensor_close(a, b, 1e-6, "state after the epoch")
