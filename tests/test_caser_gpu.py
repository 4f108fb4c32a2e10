"""Caser on the GPU beyond single gradients: chained Adam steps with weight decay against the restatement, ``query`` /
``predict`` / ``recommend_next``, the bounds checks, the dropout masks, the epoch over a ``WindowSampler``."""
import contextlib
import io

import numpy as np
import pytest
import torch

import caser_edges as ce
import caser_torch as ct
import topk_reference as tk
from helpers import REL, assert_on_trajectory, assert_scalar_close, assert_tensor_close, oracle_trajectory
from test_caser_edges_gpu import load_weights, make_engine

pytestmark = pytest.mark.gpu


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def five_batches(f):
    """The fixture's own batch and four more draws of the same shapes (distinct items per sequence)."""
    rng = np.random.default_rng(17)
    out = [ce.batch_of(f)]
    for _ in range(4):
        out.append((rng.integers(0, f["U"], f["B"]), np.argsort(rng.random((f["B"], f["I"])), axis=1)[:, :f["L"]] + 1,
                    rng.integers(1, f["I"] + 1, (f["B"], f["T"])), rng.integers(1, f["I"] + 1, (f["B"], f["N"]))))
    return out


def test_five_chained_adam_steps_with_weight_decay(hip_device):
    """``torch.optim.Adam(weight_decay=l2)`` on the restatement's gradients: every element inside the envelope of the
    restatement's own perturbed-gradient runs.  Zero outliers."""
    f = ce.fixture("defaults")
    assert f["l2"] > 0
    lr = 1e-3
    batches = five_batches(f)
    eng = make_engine(f, lr=lr)
    for s, b in enumerate(batches):
        loss = eng.train_single_batch(b)
        if s == 0:
            assert_scalar_close(loss, ce.reference("defaults")[0], what="loss step 0")

    def grad_fn(w, b):
        g = ct.grads(w, b[1], b[0], b[2], b[3], f["ac_conv"], f["ac_fc"], f["l2"], dtype=torch.float32)[1]
        return {k: v.astype(np.float32) for k, v in g.items()}

    w_ref, env, upd = oracle_trajectory(f["w"], batches, grad_fn, lambda w, g, st: ct.adam_step(w, g, st, lr),
                                        ct.new_opt_state)
    got = get_weights(eng)
    assert_on_trajectory(got, w_ref, env, upd, "adam trajectory")
    assert float(np.abs(got["item_embeddings.weight"][0]).max()) == 0.0, "the padding row moved"


def test_query_predict_and_recommend_next(hip_device):
    f = ce.fixture("defaults")
    I, L = f["I"], f["L"]
    eng = make_engine(f)
    rng = np.random.default_rng(4)
    hist = [rng.permutation(I)[:n].tolist() for n in (3, 1, L, L + 6)]       # ids 0 .. I - 1 shifted below
    hist = [[i + 1 for i in h] for h in hist]
    users = np.array([2, 0, 5, 2])
    import beta_recsys_amd as hp

    q = hp.data.last_window(hist, L)
    assert q.shape == (4, L) and q[3].tolist() == hist[3][-L:] and q[1].tolist() == [0] * (L - 1) + hist[1]
    s64 = ct.next_item_scores(f["w"], q, users)
    assert_tensor_close(eng.model.query(q, users).cpu().numpy(), ct.query(f["w"], q, users), what="query")
    ids = np.arange(1, I + 1)
    got = eng.predict(q, users, ids)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, I)
    assert_tensor_close(got.cpu().numpy(), s64, what="predict")
    some = rng.integers(1, I + 1, (4, 5))
    assert_tensor_close(eng.predict(q, users, some).cpu().numpy(), np.take_along_axis(s64, some - 1, 1), what="predict [B, K]")
    for bad in ([0, 1], [1, I + 1]):
        with pytest.raises(IndexError):
            eng.predict(q, users, bad)
    k = 7
    # the fixture separates its scores: neighbours in the ranking are further apart than the bound on a score
    gaps = -np.diff(-np.sort(-s64, axis=1), axis=1)
    assert gaps.min() > 4 * REL * np.abs(s64).max()
    items, scores = eng.recommend_next(hist, users, k)
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    assert items.shape == (4, k) and (items >= 1).all() and (items <= I).all()
    tk.check_against_float64(items - 1, scores, s64, None, "recommend_next")
    assert np.array_equal(items - 1, tk.exact_topk(s64, None, k)[0]), "not the brute-force ranking"
    # b2 decides somewhere: without it the first place would differ
    assert (items[:, 0] - 1 != (s64 - f["w"]["b2.weight"][1:, 0]).argmax(1)).any()
    rows = np.concatenate([np.full(len(h), r) for r, h in enumerate(hist)] + [[0]])
    seen_items = np.concatenate(hist + [[0]])                          # a 0 entry is ignored
    items_s, scores_s = eng.recommend_next(hist, users, k, seen=(rows, seen_items))
    items_s = items_s.cpu().numpy()
    seen = [np.unique(h) - 1 for h in hist]
    tk.check_against_float64(items_s - 1, scores_s.cpu().numpy(), s64, seen, "recommend_next with seen")
    assert np.array_equal(items_s - 1, tk.exact_topk(s64, seen, k)[0])
    for r, h in enumerate(hist):
        assert not set(items_s[r].tolist()) & set(h)
    # more than is left: the tail is -1 / -inf, never the padding id
    many, many_s = eng.recommend_next(hist[:1], users[:1], 64, seen=(np.zeros(3, dtype=np.int64), np.array(hist[0])))
    many = many.cpu().numpy()[0]
    left = I - len(hist[0])
    assert sorted(many[:left].tolist()) == sorted(set(range(1, I + 1)) - set(hist[0])) and (many[left:] == -1).all()
    assert np.isneginf(many_s.cpu().numpy()[0, left:]).all() and 0 not in many
    for bad_seen in (([0], [I + 1]), ([0], [-1]), ([4], [1]), ([-1], [1])):
        with pytest.raises(ValueError):
            eng.recommend_next(hist, users, 3, seen=bad_seen)


def test_out_of_range_ids_raise_and_leave_the_engine_usable(hip_device):
    f = ce.fixture("defaults")
    I, U = f["I"], f["U"]
    eng = make_engine(f)
    before = eng.model.flat.clone()
    # slot of (users, seq, pos, neg), position, value
    for slot, at, value in ((1, (0, 3), I + 1), (1, (0, 3), -1), (2, (1, 0), I + 1), (3, (2, 1), -2), (0, (4,), U),
                            (0, (4,), -1)):
        bad = [np.array(a).copy() for a in ce.batch_of(f)]
        bad[slot][at] = value
        with pytest.raises(IndexError):
            eng.backward_only(tuple(bad))
        assert torch.equal(eng.model.flat, before), "the weights moved"
        assert float(eng._g_flat.abs().max()) == 0.0, "a partial gradient was kept"
    with pytest.raises(IndexError):
        eng.model.query(f["seq"] * 0 + I + 1, f["users"])
    with pytest.raises(IndexError):
        eng.model.query(f["seq"], f["users"] * 0 + U)
    users, seq, pos, neg = ce.batch_of(f)
    for bad_batch in ((users, seq, pos), (users, seq[:, :-1], pos, neg), (users[:-1], seq, pos, neg),
                      (users, seq, pos[:, :-1], neg), (users, seq, pos, neg[:-1])):
        with pytest.raises(ValueError):
            eng.train_single_batch(bad_batch)
    loss, _ = eng.backward_only(ce.batch_of(f))
    assert_scalar_close(loss, ce.reference("defaults")[0], what="loss after the errors")
    first = eng.train_single_batch(ce.batch_of(f))
    assert first == loss and not torch.equal(eng.model.flat, before), "the engine trains on"


@pytest.mark.parametrize("rng", ["device", "torch_cpu"])
def test_dropout_masks_have_the_stated_shape_and_rate(hip_device, rng):
    """One mask [B, n_v d + n_h L] per step: tile_edges_4097 holds 4097 x 7 = 28 679 bytes, so four standard deviations
    of the keep rate are 1.1e-2; two steps draw different masks; eval mode draws none."""
    f = ce.fixture("tile_edges_4097")
    p = 0.3
    eng = make_engine(dict(f, p=p), dropout_rng=rng, dropout_seed=5)
    torch.manual_seed(3)
    loss1 = eng.train_single_batch(ce.batch_of(f))
    first = [k.clone() for k in eng.last_keep_masks]
    loss2 = eng.train_single_batch(ce.batch_of(f))
    second = eng.last_keep_masks
    assert np.isfinite(loss1) and np.isfinite(loss2)
    n = f["B"] * (f["n_v"] * f["d"] + f["n_h"] * f["L"])
    assert eng._mask_shapes(f["B"]) == [(f["B"], f["n_v"] * f["d"] + f["n_h"] * f["L"])]
    assert len(first) == len(second) == 1
    sigma = np.sqrt(p * (1 - p) / n)
    for m in (first[0], second[0]):
        assert m.numel() == n and m.dtype == torch.uint8 and int(m.max()) == 1
        rate = float(m.float().mean())
        assert abs(rate - (1 - p)) <= 4 * sigma, f"keep rate {rate:.5f}"
    assert not torch.equal(first[0], second[0]), "two steps drew the same mask"
    if rng == "torch_cpu":
        torch.manual_seed(3)
        again = torch.empty(f["B"], n // f["B"]).bernoulli_(1 - p).to(torch.uint8).reshape(-1)
        assert torch.equal(again, first[0].cpu()), "the torch seed does not reproduce the mask"
    eng.model.eval()
    eng.backward_only(ce.batch_of(f))
    assert eng.last_keep_masks is None
    with pytest.raises(ValueError):
        bad = make_engine(dict(f, p=p), dropout_rng="numpy")
        bad.train_single_batch(ce.batch_of(f))


def test_train_an_epoch_runs_the_sampler_once_through(hip_device):
    """Every batch of a ``WindowSampler`` epoch, the ragged last one included: the mean loss is that of the same steps
    taken one by one, and the weights agree outside the atomically accumulated tables."""
    import beta_recsys_amd as hp

    f = ce.fixture("defaults")
    rng = np.random.default_rng(2)
    user_train = {u: (rng.permutation(f["I"])[:rng.integers(2, 20)] + 1).tolist() for u in range(f["U"])}

    def sampler():
        return hp.data.WindowSampler(user_train, f["U"], f["I"], 16, f["L"], f["T"], f["N"], seed=6)

    eng = make_engine(f, optimizer="sgd", lr=0.05)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        mean = eng.train_an_epoch(sampler(), 4)
    other = make_engine(f, optimizer="sgd", lr=0.05)
    batches = list(sampler())
    assert len(batches) == len(sampler()) and len(batches[-1][0]) < 16 and len(batches) > 2
    losses = [other.train_single_batch(b) for b in batches]
    assert_scalar_close(mean, float(np.mean(losses)), what="mean epoch loss")
    tag, total, epoch_id = eng.writer.scalars[-1]
    assert (tag, epoch_id) == ("model/loss", 4) and total == mean
    wa, wb = get_weights(eng), get_weights(other)
    for k in wa:
        assert_tensor_close(wa[k], wb[k], 1e-6, f"{k} after the epoch")
