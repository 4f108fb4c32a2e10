"""SR-GNN on the GPU beyond single gradients: chained Adam steps with weight decay, the epoch over a ``SessionLoader`` and
its StepLR, ``forward`` / ``predict`` / ``recommend`` / ``recommend_next``, the bounds checks."""
import contextlib
import io

import numpy as np
import pytest
import torch

import srgnn_edges as se
import srgnn_torch as st
import topk_reference as tk
from helpers import REL, assert_on_trajectory, assert_scalar_close, assert_tensor_close, oracle_trajectory
from test_srgnn_edges_gpu import make_engine

pytestmark = pytest.mark.gpu


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def three_batches(f):
    """The fixture's own batch and two more of other shapes over the same catalogue."""
    rng = np.random.default_rng(23)
    out = [se.batch_of(f)]
    for B, T in ((5, 6), (9, 4)):
        lens = rng.integers(1, T + 1, B)
        lens[0] = T
        sessions = [rng.integers(1, 8, k).tolist() for k in lens]
        seq, lens = se._pad(sessions, T)
        out.append((seq, rng.integers(1, f["n_node"], B), lens))
    return out


def test_three_chained_adam_steps_with_weight_decay(hip_device):
    """``torch.optim.Adam(weight_decay=l2)`` on the restatement's gradients: every element inside the envelope of the
    restatement's own perturbed-gradient runs.  Zero outliers."""
    f = se.fixture("defaults")
    cfg, lr, l2 = se.cfg_of(f), 1e-3, 1e-2
    batches = three_batches(f)
    eng = make_engine(f, lr=lr, l2=l2)
    for k, b in enumerate(batches):
        loss = eng.train_single_batch(b)
        if k == 0:
            assert_scalar_close(loss, se.reference("defaults")[0], what="loss of step 0 (without the l2 term)")

    def grad_fn(w, b):
        return {k: v.astype(np.float32) for k, v in st.grads(w, cfg, b, torch.float32)[1].items()}

    w_ref, env, upd = oracle_trajectory(f["w"], batches, grad_fn, lambda w, g, s: st.adam_step(w, g, s, lr, l2),
                                        st.new_adam_state)
    assert float(np.abs(w_ref["embedding.weight"][0] - f["w"]["embedding.weight"][0]).max()) > 0, "l2 reaches row 0"
    assert_on_trajectory(get_weights(eng), w_ref, env, upd, "adam trajectory")


def test_weight_decay_is_in_the_gradient_and_not_in_the_loss(hip_device):
    f = se.fixture("revisits")
    l64, g64 = se.reference("revisits")[:2]
    eng = make_engine(f, l2=0.5)
    loss, grads = eng.backward_only(se.batch_of(f))
    assert_scalar_close(loss, l64, what="loss")
    for k, g in grads.items():
        assert_tensor_close(g.cpu().numpy(), g64[k] + 0.5 * f["w"][k].astype(np.float64), what=f"grad {k} with l2")


def test_an_epoch_returns_the_mean_loss_and_follows_steplr(hip_device):
    import beta_recsys_amd as hp

    f = se.fixture("step_2")
    rng = np.random.default_rng(3)
    sequences = [rng.integers(1, f["n_node"], rng.integers(2, 7)).tolist() for _ in range(9)]
    out_seqs, labels = hp.data.session_prefixes(sequences)

    def loader():
        return hp.data.SessionLoader(out_seqs, labels, 6, shuffle=True, seed=5)

    eng = make_engine(f, optimizer="sgd", lr=0.05, lr_dc_step=3, lr_dc=0.1)
    with contextlib.redirect_stdout(io.StringIO()):
        mean = eng.train_an_epoch(loader(), 4)
    assert eng.optimizer.lr == eng.epoch_lr(4) == 0.05 * 0.1 and eng.epoch_lr(2) == 0.05 and eng.epoch_lr(6) == 0.05 * 0.1 ** 2
    other = make_engine(f, optimizer="sgd", lr=0.05 * 0.1)
    steps = list(loader())
    assert len(steps) >= 3
    losses = [other.train_single_batch(s) for s in steps]
    assert_scalar_close(mean, float(np.mean(losses)), what="mean epoch loss")
    tag, total, epoch_id = eng.writer.scalars[-1]
    assert (tag, epoch_id) == ("model/loss", 4) and total == mean
    wa, wb = get_weights(eng), get_weights(other)
    for k in wa:
        assert_tensor_close(wa[k], wb[k], 1e-6, f"{k} after the epoch")


def test_forward_predict_and_recommend_next(hip_device):
    f = se.fixture("len_one_mixed")
    I, cfg = f["n_node"] - 1, se.cfg_of(f)
    eng = make_engine(f)
    eng.model.eval()
    s64 = se.reference("len_one_mixed")[3]
    scores = eng.model.forward(f["seq"], f["lens"])
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (f["B"], I)
    assert_tensor_close(scores.cpu().numpy(), s64, what="forward")
    profiles = [s[:] for s in f["sessions"]]
    gaps = -np.diff(-np.sort(-s64, axis=1), axis=1)
    assert gaps.min() > 4 * REL * np.abs(s64).max(), "the fixture separates its scores"
    for r in (0, 1):
        got = eng.predict(profiles[r])
        want = np.exp(s64[r] - s64[r].max())
        assert got.shape == (I,) and got.dtype == np.float32
        assert_tensor_close(got, want / want.sum(), what=f"predict profile {r}")
    rec = eng.recommend(profiles[1])
    assert [r[0][0] for r in rec] == (np.argsort(-s64[1], kind="stable") + 1).tolist() and len(rec) == I
    k = 5
    items, top = eng.recommend_next(profiles, k)
    items, top = items.cpu().numpy(), top.cpu().numpy()
    assert items.shape == (f["B"], k) and (items >= 1).all() and (items <= I).all(), "the padding id was returned"
    tk.check_against_float64(items - 1, top, s64, None, "recommend_next")
    assert np.array_equal(items - 1, tk.exact_topk(s64, None, k)[0]), "not the brute-force ranking"
    # the (padded, lengths) form gives the same
    items_p, top_p = eng.recommend_next((np.ascontiguousarray(f["seq"].T), f["lens"]), k)
    assert np.array_equal(items_p.cpu().numpy(), items) and np.array_equal(top_p.cpu().numpy(), top)
    rows = np.concatenate([np.full(len(p), r) for r, p in enumerate(profiles)] + [[0]])
    seen_items = np.concatenate(profiles + [[0]])      # a 0 entry is ignored
    items_s, top_s = eng.recommend_next(profiles, k, seen=(rows, seen_items))
    items_s = items_s.cpu().numpy()
    seen = [np.unique(p) - 1 for p in profiles]
    tk.check_against_float64(items_s - 1, top_s.cpu().numpy(), s64, seen, "recommend_next with seen")
    assert np.array_equal(items_s - 1, tk.exact_topk(s64, seen, k)[0])
    for r, p in enumerate(profiles):
        assert not set(items_s[r].tolist()) & (set(p) | {0})
    many, many_s = eng.recommend_next(profiles[:1], I + 3, seen=(np.zeros(1, dtype=np.int64), np.array(profiles[0])))
    many = many.cpu().numpy()[0]
    left = I - len(set(profiles[0]))
    assert sorted(many[:left].tolist()) == sorted(set(range(1, I + 1)) - set(profiles[0])) and (many[left:] == -1).all()
    assert np.isneginf(many_s.cpu().numpy()[0, left:]).all()
    with pytest.raises(ValueError):
        eng.recommend_next([[1, 2], []], 3)
    with pytest.raises(ValueError):
        eng.recommend_next([[1, 0, 2]], 3)


def test_bad_batches_raise_and_leave_the_engine_usable(hip_device):
    import beta_recsys_amd as hp

    f = se.fixture("defaults")
    n_node = f["n_node"]
    eng = make_engine(f)
    before = eng.model.flat.clone()
    seq, target, lens = se.batch_of(f)
    inside = np.argwhere(np.arange(f["T"])[:, None] < lens[None, :])
    t0, b0 = inside[len(inside) // 2]
    zero_inside = seq.copy()
    zero_inside[t0, b0] = 0
    for bad in ((zero_inside, target, lens),
                (seq, np.where(np.arange(f["B"]) == 2, 0, target), lens),
                (seq, np.where(np.arange(f["B"]) == 2, n_node, target), lens),
                (seq, target[:-1], lens), (seq, target, lens[:-1]), (seq, target),
                (np.ones((se.LIMITS["len"] + 1, 1), dtype=np.int64), [1], [se.LIMITS["len"] + 1]),
                (np.ones((1, se.LIMITS["batch"] + 1), dtype=np.int64), np.ones(se.LIMITS["batch"] + 1, dtype=np.int64),
                 np.ones(se.LIMITS["batch"] + 1, dtype=np.int64))):
        with pytest.raises(ValueError):
            eng.backward_only(bad)
        assert float(eng._g_flat.abs().max()) == 0.0
    # an id beyond the table is found on the device
    for value in (n_node, n_node + 7, -2):
        far = seq.copy()
        far[t0, b0] = value
        with pytest.raises(IndexError):
            eng.backward_only((far, target, lens))
        assert torch.equal(eng.model.flat, before) and float(eng._g_flat.abs().max()) == 0.0, "a partial step was kept"
        with pytest.raises(IndexError):
            eng.model.query(far, lens)
    for kw in (dict(hidden_size=se.LIMITS["hidden"] + 1), dict(step=se.LIMITS["step"] + 1)):
        with pytest.raises(ValueError):
            hp.SRGNN({"model": kw, "dataset": {"n_node": n_node}})
    loss, _ = eng.backward_only(se.batch_of(f))
    assert_scalar_close(loss, se.reference("defaults")[0], what="loss after the errors")
    first = eng.train_single_batch(se.batch_of(f))
    assert first == loss and not torch.equal(eng.model.flat, before), "the engine trains on"
