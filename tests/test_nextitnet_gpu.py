"""NextItNet on the GPU against the plain-torch restatement ``nextitnet_torch`` in float64: loss, ``f`` and every gradient
at the tile edges of csrc/nextitnet.hip, the sequence boundary of the shifts, row 0 and no-label batches, run-to-run
bits, chained Adam steps with ``l2``, ``predict`` / ``recommend_next``, the limits."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import nextitnet_torch as nt
import topk_reference as tk
from helpers import (REL, assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_tensor_close,
                     oracle_trajectory)
from srgnn_torch import adam_step, new_adam_state

pytestmark = pytest.mark.gpu


def make_engine(cfg, w, **model_kw):
    import beta_recsys_amd as hp

    model = {**cfg, "device_str": "cuda:0", "optimizer": "adam", "lr": 1e-3, **model_kw}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.NextItNetEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    eng.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return eng


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's fixture with its float64 and float32 restatement results, computed once."""
    cfg, w, batch = nt.make(case)
    return cfg, w, batch, nt.grads(w, cfg, batch, torch.float64), nt.grads(w, cfg, batch, torch.float32)


@pytest.mark.parametrize("case", sorted(nt.CASES))
def test_loss_feats_and_gradients_match_float64(hip_device, case):
    cfg, w, batch, (l64, g64, f64, _), (l32, g32, _, _) = reference(case)
    eng = make_engine(cfg, w)
    loss, grads = eng.backward_only(batch)
    print(case, "loss", loss, l64, "fp32 restatement", l32)
    assert_scalar_close(loss, l64, what=f"{case} loss")
    assert_tensor_close(eng.model.feats(batch[1]).cpu().numpy(), f64, what=f"{case} f at the last position")
    assert_grads_as_accurate(grads, g32, g64, what=case)
    assert float(grads["item_emb.weight"][0].abs().max()) == 0.0, "row 0 received a gradient"


def test_shifts_stay_inside_a_sequence(hip_device):
    """B = 2, T = 12, taps 8 and 16 rows back (a row of the flattened [B T, D] array that far back is sequence 0's), only
    sequence 1 is labelled: changing sequence 0's items changes neither sequence 1's ``f`` nor any weight gradient
    (sequence 0's rows enter them with an exact zero) by a single bit."""
    cfg, w, _ = nt.make("reach_beyond_t")
    cfg = dict(cfg, loss_positions="all")
    rng = np.random.default_rng(5)
    T, I = cfg["maxlen"], cfg["n_items"]
    seq, other = rng.integers(1, I + 1, (2, T)), rng.integers(1, I + 1, (2, T))
    other[1] = seq[1]
    pos = np.stack([np.zeros(T, dtype=np.int64), rng.integers(1, I + 1, T)])
    eng = make_engine(cfg, w)
    out = []
    for s in (seq, other):
        _, g = eng.backward_only((None, s, pos, None))
        out.append((eng.model.feats(s).clone(), g))
    assert torch.equal(out[0][0][1], out[1][0][1]), "sequence 1's f depends on sequence 0"
    assert not torch.equal(out[0][0][0], out[1][0][0])
    for k in w:
        if k != "item_emb.weight":
            assert float(out[0][1][k].abs().max()) > 0 and torch.equal(out[0][1][k], out[1][1][k]), k


def test_no_label_batch_gives_zero_loss_and_gradient(hip_device):
    cfg, w, (u, seq, pos, neg) = nt.make("tile_minus_one_k2")
    eng = make_engine(cfg, w)
    eng._enqueue_grad((u, seq, np.zeros_like(pos), neg))
    torch.cuda.synchronize()
    assert float(eng._g_flat.abs().max()) == 0.0
    loss, _ = eng.backward_only((u, seq, np.zeros_like(pos), neg))
    assert loss == 0.0


def test_gradients_are_bit_reproducible(hip_device):
    cfg, w, batch = nt.make("slab_seam_and_splits")
    eng = make_engine(cfg, w)
    (la, ga), (lb, gb) = eng.backward_only(batch), eng.backward_only(batch)
    assert la == lb
    for k in w:
        if k != "item_emb.weight":
            assert torch.equal(ga[k], gb[k]), k


def test_three_chained_adam_steps_with_l2(hip_device):
    cfg, w, batch = nt.make("tile_plus_one_d128")
    lr, l2 = 1e-3, 1e-2
    batches = [batch, (batch[0], batch[1][::-1].copy(), batch[2][::-1].copy(), batch[3]), batch]
    eng = make_engine(cfg, w, lr=lr, l2=l2)
    for b in batches:
        eng.train_single_batch(b)

    def grad_fn(wk, b):
        return {k: v.astype(np.float32) for k, v in nt.grads(wk, cfg, b, torch.float32)[1].items()}

    w_ref, env, upd = oracle_trajectory(w, batches, grad_fn, lambda wk, g, s: adam_step(wk, g, s, lr, l2), new_adam_state)
    got = {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}
    assert_on_trajectory(got, w_ref, env, upd, "adam trajectory")


def test_predict_and_recommend_next(hip_device):
    cfg, w, batch, (_, _, _, s64), _ = reference("tile_minus_one_k2")
    I, seq = cfg["n_items"], batch[1]
    eng = make_engine(cfg, w)
    cand = np.array([3, 1, I, 7])
    assert_tensor_close(eng.predict(seq, cand).cpu().numpy(), s64[:, cand - 1], what="predict")
    k = 5
    items, top = (t.cpu().numpy() for t in eng.recommend_next(seq, k))
    assert items.shape == (seq.shape[0], k) and (items >= 1).all() and (items <= I).all(), "the padding id was returned"
    tk.check_against_float64(items - 1, top, s64, None, "recommend_next")
    rows = np.concatenate([np.repeat(np.arange(seq.shape[0]), k), [0]])
    seen_items = np.concatenate([items.reshape(-1), [0]])      # a 0 entry is ignored
    items_s, top_s = (t.cpu().numpy() for t in eng.recommend_next(seq, k, seen=(rows, seen_items)))
    tk.check_against_float64(items_s - 1, top_s, s64, [r - 1 for r in items], "recommend_next with seen")
    assert (items_s >= 1).all() and not any(set(a) & set(b) for a, b in zip(items_s.tolist(), items.tolist()))


def test_limits_and_bad_ids(hip_device):
    import beta_recsys_amd as hp

    cfg, w, batch, (l64, _, _, _), _ = reference("reach_beyond_t")
    for kw in (dict(emb_dim=24), dict(emb_dim=144), dict(maxlen=257), dict(kernel_size=5), dict(kernel_size=0),
               dict(dilations=[1], block_num=17), dict(dilations=[0]), dict(loss_positions="first")):
        with pytest.raises(ValueError):
            hp.NextItNet({"model": dict(cfg, **kw)})
    eng = make_engine(cfg, w)
    before = eng.model.flat.clone()
    u, seq, pos, neg = batch
    long = np.ones((1, cfg["maxlen"] + 1), dtype=np.int64)
    for bad in ((u, long, long, long), (u, seq, pos[:, :-1], neg), (u, seq, pos)):
        with pytest.raises(ValueError):
            eng.backward_only(bad)
    with pytest.raises(ValueError):
        eng.model.workspace(eng._setup(), 2 ** 24 // cfg["maxlen"] + 1, cfg["maxlen"])
    for value in (cfg["n_items"] + 1, -2):
        far_seq, far_pos = seq.copy(), pos.copy()
        far_seq[0, -1], far_pos[2, -1] = value, value
        for bad in ((u, far_seq, pos, neg), (u, seq, far_pos, neg)):
            with pytest.raises(IndexError):
                eng.backward_only(bad)
            assert torch.equal(eng.model.flat, before) and float(eng._g_flat.abs().max()) == 0.0, "a partial step was kept"
        with pytest.raises(IndexError):
            eng.model.feats(far_seq)
    loss = eng.train_single_batch(batch)
    assert_scalar_close(loss, l64, what="loss after the errors")
    assert not torch.equal(eng.model.flat, before), "the engine trains on"
