"""HSTU on the GPU against the plain-torch restatement ``hstu_torch`` in float64: loss, ``f`` and every gradient at the tile
edges of csrc/hstu.hip, the attention stage alone, the time buckets bit for bit, given dropout masks, no-label batches,
run-to-run bits, chained Adam steps, ``predict`` / ``recommend_next``, the limits."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import hstu_torch as ht
import topk_reference as tk
from helpers import (assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_tensor_close,
                     oracle_trajectory)
from srgnn_torch import adam_step, new_adam_state

pytestmark = pytest.mark.gpu


def make_engine(cfg, w, **model_kw):
    import beta_recsys_amd as hp

    model = {**cfg, "device_str": "cuda:0", "optimizer": "adam", "lr": 1e-3, **model_kw}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.HSTUEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    eng.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return eng


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's fixture with its float64 and float32 restatement results, computed once."""
    cfg, w, batch = ht.make(case)
    return cfg, w, batch, ht.grads(w, cfg, batch, torch.float64), ht.grads(w, cfg, batch, torch.float32)


def times_of(batch):
    return batch[2] if len(batch) == 5 else None


@pytest.mark.parametrize("case", sorted(ht.CASES))
def test_loss_feats_and_gradients_match_float64(hip_device, case):
    cfg, w, batch, (l64, g64, f64, _), (l32, g32, _, _) = reference(case)
    eng = make_engine(cfg, w)
    loss, grads = eng.backward_only(batch)
    print(case, "loss", loss, l64, "fp32 restatement", l32)
    assert_scalar_close(loss, l64, what=f"{case} loss")
    assert_tensor_close(eng.model.all_feats(batch[1], times_of(batch)).cpu().numpy(), f64, what=f"{case} f")
    assert_grads_as_accurate(grads, g32, g64, what=case)
    assert float(grads["item_emb.weight"][0].abs().max()) == 0.0, "row 0 received a gradient"


@pytest.mark.parametrize("case", sorted({**ht.CASES, **ht.STAGE_ONLY}))
def test_attention_stage_matches_float64(hip_device, case):
    """``hiprec_hstu_attention`` alone at the case's own (B, T, H, dqk, dv) with N = maxlen: AV, dQ, dK, dV, d pos_w and
    d ts_w against ``hstu_torch.attention`` and its autograd in float64; what no pair reaches is exactly 0."""
    from beta_recsys_amd.hstu import attention_stage, bucket_bytes

    cfg, _, batch = ht.make(case)
    H, dq, dv, N, nbk = cfg["num_heads"], cfg["attention_dim"], cfg["linear_dim"], cfg["maxlen"], cfg["num_buckets"]
    seq = torch.as_tensor(batch[1])
    B, T = seq.shape
    timed = cfg["rel_bias"] == "pos_time"
    gen = torch.Generator().manual_seed(T * 1000 + H)
    rand = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)      # noqa: E731
    act = torch.nn.functional.silu(rand(B, T, 2 * H * (dq + dv))).requires_grad_()
    pos_w = (0.5 * rand(2 * N - 1)).requires_grad_()
    ts_w = (0.5 * rand(nbk + 1)).requires_grad_() if timed else None
    bkt = ht.buckets(torch.as_tensor(batch[2]), nbk) if timed else None
    dav = rand(B, T, H * dv)
    av64 = ht.attention(act, pos_w, ts_w, seq, bkt, H, dq, dv, N)
    leaves = (act, pos_w, ts_w) if timed else (act, pos_w)
    g64 = torch.autograd.grad(av64, leaves, dav)
    _, dv64, dq64, dk64 = g64[0].split([H * dv, H * dv, H * dq, H * dq], -1)
    dev = lambda t: None if t is None else t.detach().float().cuda()      # noqa: E731
    bytes_ = bucket_bytes(batch[2], seq.cuda(), nbk) if timed else None
    av, dq_, dk_, dv_, dpos, dts = attention_stage(dev(act), dev(pos_w), dev(ts_w), seq.cuda(), bytes_, H, dq, dv, N,
                                                   dav=dev(dav))
    pairs = [("AV", av, av64.detach()), ("dQ", dq_, dq64), ("dK", dk_, dk64), ("dV", dv_, dv64), ("dpos_w", dpos, g64[1])]
    if timed:
        pairs.append(("dts_w", dts, g64[2]))
    for name, got, ref in pairs:
        print(case, name, float(np.abs(got.cpu().numpy() - ref.numpy()).max() / max(float(ref.abs().max()), 1e-30)))
        assert_tensor_close(got.cpu().numpy(), ref.numpy(), what=f"{case} attention {name}")
    dpos = dpos.cpu().numpy()
    assert np.abs(dpos[N:]).max(initial=0.0) == 0.0 and np.abs(dpos[:N - T]).max(initial=0.0) == 0.0, "offsets no pair has"
    if timed:
        valid = seq != 0
        live = torch.tril(torch.ones(T, T, dtype=torch.bool))[None] & valid[:, :, None] & valid[:, None, :]
        unhit = np.setdiff1d(np.arange(nbk + 1), bkt[live].numpy())
        assert np.abs(dts.cpu().numpy()[unhit]).max(initial=0.0) == 0.0, "a bucket no pair hits received a gradient"


def test_bucket_bytes_are_exact_at_the_thresholds(hip_device):
    """Gaps of ``thr[k] - 1``, ``thr[k]``, ``thr[k] + 1`` around a few thresholds, the floor (gaps 0 and 1) and the clamp
    (buckets beyond ``num_buckets``): the bytes equal the float64 formula on every pair ``j <= i``."""
    from beta_recsys_amd.hstu import bucket_bytes, time_thresholds

    nbk = 32
    thr = time_thresholds(40)
    assert (np.diff(thr) >= 0).all() and thr[0] == 2
    gaps = np.concatenate([[0, 0, 1]] + [[thr[k - 1] - 1, thr[k - 1], thr[k - 1] + 1] for k in (1, 2, 3, 5, 10, 20, 32, 33, 40)])
    ts = np.stack([1_600_000_000 + np.cumsum(gaps), 5 + np.cumsum(gaps[::-1])])
    seq = torch.ones(ts.shape, dtype=torch.int64)
    got = bucket_bytes(ts, seq.cuda(), nbk).cpu().numpy()
    ref = ht.buckets(torch.as_tensor(ts), nbk).numpy()
    low = np.tril(np.ones(ts.shape[1:] * 2, dtype=bool))
    assert ref[:, low].max() == nbk and ref[:, low].min() == 0
    assert np.array_equal(got[:, low], ref[:, low])


def test_given_keep_masks_at_half_dropout(hip_device):
    cfg, w, batch = ht.make("tile_plus_one")
    B, T = batch[1].shape
    rng = np.random.default_rng(3)
    widths = [cfg["emb_dim"]] + [cfg["num_heads"] * cfg["linear_dim"]] * cfg["num_blocks"]
    keep = [rng.integers(0, 2, (B * T, n)).astype(np.uint8) for n in widths]
    (l64, g64, _, _), (_, g32, _, _) = (ht.grads(w, cfg, batch, dt, keep, 2.0) for dt in (torch.float64, torch.float32))
    eng = make_engine(cfg, w, dropout_rate=0.5)
    loss, grads = eng.backward_only(batch, keep_masks=keep)
    assert_scalar_close(loss, l64, what="loss with dropout")
    assert_grads_as_accurate(grads, g32, g64, what="dropout")


def test_no_label_batch_gives_zero_loss_and_gradient(hip_device):
    cfg, w, (u, seq, ts, pos, neg) = ht.make("below_tile")
    eng = make_engine(cfg, w, l2_emb=0.0)
    eng._enqueue_grad((u, seq, ts, np.zeros_like(pos), neg))
    torch.cuda.synchronize()
    assert float(eng._g_flat.abs().max()) == 0.0
    loss, _ = eng.backward_only((u, seq, ts, np.zeros_like(pos), neg))
    assert loss == 0.0


def test_gradients_are_bit_reproducible(hip_device):
    cfg, w, batch = ht.make("fold_seams")
    eng = make_engine(cfg, w)
    (la, ga), (lb, gb) = eng.backward_only(batch), eng.backward_only(batch)
    assert la == lb
    for k in w:
        if k != "item_emb.weight":
            assert float(ga[k].abs().max()) > 0 and torch.equal(ga[k], gb[k]), k


def test_three_chained_adam_steps(hip_device):
    cfg, w, batch = ht.make("tile_exact_dqk_ne_dv")
    lr = 1e-3
    flipped = (batch[0],) + tuple(a[::-1].copy() for a in batch[1:])
    batches = [batch, flipped, batch]
    eng = make_engine(cfg, w, lr=lr)
    for b in batches:
        eng.train_single_batch(b)

    def grad_fn(wk, b):
        return {k: v.astype(np.float32) for k, v in ht.grads(wk, cfg, b, torch.float32)[1].items()}

    w_ref, env, upd = oracle_trajectory(w, batches, grad_fn, lambda wk, g, s: adam_step(wk, g, s, lr, 0.0), new_adam_state)
    got = {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}
    assert_on_trajectory(got, w_ref, env, upd, "adam trajectory")


def test_predict_and_recommend_next(hip_device):
    cfg, w, batch, (_, _, _, s64), _ = reference("pos_only")
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
    # a shorter input is left-padded to maxlen: the same f as the padded sequence itself
    short = seq[1:2, -3:]
    assert torch.equal(eng.model.feats(short), eng.model.feats(np.pad(short, ((0, 0), (seq.shape[1] - 3, 0)))))
    # with the time term the stamps travel along
    cfg, w, batch, (_, _, _, s64), _ = reference("tile_plus_one")
    eng = make_engine(cfg, w)
    assert_tensor_close(eng.predict(batch[1], cand, time_seq=batch[2]).cpu().numpy(), s64[:, cand - 1], what="timed predict")
    items, top = (t.cpu().numpy() for t in eng.recommend_next(batch[1], k, time_seq=batch[2]))
    tk.check_against_float64(items - 1, top, s64, None, "timed recommend_next")


def test_limits_and_bad_ids(hip_device):
    import beta_recsys_amd as hp

    cfg, w, batch, (l64, _, _, _), _ = reference("below_tile")
    for kw in (dict(emb_dim=24), dict(emb_dim=144), dict(maxlen=0), dict(maxlen=257), dict(num_blocks=0),
               dict(num_blocks=17), dict(attention_dim=24), dict(linear_dim=128), dict(num_heads=0), dict(num_heads=16),
               dict(num_buckets=0), dict(num_buckets=256), dict(dropout_rate=1.0), dict(rel_bias="time")):
        with pytest.raises(ValueError):
            hp.HSTU(dict(cfg, **kw))
    with pytest.raises(ValueError):
        make_engine(cfg, w, dropout_rng="torch_cpu")
    eng = make_engine(cfg, w)
    before = eng.model.flat.clone()
    u, seq, ts, pos, neg = batch
    long = np.ones((len(u), cfg["maxlen"] + 1), dtype=np.int64)
    for bad in ((u, long, long, long, long), (u, seq, ts, pos[:-1], neg), (u, seq, ts[:, 1:], pos, neg), (u, seq, pos, neg)):
        with pytest.raises(ValueError):
            eng.backward_only(bad)
    with pytest.raises(ValueError):
        eng.model.feats(seq)                     # rel_bias pos_time needs the stamps
    for value in (cfg["n_items"] + 1, -2):
        far_seq, far_pos, far_neg = seq.copy(), pos.copy(), neg.copy()
        far_seq[0, -1], far_pos[0, 2], far_neg[0, 0] = value, value, value
        for bad in ((u, far_seq, ts, pos, neg), (u, seq, ts, far_pos, neg), (u, seq, ts, pos, far_neg)):
            with pytest.raises(IndexError):
                eng.backward_only(bad)
            assert torch.equal(eng.model.flat, before) and float(eng._g_flat.abs().max()) == 0.0, "a partial step was kept"
        with pytest.raises(IndexError):
            eng.model.feats(far_seq, ts)
    for stamp in (-1, 2**62):                    # outside [0, 2^62) at a valid position
        off = ts.copy()
        off[0, 5] = stamp
        with pytest.raises(IndexError):
            eng.backward_only((u, seq, off, pos, neg))
    assert torch.equal(eng.model.flat, before) and float(eng._g_flat.abs().max()) == 0.0, "a partial step was kept"
    loss = eng.train_single_batch(batch)
    assert_scalar_close(loss, l64, what="loss after the errors")
    assert not torch.equal(eng.model.flat, before), "the engine trains on"
