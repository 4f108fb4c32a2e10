"""Mamba4Rec on the GPU against the plain-torch restatement ``mamba4rec_torch`` in float64: loss, ``f`` and every gradient at
the lane, slab and chunk edges of csrc/mamba4rec.hip, the selective scan alone against the float64 loop, left padding, given
dropout masks, no-label batches, run-to-run bits, chained Adam steps, ``predict`` / ``recommend_next``, the limits."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import mamba4rec_torch as mt
import topk_reference as tk
from helpers import (assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_tensor_close,
                     oracle_trajectory)
from srgnn_torch import adam_step, new_adam_state

pytestmark = pytest.mark.gpu


def make_engine(cfg, w, **model_kw):
    import beta_recsys_amd as hp

    model = {**cfg, "device_str": "cuda:0", "optimizer": "adam", "lr": 1e-3, **model_kw}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.Mamba4RecEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    eng.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return eng


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's fixture with its float64 and float32 restatement results, computed once."""
    cfg, w, batch = mt.make(case)
    return cfg, w, batch, mt.grads(w, cfg, batch, torch.float64), mt.grads(w, cfg, batch, torch.float32)


@pytest.mark.parametrize("case", sorted(mt.CASES))
def test_loss_feats_and_gradients_match_float64(hip_device, case):
    cfg, w, batch, (l64, g64, f64, _), (l32, g32, _, _) = reference(case)
    eng = make_engine(cfg, w)
    loss, grads = eng.backward_only(batch)
    print(case, "loss", loss, l64, "fp32 restatement", l32)
    assert_scalar_close(loss, l64, what=f"{case} loss")
    assert_tensor_close(eng.model.feats(batch[1]).cpu().numpy(), f64, what=f"{case} f")
    assert_grads_as_accurate(grads, g32, g64, what=case)
    assert float(grads["item_emb.weight"][0].abs().max()) == 0.0, "row 0 received a gradient"


@pytest.mark.parametrize("case", sorted(mt.CASES))
def test_selective_scan_matches_the_float64_loop(hip_device, case):
    """``hiprec_mamba4rec_scan`` alone at the case's (B, T, d_inner, N) with random start slots (0 and T - 1 among them):
    ``out`` and all seven gradients against the loop and its autograd in float64."""
    from beta_recsys_amd import selective_scan

    c = mt.CASES[case]
    T, Di, N, B = c["T"], c["expand"] * c["D"], c["N"], c["B"]
    gen = torch.Generator().manual_seed(T * 1000 + Di)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)      # noqa: E731
    u, dt_pre, z, Bm, Cm, dout = rnd(B, T, Di), rnd(B, T, Di) * 2 - 2, rnd(B, T, Di), rnd(B, T, N), rnd(B, T, N), rnd(B, T, Di)
    A, Dp = -torch.exp(torch.rand(Di, N, generator=gen, dtype=torch.float64) * 3 - 1), rnd(Di)
    start = torch.randint(0, T, (B,), generator=gen)
    start[0], start[1] = 0, T - 1
    m = (torch.arange(T)[None] >= start[:, None]).double()
    ins = [t.requires_grad_() for t in (u, dt_pre, z, A, Bm, Cm, Dp)]
    out64 = mt.selective_scan(*ins, m)
    ref = [out64.detach()] + list(torch.autograd.grad(out64, ins, dout))
    got = selective_scan(*(t.detach().float().cuda() for t in ins), start.cuda(), dout=dout.float().cuda())
    for name, g, r in zip(("out", "du", "ddt", "dz", "dA", "dBm", "dCm", "dD"), got, ref):
        print(case, name, "max err", float((g.cpu().double() - r).abs().max()), "scale", float(r.abs().max()))
        assert_tensor_close(g.cpu().numpy(), r.numpy(), what=f"{case} scan {name}")


def test_left_padding_is_exact_and_matches_the_unpadded_sequence(hip_device):
    cfg, w, batch, _, _ = reference("default")
    eng, T = make_engine(cfg, w), cfg["maxlen"]
    short = batch[1][:3, -7:]
    f = eng.model.feats(short)
    assert torch.equal(f, eng.model.feats(np.pad(short, ((0, 0), (T - 7, 0)))))
    f64 = mt.grads(w, dict(cfg, maxlen=7), (None, short, np.ones(3, dtype=np.int64), np.ones(3, dtype=np.int64)))[2]
    assert_tensor_close(f.cpu().numpy(), f64, what="f of a left-padded row against the unpadded restatement")


def test_given_keep_masks_at_half_dropout(hip_device):
    cfg, w, batch = mt.make("lanes_plus_one")
    B, T, D = batch[1].shape + (cfg["emb_dim"],)
    rng = np.random.default_rng(3)
    keep = [rng.integers(0, 2, (B * T, D)).astype(np.uint8)]
    for _ in range(cfg["num_blocks"]):
        keep += [rng.integers(0, 2, (B * T, n)).astype(np.uint8) for n in (D, 4 * D, D)]
    (l64, g64, _, _), (_, g32, _, _) = (mt.grads(w, cfg, batch, dt, keep, 2.0) for dt in (torch.float64, torch.float32))
    eng = make_engine(cfg, w, dropout_rate=0.5)
    loss, grads = eng.backward_only(batch, keep_masks=keep)
    assert_scalar_close(loss, l64, what="loss with dropout")
    assert_grads_as_accurate(grads, g32, g64, what="dropout")


def test_no_label_batch_gives_zero_loss_and_gradient(hip_device):
    cfg, w, (u, seq, pos, neg) = mt.make("below_conv")
    eng = make_engine(cfg, w)
    eng._enqueue_grad((u, seq, np.zeros_like(pos), neg))
    torch.cuda.synchronize()
    assert float(eng._g_flat.abs().max()) == 0.0
    loss, _ = eng.backward_only((u, seq, np.zeros_like(pos), neg))
    assert loss == 0.0


def test_gradients_are_bit_reproducible(hip_device):
    cfg, w, batch = mt.make("batch_seams")
    eng = make_engine(cfg, w)
    (la, ga), (lb, gb) = eng.backward_only(batch), eng.backward_only(batch)
    assert la == lb
    for k in w:
        if k != "item_emb.weight":
            assert float(ga[k].abs().max()) > 0 and torch.equal(ga[k], gb[k]), k


def test_three_chained_adam_steps(hip_device):
    cfg, w, batch = mt.make("lanes_exact")
    lr = 1e-3
    batches = [batch, (batch[0], batch[1][::-1].copy(), batch[2][::-1].copy(), batch[3]), batch]
    eng = make_engine(cfg, w, lr=lr)
    for b in batches:
        eng.train_single_batch(b)

    def grad_fn(wk, b):
        return {k: v.astype(np.float32) for k, v in mt.grads(wk, cfg, b, torch.float32)[1].items()}

    w_ref, env, upd = oracle_trajectory(w, batches, grad_fn, lambda wk, g, s: adam_step(wk, g, s, lr, 0.0), new_adam_state)
    got = {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}
    assert_on_trajectory(got, w_ref, env, upd, "adam trajectory")


def test_predict_and_recommend_next(hip_device):
    cfg, w, batch, (_, _, _, s64), _ = reference("default")
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

    cfg, w, batch, (l64, _, _, _), _ = reference("below_conv")
    for kw in (dict(emb_dim=24), dict(emb_dim=144), dict(expand=3), dict(d_state=0), dict(d_state=65), dict(d_conv=1),
               dict(d_conv=5), dict(dt_rank=0), dict(dt_rank=33), dict(maxlen=0), dict(maxlen=257), dict(num_blocks=0),
               dict(num_blocks=17), dict(ffn_dim=24), dict(ffn_dim=528)):
        with pytest.raises(ValueError):
            hp.Mamba4Rec(dict(cfg, **kw))
    eng = make_engine(cfg, w)
    before = eng.model.flat.clone()
    u, seq, pos, neg = batch
    long = np.ones((len(u), cfg["maxlen"] + 1), dtype=np.int64)
    for bad in ((u, long, pos, neg), (u, seq, pos[:-1], neg), (u, seq, np.stack([pos, pos], 1), neg), (u, seq, pos)):
        with pytest.raises(ValueError):
            eng.backward_only(bad)
    for value in (cfg["n_items"] + 1, -2):
        far_seq, far_pos, far_neg = seq.copy(), pos.copy(), neg.copy()
        far_seq[0, -1], far_pos[2], far_neg[0] = value, value, value
        for bad in ((u, far_seq, pos, neg), (u, seq, far_pos, neg), (u, seq, pos, far_neg)):
            with pytest.raises(IndexError):
                eng.backward_only(bad)
            assert torch.equal(eng.model.flat, before) and float(eng._g_flat.abs().max()) == 0.0, "a partial step was kept"
        with pytest.raises(IndexError):
            eng.model.feats(far_seq)
    loss = eng.train_single_batch(batch)
    assert_scalar_close(loss, l64, what="loss after the errors")
    assert not torch.equal(eng.model.flat, before), "the engine trains on"
