"""FMLP-Rec on the GPU against the plain-torch restatement ``fmlprec_torch`` in float64: loss, ``f`` and every gradient at
the tile edges of csrc/fmlprec.hip, the filter stage alone against ``torch.fft``, given dropout masks, no-label batches,
run-to-run bits, chained Adam steps, ``predict`` / ``recommend_next``, the limits."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import fmlprec_torch as ft
import topk_reference as tk
from helpers import (assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_tensor_close,
                     oracle_trajectory)
from srgnn_torch import adam_step, new_adam_state

pytestmark = pytest.mark.gpu


def make_engine(cfg, w, **model_kw):
    import beta_recsys_amd as hp

    model = {**cfg, "device_str": "cuda:0", "optimizer": "adam", "lr": 1e-3, **model_kw}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.FMLPRecEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    eng.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return eng


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's fixture with its float64 and float32 restatement results, computed once."""
    cfg, w, batch = ft.make(case)
    return cfg, w, batch, ft.grads(w, cfg, batch, torch.float64), ft.grads(w, cfg, batch, torch.float32)


@pytest.mark.parametrize("case", sorted(ft.CASES))
def test_loss_feats_and_gradients_match_float64(hip_device, case):
    cfg, w, batch, (l64, g64, f64, _), (l32, g32, _, _) = reference(case)
    eng = make_engine(cfg, w)
    loss, grads = eng.backward_only(batch)
    print(case, "loss", loss, l64, "fp32 restatement", l32)
    assert_scalar_close(loss, l64, what=f"{case} loss")
    assert_tensor_close(eng.model.feats(batch[1]).cpu().numpy(), f64, what=f"{case} f")
    assert_grads_as_accurate(grads, g32, g64, what=case)
    assert float(grads["item_emb.weight"][0].abs().max()) == 0.0, "row 0 received a gradient"


@pytest.mark.parametrize("case", sorted(ft.CASES))
def test_filter_stage_matches_torch_fft(hip_device, case):
    """``hiprec_fmlprec_filter`` alone at the case's (T, D, B): y, dx and dW against ``torch.fft`` and its autograd in
    float64; the imaginary gradient of the DC bin and (T even) of the Nyquist bin is exactly 0."""
    from beta_recsys_amd.fmlprec import filter_stage

    c = ft.CASES[case]
    T, D, B = c["T"], c["D"], c["B"]
    gen = torch.Generator().manual_seed(T * 1000 + D)
    x = torch.randn(B, T, D, generator=gen, dtype=torch.float64, requires_grad=True)
    wt = (0.3 * torch.randn(T // 2 + 1, D, 2, generator=gen, dtype=torch.float64)).requires_grad_()
    dy = torch.randn(B, T, D, generator=gen, dtype=torch.float64)
    y64 = ft.filter_layer(x, wt)
    dx64, dw64 = torch.autograd.grad(y64, (x, wt), dy)
    y, dx, dw = (t.cpu().numpy() for t in filter_stage(x.detach().float().cuda(), wt.detach().float().cuda(),
                                                       dy=dy.float().cuda()))
    for name, got, ref in (("y", y, y64.detach()), ("dx", dx, dx64), ("dW", dw, dw64)):
        print(case, name, float(np.abs(got - ref.numpy()).max() / ref.abs().max()))
        assert_tensor_close(got, ref.numpy(), what=f"{case} filter {name}")
    assert np.abs(dw[0, :, 1]).max() == 0.0, "imaginary gradient at DC"
    if T % 2 == 0:
        assert np.abs(dw[T // 2, :, 1]).max() == 0.0, "imaginary gradient at Nyquist"


def test_given_keep_masks_at_half_dropout(hip_device):
    cfg, w, batch = ft.make("tile_plus_one")
    B, T, D = batch[1].shape + (cfg["emb_dim"],)
    rng = np.random.default_rng(3)
    keep = [rng.integers(0, 2, (B * T, D)).astype(np.uint8) for _ in range(1 + 2 * cfg["num_blocks"])]
    (l64, g64, _, _), (_, g32, _, _) = (ft.grads(w, cfg, batch, dt, keep, 2.0) for dt in (torch.float64, torch.float32))
    eng = make_engine(cfg, w, dropout_rate=0.5)
    loss, grads = eng.backward_only(batch, keep_masks=keep)
    assert_scalar_close(loss, l64, what="loss with dropout")
    assert_grads_as_accurate(grads, g32, g64, what="dropout")


def test_no_label_batch_gives_zero_loss_and_gradient(hip_device):
    cfg, w, (u, seq, pos, neg) = ft.make("odd_below_tile")
    eng = make_engine(cfg, w)
    eng._enqueue_grad((u, seq, np.zeros_like(pos), neg))
    torch.cuda.synchronize()
    assert float(eng._g_flat.abs().max()) == 0.0
    loss, _ = eng.backward_only((u, seq, np.zeros_like(pos), neg))
    assert loss == 0.0


def test_gradients_are_bit_reproducible(hip_device):
    cfg, w, batch = ft.make("dw_seams")
    eng = make_engine(cfg, w)
    (la, ga), (lb, gb) = eng.backward_only(batch), eng.backward_only(batch)
    assert la == lb
    for k in w:
        if k != "item_emb.weight":
            assert float(ga[k].abs().max()) > 0 and torch.equal(ga[k], gb[k]), k


def test_three_chained_adam_steps(hip_device):
    cfg, w, batch = ft.make("tile_exact")
    lr = 1e-3
    batches = [batch, (batch[0], batch[1][::-1].copy(), batch[2][::-1].copy(), batch[3]), batch]
    eng = make_engine(cfg, w, lr=lr)
    for b in batches:
        eng.train_single_batch(b)

    def grad_fn(wk, b):
        return {k: v.astype(np.float32) for k, v in ft.grads(wk, cfg, b, torch.float32)[1].items()}

    w_ref, env, upd = oracle_trajectory(w, batches, grad_fn, lambda wk, g, s: adam_step(wk, g, s, lr, 0.0), new_adam_state)
    got = {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}
    assert_on_trajectory(got, w_ref, env, upd, "adam trajectory")


def test_predict_and_recommend_next(hip_device):
    cfg, w, batch, (_, _, _, s64), _ = reference("default_len")
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


def test_limits_and_bad_ids(hip_device):
    import beta_recsys_amd as hp

    cfg, w, batch, (l64, _, _, _), _ = reference("odd_below_tile")
    for kw in (dict(emb_dim=24), dict(emb_dim=144), dict(maxlen=0), dict(maxlen=257), dict(num_blocks=0),
               dict(num_blocks=17), dict(ffn_dim=24)):
        with pytest.raises(ValueError):
            hp.FMLPRec(dict(cfg, **kw))
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
