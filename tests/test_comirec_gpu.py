"""ComiRec-DR on the GPU against the plain-torch restatement ``comirec_torch`` in float64: loss, interests, ``k*`` and every
gradient at the tile, group and slab edges of csrc/comirec.hip, projection + routing alone against the float64 loop, left
padding, no-label batches, run-to-run bits, chained Adam steps, ``predict`` / ``recommend_next``, the limits."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import comirec_torch as ct
import topk_reference as tk
from helpers import (assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_tensor_close,
                     oracle_trajectory)
from srgnn_torch import adam_step, new_adam_state

pytestmark = pytest.mark.gpu


def make_engine(cfg, w, probs=None, **model_kw):
    import beta_recsys_amd as hp

    model = {**cfg, "device_str": "cuda:0", "optimizer": "adam", "lr": 1e-3, **model_kw}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.ComiRecEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    eng.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    if probs is not None:
        eng.set_item_probs(probs)
    return eng


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's fixture with its float64 and float32 restatement results, computed once."""
    cfg, w, batch, probs = ct.make(case)
    return (cfg, w, batch, probs, ct.grads(w, cfg, batch, torch.float64, probs),
            ct.grads(w, cfg, batch, torch.float32, probs))


@pytest.mark.parametrize("case", sorted(ct.CASES))
def test_loss_interests_kstar_and_gradients_match_float64(hip_device, case):
    cfg, w, batch, probs, (l64, g64, v64, k64, _), (l32, g32, _, _, _) = reference(case)
    eng = make_engine(cfg, w, probs)
    loss, grads = eng.backward_only(batch)
    print(case, "loss", loss, l64, "fp32 restatement", l32)
    assert_scalar_close(loss, l64, what=f"{case} loss")
    assert np.array_equal(eng.last_kstar.cpu().numpy(), k64), f"{case} k*"
    assert_tensor_close(eng.model.interests(batch[0]).cpu().numpy(), v64, what=f"{case} interests")
    assert_grads_as_accurate(grads, g32, g64, what=case)
    assert float(grads["item_emb.weight"][0].abs().max()) == 0.0, "row 0 received a gradient"


@pytest.mark.parametrize("case", sorted(ct.CASES))
def test_routing_stage_matches_the_float64_loop(hip_device, case):
    """Projection + routing on explicit rows and an explicit mask with holes (not a left padding): interests and ``c``."""
    cfg, w, _, _, _, _ = reference(case)
    c = ct.CASES[case]
    gen = torch.Generator().manual_seed(c["T"] * 1000 + c["D"])
    e = torch.randn(c["B"], c["T"], c["D"], generator=gen, dtype=torch.float64)
    mask = torch.rand(c["B"], c["T"], generator=gen) < 0.7
    mask[0], mask[-1] = True, False
    v64, c64 = ct.route(e, torch.tensor(w["routing.weight"], dtype=torch.float64), mask, c["R"])
    v, cc = make_engine(cfg, w).model.routing_stage(e.float().cuda(), mask.cuda())
    assert_tensor_close(v.cpu().numpy(), v64.numpy(), what=f"{case} interests")
    assert_tensor_close(cc.cpu().numpy(), c64.numpy(), what=f"{case} c")
    assert float(cc.cpu().masked_select(~mask[:, None, :].expand_as(c64)).abs().sum()) == 0.0, "a dead slot has a coupling"


def test_left_padding_is_exact_and_shifts_the_routing_weight(hip_device):
    cfg, w, batch, _, _, _ = reference("published")
    eng, T = make_engine(cfg, w), cfg["maxlen"]
    short = batch[0][:3, -7:]
    v = eng.model.interests(short)
    assert torch.equal(v, eng.model.interests(np.pad(short, ((0, 0), (T - 7, 0)))))
    E, W = (torch.tensor(w[n], dtype=torch.float64) for n in ("item_emb.weight", "routing.weight"))
    s = torch.as_tensor(short)
    v64, _ = ct.route(E[s], W[T - 7:], s != 0, cfg["routing_iters"])
    assert_tensor_close(v.cpu().numpy(), v64.numpy(), what="interests of a left-padded row against the unpadded restatement")


def test_no_label_batch_gives_zero_loss_and_gradient(hip_device):
    cfg, w, (seq, target, samples), _ = ct.make("k3_d48")
    eng = make_engine(cfg, w)
    eng._enqueue_grad((seq, np.zeros_like(target), samples))
    torch.cuda.synchronize()
    assert float(eng._g_flat.abs().max()) == 0.0
    loss, _ = eng.backward_only((seq, np.zeros_like(target), samples))
    assert loss == 0.0


def test_gradients_are_bit_reproducible(hip_device):
    cfg, w, batch, _ = ct.make("slab_plus_one")
    eng = make_engine(cfg, w)
    (la, ga), (lb, gb) = eng.backward_only(batch), eng.backward_only(batch)
    assert la == lb
    assert float(ga["routing.weight"].abs().max()) > 0 and torch.equal(ga["routing.weight"], gb["routing.weight"])
    assert float(ga["item_emb.weight"].abs().max()) > 0


def test_three_chained_adam_steps(hip_device):
    cfg, w, batch, probs = ct.make("k3_d48")
    lr = 1e-3
    batches = [batch, (batch[0][::-1].copy(), batch[1][::-1].copy(), batch[2]), batch]
    eng = make_engine(cfg, w, probs, lr=lr)
    for b in batches:
        eng.train_single_batch(b)

    def grad_fn(wk, b):
        return {k: v.astype(np.float32) for k, v in ct.grads(wk, cfg, b, torch.float32, probs)[1].items()}

    w_ref, env, upd = oracle_trajectory(w, batches, grad_fn, lambda wk, g, s: adam_step(wk, g, s, lr, 0.0), new_adam_state)
    got = {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}
    assert_on_trajectory(got, w_ref, env, upd, "adam trajectory")


def test_predict_and_recommend_next(hip_device):
    cfg, w, batch, _, (_, _, _, _, s64), _ = reference("published")
    I, seq = cfg["n_items"], batch[0]
    eng = make_engine(cfg, w)
    cand = np.array([3, 1, I, 7])
    assert_tensor_close(eng.predict(seq, cand).cpu().numpy(), s64[:, cand - 1], what="predict")
    k = 5
    items, top = (t.cpu().numpy() for t in eng.recommend_next(seq, k))
    tk.check_against_float64(items - 1, top, s64, None, "recommend_next")      # distinct ids, every row, the max score
    assert items.shape == (seq.shape[0], k) and (items >= 1).all() and (items <= I).all(), "the padding id was returned"
    rows = np.concatenate([np.repeat(np.arange(seq.shape[0]), k), [0]])
    seen_items = np.concatenate([items.reshape(-1), [0]])      # a 0 entry is ignored
    items_s, top_s = (t.cpu().numpy() for t in eng.recommend_next(seq, k, seen=(rows, seen_items)))
    tk.check_against_float64(items_s - 1, top_s, s64, [r - 1 for r in items], "recommend_next with seen")
    assert (items_s >= 1).all() and not any(set(a) & set(b) for a, b in zip(items_s.tolist(), items.tolist()))
    items_all, _ = (t.cpu().numpy() for t in eng.recommend_next(seq, 100))      # k beyond the catalogue: a -1 tail
    assert all(sorted(r[:I].tolist()) == list(range(1, I + 1)) and (r[I:] == -1).all() for r in items_all)


def test_limits_and_bad_ids(hip_device):
    import beta_recsys_amd as hp

    cfg, w, batch, _, (l64, _, _, _, _), _ = reference("proj_tile_plus_one")
    for kw in (dict(emb_dim=24), dict(emb_dim=0), dict(emb_dim=144), dict(num_interest=0), dict(num_interest=9),
               dict(maxlen=0), dict(maxlen=257), dict(routing_iters=0), dict(routing_iters=5)):
        with pytest.raises(ValueError):
            hp.ComiRec(dict(cfg, **kw))
    eng = make_engine(cfg, w)
    before = eng.model.flat.clone()
    seq, target, samples = batch
    long = np.ones((len(target), cfg["maxlen"] + 1), dtype=np.int64)
    for bad in ((long, target, samples), (seq, target[:-1], samples), (seq, target, samples[:0]),
                (seq, target, np.ones(8193, dtype=np.int64)), (seq, target)):
        with pytest.raises(ValueError):
            eng.backward_only(bad)
    for value in (cfg["n_items"] + 1, -2):
        far_seq, far_target, far_samples = seq.copy(), target.copy(), samples.copy()
        far_seq[0, -1], far_target[2], far_samples[0] = value, value, value
        for bad in ((far_seq, target, samples), (seq, far_target, samples), (seq, target, far_samples)):
            with pytest.raises(IndexError):
                eng.backward_only(bad)
            assert torch.equal(eng.model.flat, before) and float(eng._g_flat.abs().max()) == 0.0, "a partial step was kept"
        with pytest.raises(IndexError):
            eng.model.interests(far_seq)
    loss = eng.train_single_batch(batch)
    assert_scalar_close(loss, l64, what="loss after the errors")
    assert not torch.equal(eng.model.flat, before), "the engine trains on"
