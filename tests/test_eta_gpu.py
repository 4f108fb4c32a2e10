"""ETA on the GPU against the plain-torch restatement ``eta_torch``: the retrieval stage's integers exactly (dyadic fixtures),
the attention stage on an explicit ``sel`` and the whole step against float64, run-to-run bits, chained Adam steps with Dice's
running buffers, ``predict`` / ``rerank``, the limits.

Largest float32-restatement error over the whole-step fixtures: 0.146 of the 1e-5 bound (k_above_live, dnn.0.bias); the
kernels' own largest: 0.091 (published, att.q.bias)."""
import contextlib
import functools
import io

import numpy as np
import pytest
import torch

import eta_torch as et
from helpers import (assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_tensor_close,
                     oracle_trajectory)
from srgnn_torch import adam_step, new_adam_state

pytestmark = pytest.mark.gpu


def make_engine(cfg, w, running=None, **model_kw):
    import beta_recsys_amd as hp

    model = {**cfg, "device_str": "cuda:0", "optimizer": "adam", "lr": 1e-3, **model_kw}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.ETAEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_test_runs"}})
    eng.model.load_state_dict({k: torch.as_tensor(v) for k, v in {**w, **(running or {})}.items()}, strict=running is not None)
    return eng


def k_bias_floor(name, g64):
    """d att.k.bias is exactly zero (it sums ds_j Qp / sqrt(dh) and a softmax's ds sums to 0): float64 leaves 1e-17 there, a
    float32 sum the rounding of its terms.  d att.k.weight sums the same terms times |e| of about 1: its scale is the floor."""
    return float(np.abs(g64["att.k.weight"]).max()) if name == "att.k.bias" else 0.0


@functools.lru_cache(maxsize=None)
def reference(case):
    """The case's fixture with its float64 and float32 restatement results, computed once."""
    cfg, w, batch, running = et.make(case)
    return cfg, w, batch, running, et.grads(w, cfg, batch, torch.float64), et.grads(w, cfg, batch, torch.float32)


@pytest.mark.parametrize("case", sorted(et.RETRIEVE_CASES))
def test_retrieve_stage_is_exact(hip_device, case):
    cfg, hash_w, e, q, mask = et.make_retrieve(case)
    ce, cq, sel = et.retrieve(e, q, mask, hash_w, cfg["top_k"])
    model = make_engine(cfg, {"hash.weight": hash_w}).model
    got = [t.cpu() for t in model.retrieve_stage(e, q, mask)]
    for name, g, r in zip(("codes_e", "codes_q", "sel"), got, (ce, cq, sel)):
        assert torch.equal(g, r), f"{case} {name}: {int((g != r).sum())} of {r.numel()} differ"
    assert int((sel[-1] >= 0).sum()) == 0 and int((sel[0] >= 0).sum(-1).min()) == min(cfg["top_k"], int(mask[0].sum()))


@pytest.mark.parametrize("case", sorted(et.ATTENTION_CASES))
def test_attention_stage_matches_float64(hip_device, case):
    cfg, w, e, q, sel, dv = et.make_attention(case)
    names = [f"att.{p}.{n}" for p in "qkvo" for n in ("weight", "bias")]
    w64 = {n: torch.tensor(w[n], dtype=torch.float64, requires_grad=True) for n in names}
    e.requires_grad_(), q.requires_grad_()
    v64 = et.attention(e, q, sel, w64, cfg["num_heads"])
    v64.backward(dv)
    model = make_engine(cfg, w).model
    v, de, dq, grads = model.attention_stage(e.detach(), q.detach(), sel, dv)
    print(case, model.tiles(sel.shape[1]))
    assert_tensor_close(v.cpu().numpy(), v64.detach().numpy(), what=f"{case} v")
    assert_tensor_close(de.cpu().numpy(), e.grad.numpy(), what=f"{case} de")
    assert_tensor_close(dq.cpu().numpy(), q.grad.numpy(), what=f"{case} dq")
    for n in names:
        assert_tensor_close(grads[n].cpu().numpy(), w64[n].grad.numpy(), what=f"{case} {n}",
                            scale_floor=k_bias_floor(n, {m: w64[m].grad.numpy() for m in names}))
    assert torch.equal(model.attention_stage(e.detach(), q.detach(), sel), v)


@pytest.mark.parametrize("case", sorted(et.CASES))
def test_loss_logits_and_gradients_match_float64(hip_device, case):
    cfg, w, batch, running, (l64, g64, z64, s64), (l32, g32, _, s32) = reference(case)
    assert np.array_equal(s64, s32), "the fixture's selection differs between float32 and float64"
    eng = make_engine(cfg, w, running)
    loss, grads = eng.backward_only(batch)
    print(case, "loss", loss, l64, "fp32 restatement", l32, eng.model.tiles(et.CASES[case]["C"]))
    for n in g64:
        scale = max(float(np.abs(g64[n]).max()), k_bias_floor(n, g64), 1e-30)
        print(f"  {n}: fp32 restatement {np.abs(g32[n] - g64[n]).max() / scale / 1e-5:.3f}, "
              f"kernel {np.abs(grads[n].cpu().numpy().reshape(g64[n].shape) - g64[n]).max() / scale / 1e-5:.3f} of the bound")
    assert_scalar_close(loss, l64, what=f"{case} loss")
    assert_tensor_close(eng.last_logits.cpu().numpy(), z64, what=f"{case} logits")
    assert_grads_as_accurate(grads, g32, g64, what=case, floor_fn=lambda n: k_bias_floor(n, g64))
    assert float(grads["item_emb.weight"][0].abs().max()) == 0.0, "row 0 received a gradient"
    for n, v in running.items():      # backward_only leaves Dice's buffers alone
        assert np.array_equal(eng.model.state_dict()[n].cpu().numpy(), v), n


def test_gradients_are_bit_reproducible(hip_device):
    cfg, w, batch, running = et.make("slices")
    eng = make_engine(cfg, w, running)
    (la, ga), (lb, gb) = eng.backward_only(batch), eng.backward_only(batch)
    assert la == lb
    for n in ga:
        assert float(ga[n].abs().max()) > 0, n
        assert n == "item_emb.weight" or torch.equal(ga[n], gb[n]), n      # item_emb.weight: row atomics


def test_three_chained_adam_steps_and_running_buffers(hip_device):
    cfg, w, batch, running = et.make("k_above_live")      # top_k >= maxlen: the selection cannot move with the weights
    lr = 1e-3
    batches = [batch, tuple(a[::-1].copy() for a in batch), batch]
    eng = make_engine(cfg, w, running, lr=lr)
    for b in batches:
        eng.train_single_batch(b)
    run32 = {n: v.copy() for n, v in running.items()}
    hw = {"hash.weight": w["hash.weight"]}
    w0 = {k: v for k, v in w.items() if k != "hash.weight"}

    def grad_fn(wk, b, run=None):
        return {k: v.astype(np.float32) for k, v in et.grads({**wk, **hw}, cfg, b, torch.float32, run)[1].items()}

    # att.k.bias: Adam normalises a gradient that is rounding noise (no output depends on it): its envelope is pooled
    g64 = et.grads(w, cfg, batch)[1]
    w_ref, env, upd = oracle_trajectory(w0, batches, grad_fn, lambda wk, g, s: adam_step(wk, g, s, lr, 0.0), new_adam_state,
                                        floor_fn=lambda n, b: k_bias_floor(n, g64))
    wk, state = {k: v.copy() for k, v in w0.items()}, new_adam_state(w0)
    for b in batches:      # the reference run once more, this time moving BatchNorm1d's buffers
        adam_step(wk, grad_fn(wk, b, run32), state, lr, 0.0)
    got = {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}
    rest = [k for k in w_ref if k != "att.k.bias"]
    assert_on_trajectory({k: got[k] for k in rest}, {k: w_ref[k] for k in rest}, env, upd, "adam trajectory")
    assert_on_trajectory(got, {"att.k.bias": w_ref["att.k.bias"]}, env, upd, "adam trajectory", pool=True)
    assert np.array_equal(got["hash.weight"], w["hash.weight"]), "the optimizer moved hash.weight"
    for n, v in run32.items():
        assert not np.array_equal(v, running[n])
        assert_tensor_close(got[n], v, what=n)


def test_predict_and_rerank(hip_device):
    cfg, w, (seq, cand, _), running = et.make("published", n_cand=100)
    cand[1, 5:] = 0      # a row with five live candidates
    z64 = et.predict(w, cfg, seq, cand, running)
    eng = make_engine(cfg, w, running)
    z = eng.predict(seq, cand).cpu().numpy()
    assert_tensor_close(z, z64, what="predict")
    assert (z[cand == 0] == 0.0).all()
    k = 10
    items, top = (t.cpu().numpy() for t in eng.rerank(seq, cand, k))
    for b in range(seq.shape[0]):
        live = np.flatnonzero(cand[b])
        n = min(k, live.size)
        assert_tensor_close(top[b, :n], np.sort(z64[b, live])[::-1][:n], what=f"rerank row {b}")
        assert all(i in cand[b, live] for i in items[b, :n]) and (items[b, n:] == -1).all() and np.isinf(top[b, n:]).all()


def test_limits_and_bad_ids(hip_device):
    import beta_recsys_amd as hp

    cfg, w, batch, running, (l64, _, _, _), _ = reference("chunk_plus_one")
    for kw in (dict(emb_dim=24), dict(emb_dim=144), dict(maxlen=0), dict(maxlen=4097), dict(hash_bits=48), dict(hash_bits=160),
               dict(top_k=0), dict(top_k=129), dict(num_heads=3), dict(num_heads=8), dict(dnn_hidden=[]),
               dict(dnn_hidden=[513]), dict(dnn_activation="relu")):
        with pytest.raises(ValueError):
            hp.ETA(dict(cfg, **kw))
    eng = make_engine(cfg, w, running)
    for B, C in (((1 << 24) // cfg["maxlen"] + 1, 1), (1 << 12, (1 << 12) // cfg["top_k"] + 1)):
        with pytest.raises(ValueError):      # batch x maxlen and batch x candidates x top_k within 2^24
            eng.model.workspace(hp._lib.load(), B, C, 1)
    before = eng.model.flat.clone()
    seq, cand, label = batch
    for bad in ((np.ones((len(seq), cfg["maxlen"] + 1), dtype=np.int64), cand, label), (seq, cand[:-1], label),
                (seq, cand, label[:, :-1]), (seq, cand)):
        with pytest.raises(ValueError):
            eng.backward_only(bad)
    for value in (cfg["n_items"] + 1, -2):
        far_seq, far_cand = seq.copy(), cand.copy()
        far_seq[0, -1], far_cand[1, 0] = value, value
        for bad in ((far_seq, cand, label), (seq, far_cand, label)):
            with pytest.raises(IndexError):
                eng.backward_only(bad)
            assert torch.equal(eng.model.flat, before) and float(eng._g_flat.abs().max()) == 0.0, "a partial step was kept"
        with pytest.raises(IndexError):
            eng.model.forward(far_seq, cand)
    loss = eng.train_single_batch(batch)
    assert_scalar_close(loss, l64, what="loss after the errors")
    assert not torch.equal(eng.model.flat, before), "the engine trains on"

    long = et.config(dict(T=257, D=16, k=4, B=2))      # where DIN stops
    with pytest.raises(ValueError):
        hp.DIN({k: long[k] for k in ("n_items", "emb_dim", "maxlen", "batch_size")})
    rng = np.random.default_rng(0)
    batch = (rng.integers(1, et.N_ITEMS + 1, (2, 257)), rng.integers(1, et.N_ITEMS + 1, (2, 3)), np.ones((2, 3), np.float32))
    eng = make_engine(long, {})
    assert eng.train_single_batch(batch) > eng.train_single_batch(batch) > 0.0
