"""The reported BPR loss of the gradient kernels (csrc/mf.hip), where nothing else can see it.

The loss term -logsigmoid(yp - yn) feeds no gradient: each wave parks its yp - yn in LDS and one wave of the block
evaluates the block's 16 terms, one per lane.  A wrong statistic moves no weight, so only loss assertions catch a slot
that is stale, skipped or counted twice.  Every case compares the per-step loss and the epoch's loss sum with
oracle/mf_numpy.py at the suite's 1e-5, on 37 x 23 tables, unshuffled batches:

  batch 1                      smallest case: one valid wave in the only block
  batch 15, 16, 17             the evaluating wave (the block's last) lies past the end of the batch / is its last
                               triple / a second block holds one triple
  batch 4096 + 5               second trip of the fused kernel's gather loop (256 blocks x 16 waves per trip) with 5
                               valid waves in one block: a stale slot would count a triple of the first trip twice
  batch 2 * 4096 + 16 * 3 + 1  ragged third trip over several blocks

through the fused resident epoch (mf_bpr_fused_kernel) and the two-kernel epoch (mf_bpr_grad_kernel), at dim 8, 64
(one column per lane) and 70 (two), with SGD, Adam and RMSprop, once with the regularizer.  Those triples never have
n == p (see _triples); x == 0 exactly is held on a first step of its own, where no weight has moved yet.
"""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

from helpers import assert_scalar_close
from oracle import mf_numpy as onp

pytestmark = pytest.mark.gpu

U, I, LR = 37, 23, 0.02
BATCHES = [1, 15, 16, 17, 4096 + 5, 2 * 4096 + 16 * 3 + 1]
CONFIGS = [(8, "sgd", None), (64, "adam", None), (70, "rmsprop", None), (64, "sgd", 0.01), (70, "adam", None)]


def _engine(D, optimizer, B, reg):
    import beta_recsys_amd as hp

    model = dict(n_users=U, n_items=I, emb_dim=D, device_str="cuda:0", optimizer=optimizer, lr=LR, batch_size=B,
                 loss="bpr")
    cfg = {"model": model, "system": {"run_dir": "/tmp/hiprec_test_runs"}}
    if reg is not None:
        cfg["reg"] = reg
        model["reg"] = reg
    with contextlib.redirect_stdout(io.StringIO()):
        return hp.MFEngine(cfg)


def _triples(n, seed):
    """Uniform triples whose negative item is never the positive one, as a BPR sampler draws them.  With n == p the
    user row's gradient dpos * p + dneg * n is the rounding residue of an exact cancellation (0 or ~1e-10 depending on
    which product a compiler fuses), which Adam / RMSprop turn into a step of up to lr: an ill-conditioned input for
    the weights (helpers.optimizer_band), and through them for the next step's loss -- not what this file is about."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, I, n)
    return rng.integers(0, U, n), pos, (pos + rng.integers(1, I, n)) % I


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_kernel"])
@pytest.mark.parametrize("D,optimizer,reg", CONFIGS)
def test_bpr_loss_statistic_against_the_oracle(hip_device, D, optimizer, reg, fused):
    """Per batch size a fresh engine: three epoch calls of one batch each (stats.loss = stats.loss_sum = that step's
    loss), then one epoch of three batches (its loss sum, and the last step's loss)."""
    import beta_recsys_amd as hp

    reg_coef = 0.0 if reg is None else reg
    for B in BATCHES:
        data = _triples(6 * B, seed=B + D)
        w = onp.init_params(U, I, D, seed=D)
        eng = _engine(D, optimizer, B, reg)
        eng.fused_step = fused
        eng.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        eng._setup()
        assert eng._fused_ok(None) == fused and eng._lazy is None
        st = onp.new_opt_state(w, optimizer)
        dev = [torch.from_numpy(a).cuda() for a in data]

        def oracle_steps(lo, hi):
            return [onp.mf_train_step(w, st, tuple(a[k:k + B] for a in data), "bpr", optimizer, LR, reg_coef=reg_coef)[0]
                    for k in range(lo, hi, B)]

        def epoch(lo, hi):
            loader = hp.DeviceTripleBatcher(*(t[lo:hi] for t in dev), B, shuffle=False)
            with contextlib.redirect_stdout(io.StringIO()):
                eng.train_an_epoch(loader, 0)
            return eng.epoch_stats()

        what = f"D={D} {optimizer} B={B}"
        for s in range(3):
            (ref,) = oracle_steps(s * B, (s + 1) * B)
            stats = epoch(s * B, (s + 1) * B)
            print(f"{what} step {s}: loss {stats.loss!r} sum {stats.loss_sum!r} oracle {ref!r}")
            assert_scalar_close(stats.loss, ref, 1e-5, f"{what} loss of step {s}")
            assert_scalar_close(stats.loss_sum, ref, 1e-5, f"{what} loss sum of the one-step epoch {s}")
        refs = oracle_steps(3 * B, 6 * B)
        stats = epoch(3 * B, 6 * B)
        print(f"{what} epoch: loss {stats.loss!r} sum {stats.loss_sum!r} oracle {refs[-1]!r} {sum(refs)!r}")
        assert stats.step == 6
        assert_scalar_close(stats.loss_sum, sum(float(r) for r in refs), 1e-5, f"{what} epoch loss sum")
        assert_scalar_close(stats.loss, refs[-1], 1e-5, f"{what} loss of the epoch's last step")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two_kernel"])
@pytest.mark.parametrize("D,optimizer", [(64, "adam"), (70, "rmsprop")])
def test_equal_items_give_a_loss_term_of_log_two(hip_device, D, optimizer, fused):
    """n == p makes yp == yn, x = yp - yn == 0 exactly and the term log1p(exp(-0)) - min(0, 0) = log 2.  The FIRST
    step of a fresh engine only: its loss is taken from the initial weights, so the ill-conditioned update such a
    triple causes (see _triples) cannot reach it.  17 triples (a second block with one wave), every other one with
    n == p; and a batch of nothing else, whose loss is log 2 itself."""
    import beta_recsys_amd as hp

    B = 17
    for every in (2, 1):
        users, pos, neg = _triples(B, seed=D + every)
        neg = neg.copy()
        neg[::every] = pos[::every]
        w = onp.init_params(U, I, D, seed=D)
        eng = _engine(D, optimizer, B, None)
        eng.fused_step = fused
        eng.model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        ref, _, _ = onp.mf_bpr_grads(w, users, pos, neg)
        loader = hp.DeviceTripleBatcher(*(torch.from_numpy(a).cuda() for a in (users, pos, neg)), B, shuffle=False)
        with contextlib.redirect_stdout(io.StringIO()):
            eng.train_an_epoch(loader, 0)
        stats = eng.epoch_stats()
        print(f"D={D} {optimizer} n == p in every {every}: loss {stats.loss!r} oracle {ref!r}")
        assert stats.step == 1
        assert_scalar_close(stats.loss, ref, 1e-5, f"D={D} {optimizer} loss with n == p in every {every} triple")
        assert_scalar_close(stats.loss_sum, ref, 1e-5, f"D={D} {optimizer} loss sum with n == p in every {every} triple")
        if every == 1:
            assert_scalar_close(stats.loss, np.log(2.0), 1e-5, "a batch of n == p triples")


def test_fused_step_leaves_a_flagged_triple_out_of_the_loss(hip_device):
    """hiprec_mf_bpr_fused_step on a batch of 32 with one out-of-range user id: the status bit is raised and the
    loss is the oracle's sum over the other 31 triples, divided by 32 (the flagged wave parks a term of exactly 0)."""
    from beta_recsys_amd import _lib
    from beta_recsys_amd._stats import _new_stats, read_stats

    lib = _lib.load()
    D, B, bad = 64, 32, 21
    w = onp.init_params(U, I, D, seed=3)
    users, pos, neg = _triples(B, seed=3)
    keep = np.arange(B) != bad
    ref31, _, _ = onp.mf_bpr_grads(w, users[keep], pos[keep], neg[keep])
    users = users.copy()
    users[bad] = U + 2
    flat = torch.from_numpy(np.concatenate([w[k].ravel() for k in (
        "user_emb.weight", "item_emb.weight", "user_bias.weight", "item_bias.weight", "global_bias")])).cuda()
    assert flat.numel() == (U + I) * (D + 1) + 1
    w_alt = torch.empty_like(flat)
    g = [torch.zeros_like(flat) for _ in range(3)]
    scratch = [torch.zeros(lib.hiprec_scratch_bytes(0), dtype=torch.uint8, device=hip_device) for _ in range(2)]
    stats = _new_stats(hip_device)
    idx = [torch.from_numpy(a).cuda() for a in (users, pos, neg)]

    def step(k, flush):
        c = _lib.FusedStep()
        c.kind, c.dim, c.n_users, c.n_items = _lib.OPT_SGD, D, U, I
        c.w_read, c.w_write = (flat, w_alt)[k & 1].data_ptr(), (flat if flush else (flat, w_alt)[(k + 1) & 1]).data_ptr()
        c.g_prev, c.g_cur, c.g_zero = g[(k + 2) % 3].data_ptr(), g[k % 3].data_ptr(), g[(k + 1) % 3].data_ptr()
        c.scratch_prev, c.scratch_cur = scratch[(k + 1) & 1].data_ptr(), scratch[k & 1].data_ptr()
        c.lr, c.beta1, c.beta2, c.eps, c.reg_coef = LR, 0.9, 0.999, 1e-8, 0.0
        return c

    stream = _lib.stream_ptr(hip_device)
    first, flush = step(0, False), step(1, True)
    _lib.check(lib.hiprec_mf_bpr_fused_step(ctypes.byref(first), *(t.data_ptr() for t in idx), B, 0, 1.0 / B,
                                            stats.data_ptr(), stream))
    _lib.check(lib.hiprec_mf_bpr_fused_step(ctypes.byref(flush), None, None, None, 0, B, 0.0, stats.data_ptr(),
                                            stream))
    st = read_stats(stats)
    print(f"flagged triple: status {st.status:#x} loss {st.loss!r} oracle {float(ref31) * 31 / 32!r}")
    assert st.status == _lib.STATUS_USER_OOB
    assert_scalar_close(st.loss, float(ref31) * 31 / 32, 1e-5, "loss of 31 valid triples over a batch of 32")
    assert_scalar_close(st.loss_sum, float(ref31) * 31 / 32, 1e-5, "loss sum of 31 valid triples over a batch of 32")
