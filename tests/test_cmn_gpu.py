"""GPU parity tests of CMN (csrc/cmn.hip, the momentum kind of csrc/optim.hip): forward + loss + backward, the clip, the
full step and chained steps vs golden vectors from the real reference's cmnEngine (tests/golden/cmn_*.npz); the padded
and the CSR form against each other; the resident epoch against stepped batches; and the numpy restatement at list
lengths that span several rounds of the kernel whatever its chunk."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import cmn_numpy as cn
import topk_reference as tk
from cmn_edges import synthetic
from helpers import EPS32, REL, assert_grads_as_accurate, assert_on_trajectory, assert_scalar_close, assert_sgd_exact
from helpers import assert_step_close, assert_tensor_close, copy_state, float64_oracle, load_golden, oracle_trajectory
from helpers import to64
from test_oracle_golden_cmn import CASES, KEYS, STATE_NAMES, cmn_band, cmn_batch, cmn_hyper, cmn_opt_state, cmn_params
from test_oracle_golden_cmn import cmn_triples, exact_grads, n_steps, term_floors

pytestmark = pytest.mark.gpu
IEEE_BUILD = os.environ.get("HIPREC_LIB", "").endswith("ieee.so")


def make_engine(w, rowptr, col, optimizer, lr, momentum, lam, clip, B):
    import beta_recsys_amd as hp

    I = len(rowptr) - 1
    lists = {i: np.asarray(col[rowptr[i]:rowptr[i + 1]]).tolist() for i in range(I)}
    name = "default" if optimizer == "rmsprop_momentum" else optimizer
    cfg = {"emb_dim": w["user_memory.weight"].shape[1], "device_str": "cuda:0", "regs": [1e-5], "batch_size": B,
           "lr": lr, "momentum": momentum or 0.9, "training_l2_lambda": lam, "grad_clip": clip, "neg_count": 4,
           "model": {"optimizer": name, "lr": lr, "device_str": "cuda:0"},
           "system": {"run_dir": "/tmp/hiprec_test_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.cmnEngine(cfg, w["user_memory.weight"], w["item_memory.weight"], lists)
    load_weights(eng, w)
    return eng


def golden_engine(case, g):
    opt, lr, mom, lam, clip = cmn_hyper(g)
    return make_engine(cmn_params(case, g, 0), g["rowptr"], g["col"], opt, lr, mom, lam, clip, int(g["meta"][3]))


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def load_opt_state(eng, st, opt):
    names = STATE_NAMES[opt]
    eng.load_optimizer_state(st["step"], st[names[0]] if names else None, st[names[1]] if names else None)


def np_grads(grads):
    return {k: v.cpu().numpy() for k, v in grads.items()}


def engine_state(eng, opt):
    names = STATE_NAMES[opt]
    bufs = (eng.optimizer.exp_avg, eng.optimizer.exp_avg_sq)
    return {n: {k: v.cpu().numpy() for k, v in eng.model.views(b).items()} for n, b in zip(names, bufs)}


def state_band(w_prev, st_prev, g_own, opt, lr, momentum, floors, rel=REL):
    """Elementwise spread of the optimizer state after one step over gradients within rel of their scale of ``g_own``."""
    outs = []
    for sign in (+1.0, -1.0):
        w, st = {k: v.copy() for k, v in w_prev.items()}, copy_state(st_prev)
        gp = {k: (g_own[k] + np.float32(sign * rel * max(float(np.abs(g_own[k]).max()), floors[k]))).astype(np.float32)
              for k in KEYS}
        cn.opt_step(w, gp, st, opt, lr, momentum)
        outs.append(st)
    return {n: {k: np.abs(outs[0][n][k].astype(np.float64) - outs[1][n][k].astype(np.float64)) for k in KEYS}
            for n in STATE_NAMES[opt]}


@pytest.mark.parametrize("case", CASES)
def test_step_matches_reference(hip_device, case):
    """Each step from the reference's own weights and optimizer state: loss, every clipped gradient (as accurate as the
    reference against the fp64 evaluation), the pre-clip norm, the stepped weights and state, the gradient left cleared."""
    g = load_golden(case)
    opt, lr, mom, lam, clip = cmn_hyper(g)
    eng = golden_engine(case, g)
    for s in range(n_steps(g)):
        batch = cmn_batch(g, s)
        w0, st0 = cmn_params(case, g, s), cmn_opt_state(case, g, s)
        load_weights(eng, w0)
        load_opt_state(eng, st0, opt)
        loss, grads, total = eng.backward_only(batch)
        grads = np_grads(grads)
        print(f"{case} step {s}: loss {loss!r} vs {float(g['losses'][s])!r}; norm {total!r} vs {float(g['total_norms'][s])!r}")
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        assert_scalar_close(total, g["total_norms"][s], what=f"total norm step {s}")
        g_ref = cmn_params(case, g, s + 1, "g")
        _, g64, _ = exact_grads(w0, batch, lam, clip)
        floors = term_floors(w0, batch, lam, clip)
        for k in KEYS:
            print(f"  grad {k}: err vs exact {np.abs(grads[k] - g64[k]).max():.3e}, reference's own "
                  f"{np.abs(g_ref[k] - g64[k]).max():.3e}, scale {max(np.abs(g64[k]).max(), floors[k]):.3e}")
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}", floor_fn=floors.get)
        assert float(eng._g_flat.abs().max()) == 0.0
        assert np.array_equal(get_weights(eng)["user_output.weight"], w0["user_output.weight"])
        # the full step
        load_opt_state(eng, st0, opt)
        loss = eng.train_single_batch(batch)
        assert_scalar_close(loss, g["losses"][s], what=f"loss (step) {s}")
        band = cmn_band(w0, st0, g_ref, opt, lr, mom, floors=floors)
        w1, w_ref = get_weights(eng), cmn_params(case, g, s + 1)
        for k in KEYS:
            assert_step_close(w0[k], w1[k], w_ref[k], band[k], what=f"weights {k} step {s}")
        # the sweep's own arithmetic: the oracle's step from the gradient this engine computed
        w2, st2 = {k: v.copy() for k, v in w0.items()}, cmn_opt_state(case, g, s)
        cn.opt_step(w2, grads, st2, opt, lr, mom)
        # (the step's gradient is a second run of the kernel: its float atomics arrive in another order, and RMSprop's
        # momentum buffer g / (sqrt(square_avg) + eps) is ill-conditioned where |g| is not >> eps -- hence the band, the
        # rule of helpers.optimizer_band applied to the state)
        got, sband = engine_state(eng, opt), state_band(w0, st0, grads, opt, lr, mom, floors)
        for i, name in enumerate(STATE_NAMES[opt]):
            for k in KEYS:
                ref = st2[name][k].astype(np.float64)
                tol = (REL if i == 0 else 2 * REL) * np.abs(ref).max() + sband[name][k]
                err = np.abs(got[name][k].astype(np.float64) - ref)
                assert (err <= tol).all(), f"{name} {k} step {s}: worst {err.max():.3e} vs {tol[np.argmax(err)]:.3e}"
        assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"


@pytest.mark.parametrize("case", CASES)
def test_trajectory_matches_reference(hip_device, case):
    """All steps chained from w0.  SGD: every element within 1e-5 of the trajectory's update; Adam / RMSprop with
    momentum: every element inside the oracle's perturbed-gradient envelope around the reference's end point."""
    g = load_golden(case)
    opt, lr, mom, lam, clip = cmn_hyper(g)
    eng = golden_engine(case, g)
    w0 = cmn_params(case, g, 0)
    batches = [cmn_batch(g, s) for s in range(n_steps(g))]
    for s, b in enumerate(batches):
        loss = eng.train_single_batch(b)
        print(f"{case} chained step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        if opt == "sgd" or s == 0:
            assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
    ref_end = cmn_params(case, g, n_steps(g))
    if opt == "sgd":
        assert_sgd_exact(get_weights(eng), ref_end, w0, "final weights")
        return
    floors = {id(b): term_floors(w0, b, lam, clip) for b in batches}     # lr 1e-4: the weights hardly move
    _, env, upd = oracle_trajectory(
        w0, batches, lambda w, b: cn.clip_grads(cn.cmn_grads(w, b, lam)[1], clip)[1],
        lambda w, gr, st: cn.opt_step(w, gr, st, opt, lr, mom), lambda w: cn.new_opt_state(w, opt),
        lambda k, b: floors[id(b)][k])
    assert_on_trajectory(get_weights(eng), ref_end, env, upd, f"{case} trajectory")


@pytest.mark.parametrize("case", CASES)
def test_csr_form_equals_padded_form(hip_device, case):
    """The same batch as triples (lists from the constructor's item_user_list, on the device) and as the seven padded
    arrays: the same loss, norm and gradients within the same bounds."""
    g = load_golden(case)
    opt, lr, mom, lam, clip = cmn_hyper(g)
    eng = golden_engine(case, g)
    s = 0
    w0 = cmn_params(case, g, s)
    _, g64, _ = exact_grads(w0, cmn_batch(g, s), lam, clip)
    floors = term_floors(w0, cmn_batch(g, s), lam, clip)
    g_ref = cmn_params(case, g, s + 1, "g")
    out = {}
    for form, batch in (("padded", cmn_batch(g, s)), ("csr", cmn_triples(g, s))):
        loss, grads, total = eng.backward_only(batch)
        assert_scalar_close(loss, g["losses"][s], what=f"{form} loss")
        assert_scalar_close(total, g["total_norms"][s], what=f"{form} total norm")
        assert_grads_as_accurate(np_grads(grads), g_ref, g64, what=f"{form} grad", floor_fn=floors.get)
        out[form] = (loss, total)
    assert_scalar_close(out["csr"][0], out["padded"][0], what="loss, csr vs padded")
    # a padded matrix narrower than max_neighbors but wide enough for the batch is honoured as given
    u, p, n, pn, pl, nn_, nl = cmn_batch(g, s)
    loss, _, _ = eng.backward_only((u, p, n, pn[:, :int(pl.max())], pl, nn_[:, :int(nl.max())], nl))
    assert_scalar_close(loss, g["losses"][s], what="trimmed padding")


def test_resident_epoch_equals_stepped_batches(hip_device):
    """hiprec_cmn_epoch (train_an_epoch on a device triple batcher) against train_single_batch on the same batches:
    the epoch's loss sum goes to the writer, the LAST batch's loss is printed, both end on the reference's trajectory."""
    from beta_recsys_amd.data import DeviceTensorBatcher

    case = "cmn_sgd_hot_clip"
    g = load_golden(case)
    stepped, epoch = golden_engine(case, g), golden_engine(case, g)
    w0 = cmn_params(case, g, 0)
    losses = [stepped.train_single_batch(cmn_triples(g, s)) for s in range(n_steps(g))]
    for s, loss in enumerate(losses):
        assert_scalar_close(loss, g["losses"][s], what=f"stepped loss {s}")
    cols = [torch.from_numpy(np.asarray(g[k], dtype=np.int64)).to(hip_device) for k in ("users", "pos", "neg")]
    loader = DeviceTensorBatcher(cols, int(g["meta"][3]), shuffle=False)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        epoch.train_an_epoch(loader, 7)
    tag, total, epoch_id = epoch.writer.scalars[-1]
    assert (tag, epoch_id) == ("model/loss", 7)
    assert_scalar_close(total, sum(losses), REL, "epoch loss sum")
    assert_scalar_close(float(out.getvalue().strip().rsplit("Loss ", 1)[1]), losses[-1], REL, "printed last loss")
    ref_end = cmn_params(case, g, n_steps(g))
    assert_sgd_exact(get_weights(stepped), ref_end, w0, "stepped")
    assert_sgd_exact(get_weights(epoch), ref_end, w0, "epoch")
    assert float(epoch._g_flat.abs().max()) == 0.0


class StubLoader:
    """Records the call the engine makes and hands out the fixture's batches as cmn_train_loader's 5-tuples."""

    def __init__(self, g):
        self.g, self.calls = g, []

    def cmn_train_loader(self, batch_size, neighborhood, neg_count):
        self.calls.append((batch_size, neighborhood, neg_count))
        for s in range(n_steps(self.g)):
            u, p, n, pn, pl, nn_, nl = cmn_batch(self.g, s)
            yield (np.stack([u, p, n], axis=1).astype(np.uint32), pn.astype(np.int32), pl.astype(np.int32),
                   nn_.astype(np.int32), nl.astype(np.int32))


def test_train_an_epoch_asks_the_loader_as_the_reference_does(hip_device):
    case = "cmn_adam"
    g = load_golden(case)
    opt, lr, mom, lam, clip = cmn_hyper(g)
    eng = golden_engine(case, g)
    loader = StubLoader(g)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        eng.train_an_epoch(loader, 3)
    assert loader.calls == [(int(g["meta"][3]), True, 4)]
    tag, total, epoch_id = eng.writer.scalars[-1]
    assert (tag, epoch_id) == ("model/loss", 3)
    assert_scalar_close(total, float(g["losses"].sum()), 2 * REL, "epoch loss sum")
    # any other iterable of 5-tuples takes the same path
    load_weights(eng, cmn_params(case, g, 0))
    eng.load_optimizer_state(0)
    with contextlib.redirect_stdout(io.StringIO()):
        eng.train_an_epoch(list(loader.cmn_train_loader(14, True, 4)), 4)
    assert_scalar_close(eng.writer.scalars[-1][1], float(g["losses"].sum()), 2 * REL, "epoch loss sum (iterable)")


@pytest.mark.parametrize("case", ["cmn_adam", "cmn_sgd_hot_clip"])
def test_forward_predict_and_recommend(hip_device, case):
    """forward / forward(evaluation=True) equal the restatement's scores, predict is the dot product of the two
    memories, and engine.recommend ranks the whole catalogue by it."""
    g = load_golden(case)
    eng = golden_engine(case, g)
    w = cmn_params(case, g, 0)
    batch = cmn_batch(g, 0)
    with float64_oracle(cn):
        sp, _ = cn.cmn_query(to64(w), batch[0], batch[1], batch[3], batch[4])
        sn, _ = cn.cmn_query(to64(w), batch[0], batch[2], batch[5], batch[6])
    pos, neg = eng.model(*batch)
    assert pos.dtype == torch.float32 and tuple(pos.shape) == (len(batch[0]),)
    assert_tensor_close(pos.cpu().numpy(), sp, what="forward pos")
    assert_tensor_close(neg.cpu().numpy(), sn, what="forward neg")
    only = eng.model(*batch, evaluation=True)
    assert torch.equal(only, pos)
    users, items = batch[0], batch[2]
    scores = eng.model.predict(users, items)
    assert_tensor_close(scores.cpu().numpy(), cn.cmn_predict(to64(w), users, items), what="predict")
    with pytest.raises(IndexError):
        eng.model.predict([0, w["user_memory.weight"].shape[0]], [0, 0])
    q = np.arange(0, w["user_memory.weight"].shape[0], 7)
    got_i, got_s = eng.recommend(q, 5)
    s64 = tk.scores64(w["user_memory.weight"], w["item_memory.weight"], 1.0, None, q)
    tk.check_against_float64(got_i.cpu().numpy(), got_s.cpu().numpy(), s64, None, "recommend")


@pytest.mark.parametrize("U,D,lengths,B", [(1600, 16, [1, 64, 65, 300, 1500], 10), (70, 7, [1, 3, 70, 64], 1),
                                           (300, 256, [2, 257, 33], 5)])
def test_synthetic_lists_against_the_restatement(hip_device, U, D, lengths, B):
    """Lists that span several rounds of the kernel whatever its chunk (up to 1500 of 1600 users), a width that is no
    multiple of 4 with a batch of ONE sample, and the widest rows: loss and gradients against the restatement in fp64,
    as accurate as its fp32 self, in both forms."""
    lam, clip = 0.001, 5.0
    w, rowptr, col, triples = synthetic(U, D, lengths, B, seed=U + D)
    eng = make_engine(w, rowptr, col, "sgd", 0.01, 0.9, lam, clip, B)
    batch = cn.padded_batch(rowptr, col, *triples)
    loss32, g32 = cn.cmn_grads(w, batch, lam)
    total32, g32 = cn.clip_grads(g32, clip)
    loss64, g64, total64 = exact_grads(w, batch, lam, clip)
    floors = term_floors(w, batch, lam, clip)
    for form, b in (("padded", batch), ("csr", triples)):
        loss, grads, total = eng.backward_only(b)
        print(f"U {U} D {D} {form}: loss {loss!r} vs exact {loss64!r}, norm {total!r} vs {total64!r}")
        assert_scalar_close(loss, loss64, what=f"{form} loss")
        assert_scalar_close(total, total64, what=f"{form} total norm")
        assert_grads_as_accurate(np_grads(grads), g32, g64, what=f"{form} grad", floor_fn=floors.get)


def test_out_of_range_ids_raise_and_leave_the_engine_usable(hip_device):
    case = "cmn_rmsprop_mom"
    g = load_golden(case)
    eng = golden_engine(case, g)
    U, I = int(g["meta"][0]), int(g["meta"][1])
    good = cmn_batch(g, 0)
    before = eng.model.flat.clone()

    def broken(slot, row, value, col=None):
        b = [a.copy() for a in good]
        if col is None:
            b[slot][row] = value
        else:
            b[slot][row, col] = value
        return tuple(b)

    first_len = int(good[4][2])
    cases = {"neighbour id": broken(3, 2, U, first_len - 1), "negative neighbour id": broken(5, 1, -1, 0),
             "user": broken(0, 3, U), "item": broken(2, 4, I), "zero length": broken(4, 0, 0),
             "length beyond the padding": broken(6, 0, good[5].shape[1] + 1)}
    for what, b in cases.items():
        with pytest.raises(IndexError):
            eng.backward_only(b)
        assert torch.equal(eng.model.flat, before), f"{what}: the weights moved"
        assert float(eng._g_flat.abs().max()) == 0.0, f"{what}: a partial gradient was kept"
    with pytest.raises(IndexError):
        eng.train_single_batch(cases["neighbour id"])
    assert float(eng._g_flat.abs().max()) == 0.0
    load_weights(eng, cmn_params(case, g, 0))
    eng.load_optimizer_state(0)
    # an id beyond a row's length is padding and is never read as a neighbour
    loss, _, _ = eng.backward_only(broken(3, 0, U, good[3].shape[1] - 1) if good[4][0] < good[3].shape[1] else good)
    assert_scalar_close(loss, g["losses"][0], what="loss with garbage in the padding")
    with pytest.raises(ValueError):
        eng.train_single_batch(good[:6])
    with pytest.raises(ValueError):
        eng.train_single_batch((good[0], good[1][:-1]) + good[2:])
    loss = eng.train_single_batch(good)
    assert_scalar_close(loss, g["losses"][0], what="loss after the errors")


def test_momentum_sweep_against_torch(hip_device):
    """hiprec_opt_dense_step(HIPREC_OPT_RMSPROP_MOMENTUM) alone on a random flat buffer, three steps, against
    torch.optim.RMSprop(momentum=0.9) on the CPU.  In the IEEE build (correctly rounded sqrt / division, op for op) the
    weights agree to an ulp or two; the default build (v_rcp_f32 / v_sqrt_f32, 1 ulp each) is held to REL of the update."""
    from beta_recsys_amd import _lib
    from beta_recsys_amd.mf import _new_stats

    lib, dev = _lib.load(), hip_device
    n, lr, mu = 4099, 1e-2, 0.9                       # not a multiple of 4: the scalar tail runs too
    gen = torch.Generator().manual_seed(5)
    w0 = torch.randn(n, generator=gen)
    p = torch.nn.Parameter(w0.clone())
    ref = torch.optim.RMSprop([p], lr=lr, momentum=mu)
    w, m, v = w0.clone().to(dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    stats = _new_stats(dev, mu, 0.99)
    for step in range(3):
        gr = torch.randn(n, generator=gen) * (10.0 ** float(step - 1))
        before = p.detach().clone()
        p.grad = gr.clone()
        ref.step()
        g_dev = gr.clone().to(dev)
        _lib.check(lib.hiprec_stats_advance_step(_lib.ptr(stats), _lib.stream_ptr(dev)))
        _lib.check(lib.hiprec_opt_dense_step(_lib.OPT_RMSPROP_MOMENTUM, _lib.ptr(w), _lib.ptr(g_dev), _lib.ptr(m),
                                             _lib.ptr(v), n, lr, mu, 0.99, 1e-8, _lib.ptr(stats), None, -1,
                                             _lib.stream_ptr(dev)))
        torch.cuda.synchronize()
        assert float(g_dev.abs().max()) == 0.0
        st = ref.state[p]
        upd = float((p.detach() - before).abs().max())
        err_w = float((w.cpu() - p.detach()).abs().max())
        err_m = float((m.cpu() - st["momentum_buffer"]).abs().max() / st["momentum_buffer"].abs().max())
        err_v = float((v.cpu() - st["square_avg"]).abs().max() / st["square_avg"].abs().max())
        print(f"step {step}: |dw| {err_w:.3e} (update {upd:.3e}), buf {err_m:.3e}, square_avg {err_v:.3e}")
        assert err_v <= 4 * EPS32
        if IEEE_BUILD:
            assert err_w <= 2 * EPS32 * float(p.detach().abs().max()) and err_m <= 4 * EPS32
        else:
            assert err_w <= REL * upd + 4 * EPS32 * float(p.detach().abs().max()) and err_m <= REL


def test_cmn_suite_against_the_ieee_arithmetic_build(hip_device):
    """The step, trajectory and momentum-sweep tests again against libhiprec_ieee.so in a fresh interpreter (HIPREC_LIB
    selects the library), as the MF / NCF parity files do."""
    import subprocess
    import sys

    from beta_recsys_amd import _lib

    if IEEE_BUILD:
        return
    ieee = os.path.join(os.path.dirname(_lib.LIB_PATH), "libhiprec_ieee.so")
    assert os.path.exists(ieee), "libhiprec_ieee.so is missing: run __graft_entry__.build()"
    out = subprocess.run(
        [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k",
         "step_matches_reference or trajectory_matches_reference or momentum_sweep"],
        env=dict(os.environ, HIPREC_LIB="libhiprec_ieee.so"), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout
