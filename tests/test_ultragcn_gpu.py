"""GPU parity tests of UltraGCN (csrc/ultragcn.hip: the gradient kernel and the decay sweep): forward + loss + backward, the
full step and chained steps vs golden vectors from the real reference's UltraGCNEngine (tests/golden/ug_*.npz), and vs
the numpy restatement at the reference's default shape and at the paper's negative count."""
import contextlib
import io
import types

import numpy as np
import pytest
import torch

import ultragcn_numpy as ug
from helpers import REL, assert_on_trajectory, assert_scalar_close, assert_sgd_exact, assert_step_close
from helpers import assert_tensor_close, float64_oracle, load_golden, oracle_trajectory, to64
from test_oracle_golden_ultragcn import CASES, KEYS, ug_band, ug_consts, ug_opt_state, ug_params

pytestmark = pytest.mark.gpu


def make_engine(U, I, D, consts, optimizer="adam", lr=0.05, B=32):
    import beta_recsys_amd as hp

    hpv, bu, bi, nbr, sim = consts
    model = dict(n_users=U, n_items=I, emb_dim=D, batch_size=B, regs=[1e-5], optimizer=optimizer, lr=lr,
                 device_str="cuda:0", constraint_mat={"beta_uD": bu, "beta_iD": bi}, ii_neighbor_num=nbr.shape[1],
                 ii_neighbor_mat=nbr, ii_constraint_mat=sim, **hpv)
    with contextlib.redirect_stdout(io.StringIO()):
        return hp.UltraGCNEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_test_runs"}})


def golden_engine(g):
    U, I, D, B = (int(x) for x in g["meta"][:4])
    return make_engine(U, I, D, ug_consts(g), str(g["optimizer"]), float(g["lr"]), B)


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in w.items()})


def get_weights(eng):
    return {k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()}


def load_opt_state(eng, st):
    eng.load_optimizer_state(st["step"], st.get("exp_avg"), st.get("exp_avg_sq", st.get("square_avg")))


def np_grads(grads):
    return {k: v.cpu().numpy() for k, v in grads.items()}


@pytest.mark.parametrize("case", CASES)
def test_step_matches_reference(hip_device, case):
    """Each step from the reference's own weights and optimizer state: loss, both gradients INCLUDING the gamma term,
    the updated weights and moments."""
    g = load_golden(case)
    n_steps = int(g["meta"][6])
    opt, lr = str(g["optimizer"]), float(g["lr"])
    eng = golden_engine(g)
    for s in range(n_steps):
        batch = (g["users"][s], g["pos"][s], g["neg"][s])
        w0, st0 = ug_params(g, f"w{s}"), ug_opt_state(g, s, opt)
        load_weights(eng, w0)
        load_opt_state(eng, st0)
        loss, grads = eng.backward_only(batch)
        print(f"{case} step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        g_ref = ug_params(g, f"g{s + 1}")
        for k in KEYS:
            got = np_grads(grads)[k]
            print(f"  grad {k}: max err {np.abs(got - g_ref[k]).max():.3e} of scale {np.abs(g_ref[k]).max():.3e}")
            assert_tensor_close(got, g_ref[k], what=f"grad {k} step {s}")
        assert float(eng._g_flat.abs().max()) == 0.0
        assert np.array_equal(get_weights(eng)["item_embeds.weight"], w0["item_embeds.weight"])
        # the model's own forward: the same loss, no gradient kept
        assert_scalar_close(float(eng.model(*batch)), g["losses"][s], what=f"forward step {s}")
        # the full step
        load_opt_state(eng, st0)
        loss = eng.train_single_batch(batch)
        assert_scalar_close(loss, g["losses"][s], what=f"loss (step) {s}")
        band = ug_band(w0, st0, g_ref, opt, lr)
        w1 = get_weights(eng)
        for k in KEYS:
            assert_step_close(w0[k], w1[k], g[f"w{s + 1}/{k}"], band[k], what=f"weights {k} step {s}")
        nxt = ug_opt_state(g, s + 1, opt)
        views = {"exp_avg": eng.optimizer.exp_avg, "exp_avg_sq": eng.optimizer.exp_avg_sq}
        for name, ref_name in (("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq" if opt == "adam" else "square_avg")):
            if views[name] is None:
                continue
            got = {k: v.cpu().numpy() for k, v in eng.model.views(views[name]).items()}
            for k in KEYS:
                assert_tensor_close(got[k], nxt[ref_name][k], REL if name == "exp_avg" else 2 * REL,
                                    f"{name} {k} step {s}")   # linear / quadratic in the gradient
        assert float(eng._g_flat.abs().max()) == 0.0, "the optimizer sweep leaves the gradient cleared"


@pytest.mark.parametrize("case", CASES)
def test_trajectory_matches_reference(hip_device, case):
    """All steps chained from w0, the sums of squares handed from sweep to step.  SGD: every element within 1e-5 of the
    trajectory's update; Adam / RMSprop: every element inside the oracle's perturbed-gradient envelope around the
    reference's end point, zero outliers."""
    g = load_golden(case)
    n_steps = int(g["meta"][6])
    opt, lr = str(g["optimizer"]), float(g["lr"])
    consts = ug_consts(g)
    eng = golden_engine(g)
    w0 = ug_params(g, "w0")
    load_weights(eng, w0)
    batches = [(g["users"][s], g["pos"][s], g["neg"][s]) for s in range(n_steps)]
    for s, b in enumerate(batches):
        loss = eng.train_single_batch(b)
        print(f"{case} chained step {s}: loss {loss!r} vs {float(g['losses'][s])!r}")
        if opt == "sgd" or s == 0:   # later Adam / RMSprop losses are held through the weights' envelope below
            assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
    ref_end = ug_params(g, f"w{n_steps}")
    if opt == "sgd":
        assert_sgd_exact(get_weights(eng), ref_end, w0, "final weights")
        return
    _, env, upd = oracle_trajectory(
        w0, batches, lambda w, b: ug.ug_grads(w, b[0], b[1], b[2], *consts)[1],
        lambda w, gr, st: ug.opt_step(w, gr, st, opt, lr), lambda w: ug.new_opt_state(w, opt))
    assert_on_trajectory(get_weights(eng), ref_end, env, upd, f"{case} trajectory")


@pytest.mark.parametrize("case", CASES)
def test_predict_matches_reference(hip_device, case):
    g = load_golden(case)
    eng = golden_engine(g)
    load_weights(eng, ug_params(g, f"w{int(g['meta'][6])}"))
    scores = eng.model.predict(g["predict_users"], g["predict_items"])
    assert scores.dtype == torch.float32 and tuple(scores.shape) == (len(g["predict_users"]),)
    assert_tensor_close(scores.cpu().numpy(), g["predict_scores"], what="predict")
    with pytest.raises(IndexError):
        eng.model.predict([0, int(g["meta"][0])], [0, 0])
    with pytest.raises(IndexError):
        eng.model.predict([0, 0], [0, -1])
    assert np.isfinite(eng.model.predict([0], [0]).cpu().numpy()).all()     # usable after the error


def test_out_of_range_ids_raise_and_leave_the_tables_untouched(hip_device):
    g = load_golden("ug_adam")
    U, I, D, B, N = (int(x) for x in g["meta"][:5])
    eng = golden_engine(g)
    load_weights(eng, ug_params(g, "w0"))
    users, pos, neg = g["users"][0].copy(), g["pos"][0].copy(), g["neg"][0].copy()
    before = eng.model.flat.clone()
    for what, (du, dp, dn) in {"user": (U, None, None), "pos": (None, I, None), "neg": (None, None, I),
                               "negative id": (None, None, -1)}.items():
        u2, p2, n2 = users.copy(), pos.copy(), neg.copy()
        if du is not None:
            u2[3] = du
        if dp is not None:
            p2[5] = dp
        if dn is not None:
            n2[7, N - 1] = dn
        with pytest.raises(IndexError):
            eng.train_single_batch((u2, p2, n2))
        assert torch.equal(eng.model.flat, before), f"{what}: the tables moved"
        assert float(eng._g_flat.abs().max()) == 0.0
        with pytest.raises(IndexError):
            eng.backward_only((u2, p2, n2))
    with pytest.raises(ValueError):
        eng.train_single_batch((users, pos[:-1], neg))
    with pytest.raises(ValueError):
        eng.train_single_batch((users, pos, neg.reshape(-1)))
    with pytest.raises(ValueError):
        eng.train_single_batch(([], [], np.zeros((0, N), dtype=np.int64)))
    # the engine keeps working after the errors
    loss = eng.backward_only((users, pos, neg))[0]
    assert_scalar_close(loss, g["losses"][0], what="loss after the errors")


def planted_frame(U, I, per_user, seed):
    rng = np.random.default_rng(seed)
    users = np.repeat(np.arange(U), per_user)
    items = np.concatenate([rng.choice(I, per_user, replace=False) for _ in range(U)])
    items[:I] = np.arange(I)                      # every item occurs
    return users, items


def constants_for(users, items, U, I, K):
    """beta vectors (base_data.py:424-428) and the Omega tables through the package's own sparse construction."""
    import scipy.sparse as sp

    import beta_recsys_amd as hp

    M = sp.csr_matrix((np.ones(len(users), dtype=np.float32), (users, items)), shape=(U, I))
    M.data[:] = 1.0
    items_D = np.asarray(M.sum(axis=0)).reshape(-1)
    users_D = np.asarray(M.sum(axis=1)).reshape(-1)
    bu = (np.sqrt(users_D + 1) / users_D).astype(np.float32)
    bi = (1 / np.sqrt(items_D + 1)).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        nbr, sim = hp.get_ii_constraint_mat(M, K)
    return dict(ug.DEFAULT_HP), bu, bi, nbr.numpy(), sim.numpy()


def test_train_an_epoch_through_the_multi_negative_loader(hip_device):
    """data.instance_mul_neg_loader -> train_an_epoch (one C call for the epoch) equals stepping the same batches one
    by one; the epoch sum goes to the writer, the LAST batch's loss is printed."""
    import pandas as pd

    from beta_recsys_amd import data as hip_data

    U, I, D, B, N, K = 60, 50, 32, 64, 6, 4
    users, items = planted_frame(U, I, 5, 1)
    consts = constants_for(users, items, U, I, K)
    frame = types.SimpleNamespace(train=pd.DataFrame({"col_user": users, "col_item": items}), n_users=U, n_items=I)
    with contextlib.redirect_stdout(io.StringIO()):
        loader = hip_data.instance_mul_neg_loader(frame, B, hip_device, N, seed=5)
    assert len(loader) == (len(users) + B - 1) // B and len(users) % B != 0      # a short last batch
    engines = [make_engine(U, I, D, consts, "adam", 0.01, B) for _ in range(2)]
    w0 = get_weights(engines[0])
    w0 = {k: v * 300.0 for k, v in w0.items()}
    for e in engines:
        load_weights(e, w0)
    torch.manual_seed(77)
    batches = [tuple(t.clone() for t in b) for b in loader]
    assert tuple(batches[0][2].shape) == (B, N)
    losses = [engines[0].train_single_batch(b) for b in batches]
    torch.manual_seed(77)                                           # the same device-side permutation
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        engines[1].train_an_epoch(loader, 4)
    tag, total, epoch = engines[1].writer.scalars[-1]
    assert (tag, epoch) == ("model/loss", 4)
    assert_scalar_close(total, sum(losses), REL, "epoch loss sum")
    assert_scalar_close(float(out.getvalue().strip().rsplit("Loss ", 1)[1]), losses[-1], REL, "printed last loss")
    # the two runs differ only in the order their float atomics arrived: inside the legal-trajectory envelope
    np_batches = [tuple(t.cpu().numpy() for t in b) for b in batches]
    w_ref, env, upd = oracle_trajectory(
        w0, np_batches, lambda w, b: ug.ug_grads(w, b[0], b[1], b[2], *consts)[1],
        lambda w, gr, st: ug.opt_step(w, gr, st, "adam", 0.01), lambda w: ug.new_opt_state(w, "adam"))
    assert_on_trajectory(get_weights(engines[0]), w_ref, env, upd, "stepped")
    assert_on_trajectory(get_weights(engines[1]), w_ref, env, upd, "epoch")
    # a plain iterable of batches takes the same path
    load_weights(engines[1], w0)
    engines[1].load_optimizer_state(0)
    with contextlib.redirect_stdout(io.StringIO()):
        engines[1].train_an_epoch(np_batches, 5)
    assert_scalar_close(engines[1].writer.scalars[-1][1], sum(losses), REL, "epoch loss sum (iterable)")
    assert_on_trajectory(get_weights(engines[1]), w_ref, env, upd, "epoch (iterable)")


@pytest.mark.parametrize("n_neg,optimizer", [(20, "adam"), (300, "sgd")])
def test_reference_default_shape_vs_restatement(hip_device, n_neg, optimizer):
    """ML-100K tables (943 x 1682), D 64, B 1000, K 10, ultragcn_default.json weights, at the default negative count and
    at the paper's: loss and gradients against the restatement evaluated in fp64 (the exact value), one full step
    against the fp32 restatement."""
    U, I, D, B, K = 943, 1682, 64, 1000, 10
    users_f, items_f = planted_frame(U, I, 20, n_neg)
    consts = constants_for(users_f, items_f, U, I, K)
    lr = 0.05 if optimizer == "sgd" else 1e-3
    torch.manual_seed(n_neg)
    eng = make_engine(U, I, D, consts, optimizer, lr, B)
    w = {k: (v * 500.0).astype(np.float32) for k, v in get_weights(eng).items()}
    load_weights(eng, w)
    rng = np.random.default_rng(n_neg)
    pick = rng.integers(0, len(users_f), B)
    batch = (users_f[pick], items_f[pick], rng.integers(0, I, (B, n_neg)))
    with float64_oracle(ug):
        loss64, g64 = ug.ug_grads(to64(w), *batch, *consts)
    loss, grads = eng.backward_only(batch)
    print(f"N={n_neg}: loss {loss!r} vs exact {loss64!r}")
    assert_scalar_close(loss, loss64, what="loss")
    for k in KEYS:
        got = np_grads(grads)[k]
        print(f"  grad {k}: max err {np.abs(got - g64[k]).max():.3e} of scale {np.abs(g64[k]).max():.3e}")
        assert_tensor_close(got, g64[k], what=f"grad {k}")
    st = ug.new_opt_state(w, optimizer)
    w_prev, st_prev = {k: v.copy() for k, v in w.items()}, ug.new_opt_state(w, optimizer)
    g32 = ug.ug_grads(w_prev, *batch, *consts)[1]
    loss_o = ug.ug_train_step(w, st, batch, *consts, optimizer, lr)
    eng.load_optimizer_state(0)
    assert_scalar_close(eng.train_single_batch(batch), loss_o, what="loss (step)")
    band = ug_band(w_prev, st_prev, g32, optimizer, lr)
    got = get_weights(eng)
    for k in KEYS:
        assert_step_close(w_prev[k], got[k], w[k], band[k], what=f"weights {k}")


def test_checkpoint_round_trip(hip_device, tmp_path):
    """save_checkpoint / resume_checkpoint through the base class: the reference's state_dict file, plus the optional
    optimizer state; a resumed engine continues like the one that wrote the file."""
    g = load_golden("ug_adam")
    consts = ug_consts(g)
    eng = golden_engine(g)
    w0 = ug_params(g, "w0")
    load_weights(eng, w0)
    batches = [(g["users"][s], g["pos"][s], g["neg"][s]) for s in range(3)]
    eng.train_single_batch(batches[0])
    path = str(tmp_path / "ultragcn.model")
    eng.save_checkpoint(path, optimizer_state=True)
    sd = torch.load(path, map_location="cpu")
    assert list(sd) == ["user_embeds.weight", "item_embeds.weight"]
    other = golden_engine(g)
    with contextlib.redirect_stdout(io.StringIO()):
        other.resume_checkpoint(path, optimizer_state=True)
    assert torch.equal(other.model.flat, eng.model.flat)
    assert torch.equal(other.optimizer.exp_avg, eng.optimizer.exp_avg)
    assert torch.equal(other.optimizer.exp_avg_sq, eng.optimizer.exp_avg_sq)
    losses = [[e.train_single_batch(b) for b in batches[1:]] for e in (eng, other)]
    for a, b in zip(losses[0], losses[1]):
        assert_scalar_close(b, a, REL, "loss after resume")
    _, env, upd = oracle_trajectory(
        w0, batches, lambda w, b: ug.ug_grads(w, b[0], b[1], b[2], *consts)[1],
        lambda w, gr, st: ug.opt_step(w, gr, st, "adam", float(g["lr"])), lambda w: ug.new_opt_state(w, "adam"))
    assert_on_trajectory(get_weights(other), ug_params(g, "w3"), env, upd, "resumed trajectory")
