"""Pin tests/ultragcn_numpy.py against golden vectors captured from the real reference's UltraGCNEngine by
``tools/gen_golden_ultragcn.py``.  CPU only."""
import numpy as np
import pytest

import ultragcn_numpy as ug
from helpers import REL, assert_scalar_close, assert_step_close, assert_tensor_close, copy_state, load_golden

CASES = ["ug_adam", "ug_sgd_d100", "ug_rmsprop_hot"]
KEYS = ug.KEYS
OPEN_SHARE_CAP = 0.10   # of a fixture's non-zero table entries (torch.topk leaves the order of ties open)


def ug_params(g, prefix):
    return {k: g[f"{prefix}/{k}"].astype(np.float32).copy() for k in KEYS}


def ug_hp(g):
    return {str(k): float(v) for k, v in zip(g["hp_names"], g["hp"])}


def ug_consts(g):
    """(hp, beta_u, beta_i, neighbour ids, sims) of a fixture."""
    return ug_hp(g), g["beta_u"], g["beta_i"], g["ii_neighbor_mat"], g["ii_constraint_mat"]


def ug_train_mat(g, prefix=""):
    U, I = (int(x) for x in g[prefix + "meta"][:2])
    M = np.zeros((U, I), dtype=np.float32)
    M[g[prefix + "train_users"], g[prefix + "train_items"]] = 1.0
    return M


def ug_opt_state(g, step, opt):
    st = ug.new_opt_state(ug_params(g, "w0"), opt)
    st["step"] = step
    if step > 0 and opt == "adam":
        st["exp_avg"], st["exp_avg_sq"] = ug_params(g, f"m{step}"), ug_params(g, f"v{step}")
    elif step > 0 and opt == "rmsprop":
        st["square_avg"] = ug_params(g, f"v{step}")
    return st


def ug_band(w_prev, st_prev, g_ref, opt, lr, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel * its scale of g_ref
    (Adam / RMSprop are ill-conditioned where |g| is not >> eps; see helpers.optimizer_band)."""
    outs = []
    for sign in (+1.0, -1.0):
        w = {k: v.copy() for k, v in w_prev.items()}
        st = copy_state(st_prev)
        g = {k: (g_ref[k] + np.float32(sign * rel * float(np.abs(g_ref[k]).max()))).astype(np.float32) for k in KEYS}
        ug.opt_step(w, g, st, opt, lr)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in KEYS}


def assert_tables_match(nbr, sim, ref_nbr, ref_sim, omega, what=""):
    """Rule for the Omega tables: sims (sorted, per row) to 1e-6 relative; ids equal wherever the reference's sim is
    non-zero and differs from both adjacent sims of its row and from the first excluded value (``torch.topk`` leaves
    the order of ties open, and the ids of zero-sim padding arbitrary).  Returns the share of the non-zero entries the
    rule leaves out, which may not exceed OPEN_SHARE_CAP."""
    nbr, sim, ref_nbr, ref_sim = (np.asarray(a) for a in (nbr, sim, ref_nbr, ref_sim))
    K = ref_sim.shape[1]
    assert nbr.shape == ref_nbr.shape and sim.shape == ref_sim.shape, f"{what}: table shapes"
    a, b = -np.sort(-sim.astype(np.float64), axis=1), -np.sort(-ref_sim.astype(np.float64), axis=1)
    assert np.all(np.abs(a - b) <= 1e-6 * np.abs(b)), f"{what}: sims differ by {np.abs(a - b).max():.3e}"
    srt = -np.sort(-np.asarray(omega), axis=1)
    excluded = srt[:, K] if srt.shape[1] > K else np.zeros(srt.shape[0], dtype=np.float32)
    left = np.concatenate([np.full((ref_sim.shape[0], 1), np.inf, dtype=np.float32), ref_sim[:, :-1]], axis=1)
    right = np.concatenate([ref_sim[:, 1:], excluded[:, None]], axis=1)
    nz = ref_sim != 0
    determined = nz & (ref_sim != left) & (ref_sim != right)
    assert np.array_equal(nbr[determined], ref_nbr[determined]), (
        f"{what}: {int((nbr[determined] != ref_nbr[determined]).sum())} neighbour ids differ where the order is determined")
    share = 1.0 - determined.sum() / max(1, nz.sum())
    assert share <= OPEN_SHARE_CAP, f"{what}: the rule leaves {share:.1%} of the non-zero entries unchecked"
    return share


@pytest.mark.parametrize("case", CASES)
def test_numpy_oracle_matches_reference(case):
    """Every step in isolation from the reference's own weights and optimizer state: loss, both gradients (the gamma
    term included), the new weights and the new moments."""
    g = load_golden(case)
    n_steps = int(g["meta"][6])
    opt, lr = str(g["optimizer"]), float(g["lr"])
    consts = ug_consts(g)
    for s in range(n_steps):
        w = ug_params(g, f"w{s}")
        st = ug_opt_state(g, s, opt)
        loss, grads = ug.ug_grads(w, g["users"][s], g["pos"][s], g["neg"][s], *consts)
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        g_ref = ug_params(g, f"g{s + 1}")
        for k in KEYS:
            assert_tensor_close(grads[k], g_ref[k], what=f"grad {k} step {s}")
        band = ug_band(w, st, g_ref, opt, lr)
        w_prev = {k: v.copy() for k, v in w.items()}
        ug.opt_step(w, grads, st, opt, lr)
        for k in KEYS:
            assert_step_close(w_prev[k], w[k], g[f"w{s + 1}/{k}"], band[k], what=f"weights {k} step {s}")
        nxt = ug_opt_state(g, s + 1, opt)
        for name in ("exp_avg", "exp_avg_sq", "square_avg"):
            if name in st:
                for k in KEYS:
                    assert_tensor_close(st[name][k], nxt[name][k], 4e-5, f"{name} {k} step {s}")


@pytest.mark.parametrize("case", CASES)
def test_fixtures_see_the_nonlinearity_and_every_term(case):
    """Scores spread over several units but stay inside |s| < 20 (where sigmoid().log() and -softplus(-s) agree far
    inside the tolerance); every user and item has an interaction; the hot fixture repeats (u, p) pairs."""
    g = load_golden(case)
    hp, bu, bi, nbr, sim = ug_consts(g)
    w = ug_params(g, "w0")
    users, pos, neg = g["users"][0], g["pos"][0], g["neg"][0]
    ids = np.concatenate([pos[:, None], neg, nbr[pos]], axis=1)
    s = np.einsum("bd,bkd->bk", w["user_embeds.weight"][users], w["item_embeds.weight"][ids])
    assert 2.0 < np.abs(s).max() < 20.0 and s.std() > 0.5
    M = ug_train_mat(g)
    assert M.sum(axis=0).min() >= 1 and M.sum(axis=1).min() >= 1
    assert np.isfinite(bu).all() and np.isfinite(bi).all()
    assert (sim != 0).any()
    if case == "ug_rmsprop_hot":
        pairs = set(zip(users.tolist(), pos.tolist()))
        assert len(pairs) <= 40 < len(users) / 4
        hits = np.bincount(neg.reshape(-1), minlength=M.shape[1])
        assert hits.max() > 5 * hits.mean() and hits.max() > 2 * len(users)      # hundreds of terms on one row
    if case == "ug_sgd_d100":
        assert hp["w4"] == 0.0 and neg.shape[1] % 2 == 1


@pytest.mark.parametrize("case", CASES)
def test_betas_and_omega_tables_match_reference(case):
    g = load_golden(case)
    M = ug_train_mat(g)
    bu, bi = ug.betas(M)
    assert np.array_equal(bu, g["beta_u"]) and np.array_equal(bi, g["beta_i"])
    K = int(g["meta"][5])
    nbr, sim = ug.ii_constraint_tables(M, K)
    share = assert_tables_match(nbr, sim, g["ii_neighbor_mat"], g["ii_constraint_mat"], ug.omega_matrix(M), case)
    print(f"{case}: {share:.2%} of the non-zero table entries left open by ties")


@pytest.mark.parametrize("case", CASES)
def test_reference_own_rounding_leaves_room(case):
    """The GPU tests hold an implementation to REL of a gradient's scale AGAINST THESE VECTORS.  That bound only means
    something while the reference's own fp32 rounding -- the distance of its gradient from the fp64 restatement's --
    stays well inside it: at most a third, so that an implementation summing in another order has two thirds left."""
    from helpers import float64_oracle, to64

    g = load_golden(case)
    worst = 0.0
    for s in range(int(g["meta"][6])):
        with float64_oracle(ug):
            _, g64 = ug.ug_grads(to64(ug_params(g, f"w{s}")), g["users"][s], g["pos"][s], g["neg"][s], *ug_consts(g))
        for k in KEYS:
            worst = max(worst, float(np.abs(g[f"g{s + 1}/{k}"] - g64[k]).max() / np.abs(g64[k]).max()))
    print(f"{case}: the reference's gradients are within {worst:.2e} of their scale of the exact ones")
    assert worst <= REL / 3


def test_trajectory_from_initial_weights():
    """All steps chained from w0 (the oracle's own state carried along) stay on the reference's path."""
    g = load_golden("ug_sgd_d100")
    w = ug_params(g, "w0")
    st = ug.new_opt_state(w, "sgd")
    n_steps = int(g["meta"][6])
    for s in range(n_steps):
        loss = ug.ug_train_step(w, st, (g["users"][s], g["pos"][s], g["neg"][s]), *ug_consts(g), "sgd", float(g["lr"]))
        assert_scalar_close(loss, g["losses"][s], 5e-5, what=f"loss step {s}")
    for k in KEYS:
        assert_tensor_close(w[k], g[f"w{n_steps}/{k}"], 5e-5, what=f"final {k}")


def test_fp64_restatement_is_the_same_function():
    """The restatement in fp64 (the yardstick of the large-shape GPU runs) agrees with its fp32 self."""
    from helpers import float64_oracle, to64

    g = load_golden("ug_adam")
    w = ug_params(g, "w0")
    loss32, g32 = ug.ug_grads(w, g["users"][0], g["pos"][0], g["neg"][0], *ug_consts(g))
    with float64_oracle(ug):
        loss64, g64 = ug.ug_grads(to64(w), g["users"][0], g["pos"][0], g["neg"][0], *ug_consts(g))
    assert g64["item_embeds.weight"].dtype == np.float64
    assert_scalar_close(loss32, loss64, what="loss")
    for k in KEYS:
        assert_tensor_close(g32[k], g64[k], what=k)
