"""Host-side checks of the UltraGCN mirror that need no GPU: construction parity with the reference (ug_init golden),
the sparse Omega construction, argument validation of the new C entry points, the compat table."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

import ultragcn_numpy as ug
from helpers import load_golden
from test_oracle_golden_ultragcn import assert_tables_match, ug_train_mat


def model_config(g, tag, **over):
    import scipy.sparse as sp

    U, I, D, K, seed = (int(x) for x in g[f"{tag}/meta"])
    cfg = dict(n_users=U, n_items=I, emb_dim=D, ii_neighbor_num=K, train_mat=sp.csr_matrix(ug_train_mat(g, f"{tag}/")),
               constraint_mat={"beta_uD": g[f"{tag}/beta_u"], "beta_iD": g[f"{tag}/beta_i"]}, **ug.DEFAULT_HP)
    cfg.update(over)
    return cfg, seed


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_construction_matches_reference(tag):
    """Same initial weights bit for bit for the same torch seed, the reference's state_dict keys in its order, and the
    flat layout [user_embeds | item_embeds]; the Omega tables built at construction match the reference's."""
    import beta_recsys_amd as hp

    g = load_golden("ug_init")
    cfg, seed = model_config(g, tag)
    torch.manual_seed(seed)
    m = quiet(hp.UltraGCN, cfg)
    sd = m.state_dict()
    assert list(sd) == ["user_embeds.weight", "item_embeds.weight"]
    for k in sd:
        assert np.array_equal(sd[k].numpy(), g[f"{tag}/w/{k}"]), k
    U, I, D = m.user_num, m.item_num, m.emb_dim
    assert m.flat.numel() == (U + I) * D
    assert np.array_equal(m.flat[:U * D].view(U, D).numpy(), g[f"{tag}/w/user_embeds.weight"])
    assert np.array_equal(m.flat[U * D:].view(I, D).numpy(), g[f"{tag}/w/item_embeds.weight"])
    assert m.ii_neighbor_mat.dtype == torch.int64 and m.ii_constraint_mat.dtype == torch.float32
    assert_tables_match(m.ii_neighbor_mat.numpy(), m.ii_constraint_mat.numpy(), g[f"{tag}/ii_neighbor_mat"],
                        g[f"{tag}/ii_constraint_mat"], ug.omega_matrix(ug_train_mat(g, f"{tag}/")), f"ug_init {tag}")
    t = m.tables()
    assert (t.n_users, t.n_items, t.dim) == (U, I, D) and t.item_embeds - t.user_embeds == 4 * U * D


@pytest.mark.parametrize("case", ["ug_adam", "ug_sgd_d100", "ug_rmsprop_hot"])
def test_get_ii_constraint_mat_matches_reference(case):
    """The sparse construction (never an I x I dense matrix) against the tables the reference built from the same
    interactions: sims to 1e-6, ids wherever torch.topk's order is determined."""
    import scipy.sparse as sp

    import beta_recsys_amd as hp

    g = load_golden(case)
    M = ug_train_mat(g)
    K = int(g["meta"][5])
    nbr, sim = quiet(hp.get_ii_constraint_mat, sp.csr_matrix(M), K)
    assert tuple(nbr.shape) == (M.shape[1], K) and nbr.dtype == torch.int64 and sim.dtype == torch.float32
    assert_tables_match(nbr.numpy(), sim.numpy(), g["ii_neighbor_mat"], g["ii_constraint_mat"], ug.omega_matrix(M), case)
    # the diagonal-free variant against the restatement (the reference's own call never uses it)
    nbr0, sim0 = quiet(hp.get_ii_constraint_mat, sp.csr_matrix(M), K, True)
    ref_nbr0, ref_sim0 = ug.ii_constraint_tables(M, K, True)
    assert_tables_match(nbr0.numpy(), sim0.numpy(), ref_nbr0, ref_sim0, ug.omega_matrix(M, True), case + " diag 0")
    assert not (nbr0.numpy() == np.arange(M.shape[1])[:, None])[sim0.numpy() != 0].any()


def test_rows_with_few_neighbours_are_padded_with_zero_sims():
    import scipy.sparse as sp

    import beta_recsys_amd as hp

    M = np.zeros((3, 4), dtype=np.float32)
    M[0, 0] = M[0, 1] = M[1, 2] = M[2, 3] = M[2, 2] = 1
    nbr, sim = quiet(hp.get_ii_constraint_mat, sp.csr_matrix(M), 3)
    ref_nbr, ref_sim = ug.ii_constraint_tables(M, 3)
    assert np.allclose(sim.numpy(), ref_sim, rtol=1e-6)
    assert ((sim.numpy() == 0).sum(axis=1) == [1, 1, 1, 1]).all()
    assert int(nbr.min()) >= 0 and int(nbr.max()) < 4


def test_w2_not_positive_raises():
    import beta_recsys_amd as hp

    g = load_golden("ug_init")
    for w2 in (0.0, -1.0):
        cfg, _ = model_config(g, "a", w2=w2)
        with pytest.raises(ValueError, match="w2"):
            quiet(hp.UltraGCN, cfg)


def test_precomputed_tables_are_taken_from_the_config():
    import beta_recsys_amd as hp

    g = load_golden("ug_init")
    cfg, _ = model_config(g, "a", ii_neighbor_mat=g["a/ii_neighbor_mat"], ii_constraint_mat=g["a/ii_constraint_mat"])
    del cfg["train_mat"]
    m = quiet(hp.UltraGCN, cfg)
    assert np.array_equal(m.ii_neighbor_mat.numpy(), g["a/ii_neighbor_mat"])
    assert np.array_equal(m.ii_constraint_mat.numpy(), g["a/ii_constraint_mat"])
    bad = g["a/ii_neighbor_mat"].copy()
    bad[0, 0] = m.item_num
    cfg["ii_neighbor_mat"] = bad
    with pytest.raises(ValueError):
        quiet(hp.UltraGCN, cfg)
    om = m.get_omegas([0, 1], [1, 2], [[0, 1, 2], [3, 4, 5]])
    wp, wn = ug.omegas(ug.DEFAULT_HP, g["a/beta_u"], g["a/beta_i"], np.array([0, 1]), np.array([1, 2]),
                       np.array([[0, 1, 2], [3, 4, 5]]))
    assert np.allclose(om.numpy(), np.concatenate([wp, wn.reshape(-1)]), rtol=1e-6)


def test_no_cpu_path():
    import beta_recsys_amd as hp

    g = load_golden("ug_init")
    cfg, _ = model_config(g, "a")
    m = quiet(hp.UltraGCN, cfg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict([0], [0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m([0], [0], [[1, 2]])


def test_new_entry_points_validate_before_touching_the_gpu():
    """Argument validation happens before any HIP call: every new entry point returns -1 on the CPU box."""
    from beta_recsys_amd import _lib

    lib = _lib.load()
    ws_bytes = lib.hiprec_sumsq_workspace_bytes()
    assert ws_bytes >= 8 * 2049
    assert lib.hiprec_sumsq(None, 16, None, ws_bytes, None) == -1 and b"NULL" in lib.hiprec_last_error()
    assert lib.hiprec_sumsq(None, -1, None, 0, None) == -1
    buf = (ctypes.c_double * 4)()
    assert lib.hiprec_sumsq(None, 0, buf, 32, None) == -1 and b"workspace" in lib.hiprec_last_error()
    assert lib.hiprec_decay_grad(None, None, 8, 0.1, None) == -1
    assert lib.hiprec_decay_grad(None, None, -8, 0.1, None) == -1
    args = (1, None, None, None, None, 4, 0.1, 0.9, 0.999, 1e-8, None, None, 1e-4)
    assert lib.hiprec_opt_dense_step_decay(*args, None, ws_bytes, None) == -1
    assert lib.hiprec_opt_dense_step_decay(*args, buf, 32, None) == -1 and b"workspace" in lib.hiprec_last_error()
    assert lib.hiprec_opt_dense_step_decay(*args, buf, ws_bytes, None) == -1   # NULL w / g / stats
    t = _lib.UltraGcnTables(0, 0, 4, 5, 8, 0)
    p = _lib.UltraGcnParams(None, None, None, None, 0, 1e-7, 1.0, 1e-7, 1.0, 200.0, 1e-4, 1e-3)
    grad = lambda tw, tg, pp, n_neg=2: lib.hiprec_ultragcn_grad(  # noqa: E731
        ctypes.byref(tw), ctypes.byref(tg), ctypes.byref(pp), None, None, None, 3, n_neg, None, None, None, 0, None)
    assert grad(t, t, p) == -1 and b"NULL tensor pointer" in lib.hiprec_last_error()
    ok = _lib.UltraGcnTables(64, 128, 4, 5, 8, 0)        # non-NULL (never dereferenced: validation fails first)
    assert grad(ok, _lib.UltraGcnTables(64, 128, 4, 5, 300, 0), p) == -1 and b"dim" in lib.hiprec_last_error()
    assert grad(ok, _lib.UltraGcnTables(64, 128, 4, 6, 8, 0), p) == -1 and b"shapes differ" in lib.hiprec_last_error()
    assert grad(ok, ok, p) == -1 and b"beta" in lib.hiprec_last_error()
    p2 = _lib.UltraGcnParams(64, 64, None, None, 3, 1e-7, 1.0, 1e-7, 1.0, 200.0, 1e-4, 1e-3)
    assert grad(ok, ok, p2) == -1 and b"neighbour" in lib.hiprec_last_error()
    p3 = _lib.UltraGcnParams(64, 64, None, None, 0, 1e-7, 0.0, 1e-7, 1.0, 200.0, 1e-4, 1e-3)
    assert grad(ok, ok, p3) == -1 and b"w2" in lib.hiprec_last_error()
    p4 = _lib.UltraGcnParams(64, 64, None, None, 0, 1e-7, 1.0, 1e-7, 1.0, 200.0, 1e-4, 1e-3)
    assert grad(ok, ok, p4) == -1 and b"NULL stats" in lib.hiprec_last_error()
    assert grad(ok, ok, p4, n_neg=0) == -1
    assert lib.hiprec_ultragcn_predict(ctypes.byref(t), None, None, 3, None, None, None) == -1
    assert lib.hiprec_ultragcn_predict(ctypes.byref(ok), None, None, 3, None, None, None) == -1
    assert lib.hiprec_ultragcn_predict(ctypes.byref(ok), None, None, -3, None, None, None) == -1
    epoch = lambda n, b, n_neg, fw: lib.hiprec_ultragcn_epoch(  # noqa: E731
        ctypes.byref(ok), ctypes.byref(ok), ctypes.byref(p4), None, None, None, n, b, n_neg, 1, 0.1, 0.9, 0.999, 1e-8, fw,
        fw, None, None, 52, None, 0, None, None, 0, None)
    assert epoch(10, 0, 2, 64) == -1
    assert epoch(10, 4, 0, 64) == -1
    assert epoch(10, 4, 2, None) == -1 and b"flat buffers" in lib.hiprec_last_error()
    assert epoch(10, 4, 2, 64) == -1     # NULL sums-of-squares workspace
    with pytest.raises(_lib.HiprecError):
        _lib.check(-1)


def test_compat_table_routes_the_reference_module():
    from beta_recsys_amd import compat, ultragcn

    assert compat.MIRRORS["beta_rec.models.ultragcn"] == "ultragcn"
    for name in ("UltraGCN", "UltraGCNEngine", "get_ii_constraint_mat"):
        assert hasattr(ultragcn, name)
