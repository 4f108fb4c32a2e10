"""Host-side logic of the SGL mirror (no GPU): config validation, initial weights, the numpy replay of the reference's
draws through the mirror's own ``draw_keep``, the symmetric CSR structure and the reference-dict conversion, the ctypes
plan layout, and the defects the restatement must be able to see."""
import contextlib
import ctypes
import io
import types

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import sgl_numpy as sx
from helpers import REL, float64_oracle, load_golden, to64
from test_oracle_golden_sgl import CASES, KEYS, n_refreshes, recorded_coo, recorded_subs, reference_dict, replayed_keeps
from test_oracle_golden_sgl import sgl_batch, sgl_graph, sgl_hp, sgl_meta, sgl_params

MIN_MARGIN = 10.0


def adj_matrix(g):
    rows, cols, vals, N = sgl_graph(g)
    return sp.csr_matrix((vals, (rows, cols)), shape=(N, N))


def model_config(g, **over):
    m, hp = sgl_meta(g), sgl_hp(g)
    cfg = dict(n_users=m["U"], n_items=m["I"], emb_dim=m["D"], n_layers=m["L"], regs=hp["regs"], ssl_reg=hp["ssl_reg"],
               ssl_temp=hp["ssl_temp"], ssl_mode=hp["ssl_mode"], ssl_ratio=hp["ssl_ratio"], aug_type=m["aug_type"],
               is_subgraph=True, pretrain=m["pretrain"], norm_adj=adj_matrix(g), optimizer=str(g["optimizer"]),
               lr=float(g["lr"]), device_str="cpu", batch_size=m["B"])
    cfg.update(over)
    return cfg


def make_engine(g, **over):
    import beta_recsys_amd as hp

    with contextlib.redirect_stdout(io.StringIO()):
        return hp.SGLEngine({"model": model_config(g, **over), "system": {"run_dir": "/tmp/hiprec_test_runs"}})


def loader_of(g, users=None, items=None):
    users = g["inter_user"] if users is None else users
    items = g["inter_item"] if items is None else items
    return types.SimpleNamespace(dataset=types.SimpleNamespace(user_tensor=torch.from_numpy(np.asarray(users)),
                                                               pos_item_tensor=torch.from_numpy(np.asarray(items))))


def test_config_is_validated():
    g = load_golden("sgl_both_edge_adam")
    eng = make_engine(g)
    assert list(eng.model.state_dict()) == list(KEYS)
    for over, text in (({"ssl_mode": "merge"}, "merge"), ({"ssl_mode": "sideways"}, "Invalid ssl_mode"),
                       ({"emb_dim": 257}, "emb_dim"), ({"emb_dim": 0}, "emb_dim"), ({"n_layers": 7}, "n_layers"),
                       ({"ssl_temp": 0.0}, "ssl_temp"), ({"aug_type": 3}, "aug_type"), ({"sub_rng": "torch"}, "sub_rng")):
        with pytest.raises(ValueError, match=text):
            make_engine(g, **over)
    users, pos, neg = sgl_batch(g, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP path"):
        eng.train_single_batch(reference_dict(g, 0), (users, pos, neg))
    with pytest.raises(ValueError, match="expected"):
        make_engine(g, norm_adj=sp.identity(5, format="csr")).model.graph()


def test_repeated_pairs_are_rejected():
    g = load_golden("sgl_both_edge_adam")
    m = sgl_meta(g)
    from beta_recsys_amd.sgl import symmetric_structure

    eu, ei = g["inter_user"], g["inter_item"]
    with pytest.raises(ValueError, match="repeated"):
        symmetric_structure(np.append(eu, eu[3]), np.append(ei, ei[3]), m["U"], m["I"])
    with pytest.raises(ValueError, match="outside"):
        symmetric_structure(np.append(eu, m["U"]), np.append(ei, 0), m["U"], m["I"])
    eng = make_engine(g)
    with pytest.raises(ValueError, match="repeated"):
        eng._loader_structure(loader_of(g, np.append(eu, eu[3]), np.append(ei, ei[3])))


@pytest.mark.parametrize("case", ["sgl_both_edge_adam", "sgl_user_walk_sgd"])
def test_same_seed_gives_the_references_initial_weights(case):
    g = load_golden(case)
    torch.manual_seed(int(g["torch_seed"]))
    sd = make_engine(g).model.state_dict()
    assert list(sd) == list(KEYS)
    for k in KEYS:
        assert np.array_equal(sd[k].numpy(), g[f"w0/{k}"]), k


@pytest.mark.parametrize("case", CASES)
def test_the_mirrors_numpy_draws_are_the_references(case):
    """``sub_rng = "numpy"``: the mirror's own draw_keep under the fixture's numpy seed gives the kept sets of the
    reference's sub-matrices, refresh after refresh (the restated replay is held to the recorded matrices in
    test_oracle_golden_sgl.py)."""
    g = load_golden(case)
    m = sgl_meta(g)
    want = replayed_keeps(g)
    eng = make_engine(g)
    np.random.seed(int(g["numpy_seed"]))
    for r in range(n_refreshes(g)):
        got = eng.draw_keep(g["inter_user"].size)
        for v in range(2):
            for l in range(max(m["L"], 1)):
                assert np.array_equal(got[v][l].numpy(), want[r][v][l]), f"refresh {r} view {v} layer {l}"


def test_node_dropout_draws_int_of_n_times_ratio():
    g = load_golden("sgl_both_edge_adam")
    m, hp = sgl_meta(g), sgl_hp(g)
    eng = make_engine(g, aug_type=0)
    np.random.seed(3)
    got = eng.draw_keep(g["inter_user"].size)
    np.random.seed(3)
    want = sx.keep_sets(g["inter_user"].size, m["U"], m["I"], 0, hp["ssl_ratio"], m["L"])
    for v in range(2):
        ku, ki = got[v][0]
        assert np.array_equal(ku.numpy(), want[v][0][0]) and np.array_equal(ki.numpy(), want[v][0][1])
        assert int((ku == 0).sum()) == int(m["U"] * hp["ssl_ratio"]) and int((ki == 0).sum()) == int(m["I"] * hp["ssl_ratio"])
    # ssl_ratio 0 or is_subgraph false: nothing is drawn and nothing dropped
    state = np.random.get_state()[1].copy()
    assert make_engine(g, ssl_ratio=0.0).draw_keep(10)[0][0] is None
    assert make_engine(g, is_subgraph=False).draw_keep(10)[1][0] is None
    assert np.array_equal(np.random.get_state()[1], state)


def test_structure_and_reference_dict_conversion():
    """The symmetric CSR holds every interaction twice with one interaction number for both directions; the reference's
    dict becomes one structure over the union of its coordinates with every view's values in place."""
    from beta_recsys_amd.sgl import symmetric_structure

    g = load_golden("sgl_refresh_walk_adam")
    m = sgl_meta(g)
    N = m["U"] + m["I"]
    eu, ei = g["inter_user"], g["inter_item"]
    rowptr, col, inter = (t.numpy() for t in symmetric_structure(eu, ei, m["U"], m["I"]))
    row = np.repeat(np.arange(N), np.diff(rowptr))
    assert col.size == 2 * eu.size and np.all(np.diff(row * N + col) > 0)
    lo, hi = np.minimum(row, col), np.maximum(row, col)
    assert np.array_equal(lo, eu[inter]) and np.array_equal(hi, m["U"] + ei[inter])
    eng = make_engine(g)
    for r in range(n_refreshes(g)):
        sub = eng.from_reference_dict(reference_dict(g, r))
        want = recorded_subs(g, r)
        srow = np.repeat(np.arange(N), np.diff(sub.rowptr.numpy()))
        for v in range(2):
            for l in range(m["L"]):
                A = np.zeros((N, N), dtype=np.float32)
                A[srow, sub.col.numpy()] = sub.vals[v][l].numpy()[: sub.nnz]
                assert np.array_equal(A, want[v][l])
    d = reference_dict(g, 0)
    d["adj_shape_sub11"] = (N + 1, N + 1)
    with pytest.raises(ValueError, match="expected"):
        eng.from_reference_dict(d)


def test_plan_struct_matches_the_library():
    from beta_recsys_amd import _lib

    lib = _lib.load()
    assert lib.hiprec_sgl_plan_bytes() == ctypes.sizeof(_lib.SglPlan)
    assert (_lib.SGL_TILE_B, _lib.SGL_TILE_N, _lib.SGL_MAX_LAYERS) == (32, 64, 6)
    p = _lib.SglPlan()
    assert lib.hiprec_sgl_propagate(ctypes.byref(p), None) == -1 and lib.hiprec_last_error()   # validated before any HIP call
    assert lib.hiprec_sgl_grad(None, None, None, None, 0, None, None, None, 0, None) == -1
    assert lib.hiprec_sgl_sub_values(None, None, None, None, None, 0, None, None, None) == -1
    assert lib.hiprec_sgl_ws_floats(10, 8) == 8 * 10 * 8 + 2 * 10


DEFECT_CASE = {"no_onehot": "sgl_both_edge_adam", "views_swapped": "sgl_both_edge_adam", "deduplicated": "sgl_hot_sgd",
               "bpr_mean": "sgl_both_edge_adam", "hop0_unscaled": "sgl_both_edge_adam"}


@pytest.mark.parametrize("defect", sx.DEFECTS)
def test_defects_are_visible(defect):
    """Each named defect moves a loss part or a gradient of the fp64 restatement by at least 10x what the GPU test's
    bound allows (REL of the quantity for a loss part, REL of the tensor's scale for a gradient)."""
    g = load_golden(DEFECT_CASE[defect])
    hp, graph = sgl_hp(g), sgl_graph(g)
    with float64_oracle(sx):
        subs = recorded_subs(g, 0, np.float64)
        w = to64(sgl_params(g, "w0"))
        parts, _, grads = sx.sgl_grads(w, graph, subs, hp, sgl_batch(g, 0))
        parts_d, _, grads_d = sx.sgl_grads(w, graph, subs, hp, sgl_batch(g, 0), defect=defect)
    margins = [abs(a - b) / (REL * abs(a)) for a, b in zip(parts, parts_d) if a != 0]
    margins += [float(np.abs(grads[k] - grads_d[k]).max() / (REL * np.abs(grads[k]).max())) for k in KEYS]
    print(f"{defect}: margins {['%.3g' % x for x in margins]}")
    assert max(margins) >= MIN_MARGIN, f"{defect}: the bounds cannot see it ({max(margins):.3g} x)"
    if defect == "no_onehot":       # the loss is untouched: only the gradients can show it
        assert parts == parts_d
