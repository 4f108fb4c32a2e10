"""Host-side tests of the LCFN mirror (no GPU): limits, the reference's RNG order, state_dict keys, the ctypes plan, the
"no CPU fallback" error, data.graph_embeddings, and the visibility of every named defect at the edge fixtures."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

import lcfn_edges as le
import lcfn_numpy as lx
from helpers import REL
from test_oracle_golden_lcfn import CASES, KEYS, lcfn_batch, lcfn_golden, lcfn_meta

MIN_MARGIN = 10.0


def model_config(g, **over):
    m = lcfn_meta(g)
    cfg = dict(n_users=m["U"], n_items=m["I"], emb_dim=m["D"], layer=m["L"], lamda=float(g["lamda"]),
               graph_embeddings=[g["P"], g["Q"]], optimizer=str(g["optimizer"]), lr=float(g["lr"]), device_str="cpu",
               batch_size=m["B"])
    cfg.update(over)
    return cfg


def engine_of(cfg):
    import beta_recsys_amd as hp

    with contextlib.redirect_stdout(io.StringIO()):
        return hp.LCFNEngine({"model": cfg, "system": {"run_dir": "/tmp/hiprec_test_runs"}})


def make_engine(g, **over):
    return engine_of(model_config(g, **over))


def edge_engine(case, optimizer="sgd", lr=0.05, **over):
    """An engine for an edge fixture (tests/lcfn_edges.py), its weights and tail loaded."""
    cfg = dict(n_users=case["U"], n_items=case["I"], emb_dim=case["D"], layer=case["L"], lamda=case["hp"]["lamda"],
               graph_embeddings=[case["P"], case["Q"]], optimizer=optimizer, lr=lr, device_str="cpu", batch_size=case["B"],
               train_filters=case["train_filters"])
    if "slots" in case:
        cfg["project_slots"] = case["slots"]
    cfg.update(over)
    eng = engine_of(cfg)
    load_weights(eng, case["w"])
    return eng


def load_weights(eng, w):
    eng.model.load_state_dict({k: torch.from_numpy(np.asarray(w[k], dtype=np.float32)) for k in KEYS})
    if any(k not in KEYS for k in w):
        eng.model.load_filter_state({k: v for k, v in w.items() if k not in KEYS})


def test_limits_raise_value_error():
    g = lcfn_golden("lcfn_adam")
    m = lcfn_meta(g)
    assert list(make_engine(g).model.state_dict()) == list(KEYS)
    wide = np.zeros((m["U"], 257), dtype=np.float32)
    for over, text in (({"emb_dim": 0}, "emb_dim"), ({"emb_dim": 129}, "emb_dim"), ({"layer": 0}, "layer"),
                       ({"layer": 5}, "layer"), ({"emb_dim": 128, "layer": 4}, "at most 512"),
                       ({"graph_embeddings": [wide, g["Q"]]}, "frequence_user"),
                       ({"graph_embeddings": [g["P"], np.zeros((m["I"], 0), dtype=np.float32)]}, "frequence_item"),
                       ({"graph_embeddings": [g["P"][:-1], g["Q"]]}, "expected"), ({"project_slots": -1}, "project_slots")):
        with pytest.raises(ValueError, match=text):
            make_engine(g, **over)
    for ok in ({"emb_dim": 128, "layer": 3}, {"emb_dim": 1, "layer": 4},
               {"graph_embeddings": [np.zeros((m["U"], 256), dtype=np.float32), g["Q"]]}):
        make_engine(g, **ok)


def test_training_on_the_cpu_raises():
    g = lcfn_golden("lcfn_adam")
    eng = make_engine(g)
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP path"):
        eng.train_single_batch(lcfn_batch(g, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback|no HIP path"):
        eng.model.predict([0], [0])


@pytest.mark.parametrize("case", CASES)
def test_same_seeds_give_the_references_initial_state(case):
    """The reference's order of draws (lcfn.py:24-48): torch for the tables and the filters, numpy for the transformers."""
    g = lcfn_golden(case)
    torch.manual_seed(int(g["torch_seed"]))
    np.random.seed(int(g["numpy_seed"]))
    model = make_engine(g).model
    sd = model.state_dict()
    assert list(sd) == list(KEYS)
    for k in KEYS:
        assert np.array_equal(sd[k].numpy(), g[f"w0/{k}"]), k
    for name in ("user_filters", "item_filters", "transformers"):
        lst = getattr(model, name)
        assert isinstance(lst, list) and len(lst) == 1 and not lst[0].requires_grad
        assert np.array_equal(lst[0].numpy(), g[f"w0/{name}.0"]), name
    assert (model.frequence_user, model.frequence_item) == (g["P"].shape[1], g["Q"].shape[1])
    assert model.layer == 1 and model.lamda == float(g["lamda"]) and tuple(model.P.shape) == g["P"].shape


@pytest.mark.parametrize("train_filters", [False, True])
def test_state_dict_keys_are_the_references_two(train_filters):
    g = lcfn_golden("lcfn_adam")
    eng = make_engine(g, train_filters=train_filters, layer=2)
    m = eng.model
    assert list(m.state_dict()) == list(KEYS)
    assert [n for n, _ in m.named_parameters()] == list(KEYS) and not list(m.named_buffers())
    # the tail follows the tables in the flat buffer and the lists are views of it
    assert m.flat.numel() == m.table_floats + 2 * (m.frequence_user + m.frequence_item + m.emb_dim ** 2)
    assert m.user_filters[0].data_ptr() == m.flat.data_ptr() + 4 * m.table_floats
    assert eng._sweep_floats() == (m.flat.numel() if train_filters else m.table_floats)
    state = m.filter_state()
    assert sorted(state) == sorted(lx.tail_keys(2))
    state["transformers.1"] = state["transformers.1"] + 1
    m.load_filter_state(state)
    assert torch.equal(m.transformers[1], state["transformers.1"]) and torch.equal(m.filter_state()["user_filters.0"],
                                                                                 state["user_filters.0"])
    eng._dp_world = 2
    with pytest.raises(NotImplementedError, match="data-parallel"):
        eng._enqueue_grad(lcfn_batch(g, 0))


def test_plan_struct_matches_the_library():
    from beta_recsys_amd import _lib

    lib = _lib.load()
    assert lib.hiprec_lcfn_plan_bytes() == ctypes.sizeof(_lib.LcfnPlan)
    assert (lib.hiprec_lcfn_tile_rows(), lib.hiprec_lcfn_max_slots()) == (_lib.LCFN_TILE_ROWS, _lib.LCFN_MAX_SLOTS)
    p = _lib.LcfnPlan()
    assert lib.hiprec_lcfn_propagate(ctypes.byref(p), None) == -1 and lib.hiprec_last_error()   # validated before any HIP call
    assert lib.hiprec_lcfn_grad(None, None, None, None, 0, None, None, None, 0, None) == -1
    assert lib.hiprec_lcfn_predict(None, None, None, 0, None, None, None) == -1
    p.n_users, p.n_items, p.f_user, p.f_item, p.dim, p.layer = 10, 10, 4, 4, 129, 1
    assert lib.hiprec_lcfn_propagate(ctypes.byref(p), None) == -1 and b"emb_dim" in lib.hiprec_last_error()
    p.dim, p.layer = 128, 4
    assert lib.hiprec_lcfn_propagate(ctypes.byref(p), None) == -1 and b"at most" in lib.hiprec_last_error()
    # a bounded slot count shrinks the workspace by exactly the slots it saves
    T = _lib.LCFN_TILE_ROWS
    full, two = lib.hiprec_lcfn_ws_floats(5 * T, 3 * T, 6, 4, 8, 1, 0), lib.hiprec_lcfn_ws_floats(5 * T, 3 * T, 6, 4, 8, 1, 2)
    assert full - two == (3 * 6 + 1 * 4) * 8
    assert lib.hiprec_lcfn_batch_ws_floats(7) == 28


def test_graph_embeddings_are_the_low_eigenvectors_of_the_references_laplacians():
    """Columns satisfy ||L v - lambda v|| <= 1e-4 for the Laplacian deprecated_data_base.py:420-452 builds (restated
    here with its loops, repeated pairs included), eigenvalues ascend, shapes are int(cut_off * n); signs are free."""
    import scipy.sparse as sp

    from beta_recsys_amd.data import graph_embeddings

    rng = np.random.default_rng(3)
    U, I, cut = 41, 33, 0.2
    users = np.concatenate([np.arange(U), rng.integers(0, U, 160)])
    items = np.concatenate([rng.integers(0, I, U - I + I), rng.integers(0, I, 160)])[: users.size]
    items[:I] = np.arange(I)
    users, items = np.append(users, users[:5]), np.append(items, items[:5])      # repeated pairs
    P, Q = graph_embeddings(users, items, U, I, cut)
    assert P.dtype == np.float32 and Q.dtype == np.float32
    assert P.shape == (U, int(cut * U)) and Q.shape == (I, int(cut * I))
    H_u, D_u, D_v = sp.lil_matrix((U, I)), np.zeros(U), np.zeros(I)
    for u, i in zip(users, items):                       # the reference's loop
        H_u[u, i] = 1
        D_u[u] += 1
        D_v[i] += 1
    H = H_u.toarray()
    for B, Hm, dn, de in ((P, H, D_u, D_v), (Q, H.T, D_v, D_u)):
        Dn, De = np.diag(1 / np.maximum(np.sqrt(dn), 1e-10)), np.diag(1 / np.maximum(de, 1e-10))
        L = np.eye(len(dn)) - Dn @ Hm @ De @ Hm.T @ Dn
        B = B.astype(np.float64)
        lam = np.einsum("ij,ij->j", B, L @ B) / np.einsum("ij,ij->j", B, B)
        assert np.all(np.diff(lam) >= -1e-6), "eigenvalues do not ascend"
        assert np.abs(L @ B - B * lam).max() <= 1e-4 and np.linalg.norm(L @ B - B * lam, axis=0).max() <= 1e-4
        assert np.allclose(lam, np.linalg.eigvalsh(L)[: B.shape[1]], atol=1e-4), "not the LOWEST frequencies"
    with pytest.raises(ValueError):
        graph_embeddings(users, items, U, I, 0.0)
    with pytest.raises(ValueError, match="outside"):
        graph_embeddings([U], [0], U, I, cut)


DEFECT_CASE = {"no_filter": "f16_17_d15", "w_transposed": "f16_17_d15", "no_sigmoid_derivative": "f16_17_d15",
               "no_hop_gradient": "f4_5_d8_above_tile", "squared_norms": "f16_17_d15", "reg_deduplicated": "repeated_triple",
               "dw_user_only": "train_f4_5_d8", "tile_tail_rows": "f16_17_d15", "freq_tail": "f16_17_d15",
               "dim_tail": "f16_17_d15"}


@pytest.mark.parametrize("defect", lx.DEFECTS)
def test_defects_are_visible(defect):
    """Each named defect moves a loss part or a gradient of the fp64 restatement at an edge fixture by at least 10x what
    the GPU test's bound allows (REL of the quantity for a loss part, REL of the tensor's scale for a gradient)."""
    case = le.make_case(DEFECT_CASE[defect])
    parts, _, grads = le.restated(case)
    parts_d, _, grads_d = le.restated(case, defect)
    margins = [abs(a - b) / (REL * abs(a)) for a, b in zip(parts, parts_d) if a != 0]
    margins += [float(np.abs(grads[k] - grads_d[k]).max() / (REL * np.abs(grads[k]).max())) for k in grads]
    print(f"{defect}: margins {['%.3g' % x for x in margins]}")
    assert max(margins) >= MIN_MARGIN, f"{defect}: the bounds cannot see it ({max(margins):.3g} x)"


def test_every_edge_case_sits_on_a_seam():
    s = le.seams()
    cs = le.cases()
    T, K = s["tile"], s["triples"]
    assert {c["Fu"] for c in cs.values()} | {c["Fi"] for c in cs.values()} >= {1, 3, 4, 5, 16, 17, 33, s["max_freq"]}
    assert {c["D"] for c in cs.values()} >= {1, 8, 15, 16, 33, 64, s["max_dim"]}
    assert all(c["Fu"] != c["Fi"] for c in cs.values())
    ns = {c["U"] for c in cs.values()} | {c["I"] for c in cs.values()}
    assert {T - 1, T, T + 1} <= ns and max(ns) <= 4096
    assert {c["L"] for c in cs.values()} == set(range(1, s["max_layers"] + 1))
    assert any((c["L"] + 1) * c["D"] == s["max_width"] for c in cs.values())
    assert any(c["B"] == 1 for c in cs.values()) and any(c["B"] % K for c in cs.values())
    r = cs["slot_rounds"]
    assert -(-r["U"] // T) > r["slots"] and -(-r["I"] // T) > r["slots"] and r["slots"] < s["max_slots"]
    assert sum(1 for c in cs.values() if c.get("train_filters")) == 2
