"""SR-GNN on the CPU: the fixtures of srgnn_edges.py see every defect of the restatement and cover what their table
claims; the float32 restatement against the float64 one; the session graph's worked examples; the edge lists against the
dense matrices; the limits against csrc/srgnn.hpp; the ABI; config validation; the evidence group; ``SessionLoader``'s
``shuffle``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import srgnn_edges as se
import srgnn_torch as st
from helpers import REL, assert_as_accurate_as_reference, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement and its fixtures ------------------------------------------------------------------------------------
def _moved(f, defect):
    """The largest relative change of the loss or of a gradient tensor (relative to the tensor's scale)."""
    l0, g0, _, _ = se.reference(f["name"])[:4]
    l1, g1, _, _ = st.grads(f["w"], se.cfg_of(f), se.batch_of(f), torch.float64, defect)
    out = abs(l1 - l0) / abs(l0)
    for k in g0:
        scale = np.abs(g0[k]).max()
        if scale > 0:
            out = max(out, float(np.abs(g1[k] - g0[k]).max() / scale))
        elif np.abs(g1[k]).max() > 0:
            out = np.inf      # a gradient where there must be none
    return out


@pytest.mark.parametrize("defect", [d for d in st.DEFECTS if d not in st.GRAPH_DEFECTS])
def test_some_fixture_sees_the_defect(defect):
    worst = {name: _moved(se.fixture(name), defect) for name in se.SCAN}
    print(defect, worst)
    assert max(worst.values()) > 10 * REL, f"{defect}: no fixture moves by more than {10 * REL:g}: {worst}"


@pytest.mark.parametrize("defect", st.GRAPH_DEFECTS)
def test_the_builder_comparison_sees_the_graph_defect(defect):
    """Numbering the nodes differently moves no loss and no gradient; it shows where the builder's arrays are compared."""
    f = se.fixture("revisits")
    assert _moved(f, defect) < 1e-12
    want = se.numpy_graph(f)
    moved = False
    for b, sess in enumerate(f["sessions"]):
        nodes, alias, _ = st.session_graph(sess, defect)
        lo = want["node_off"][b]
        moved |= nodes != want["nodes"][lo:lo + len(nodes)].tolist()
        moved |= alias != (want["alias"][:len(sess), b] - lo).tolist()
    assert moved


def test_every_defect_is_listed():
    assert len(st.DEFECTS) == len(set(st.DEFECTS)) >= 19 and set(st.GRAPH_DEFECTS) < set(st.DEFECTS)


@pytest.mark.parametrize("name", se.NAMES)
def test_float32_restatement_stays_inside_the_bound(name):
    f = se.fixture(name)
    l64, g64, q64, s64, l32, g32 = se.reference(name)
    assert np.isfinite(l64) and abs(l32 - l64) <= REL * abs(l64), (l32, l64)
    assert list(g64) == list(f["w"]) == list(st.shapes(f["n_node"], f["H"]))
    assert all(g64[k].shape == f["w"][k].shape and np.isfinite(g64[k]).all() for k in f["w"])
    for k in g64:      # the bound of the GPU test with the float32 restatement in the product's place
        assert_as_accurate_as_reference(g32[k], g64[k], g64[k], what=f"{name} {k}")
    assert 0.3 < np.abs(s64).max() < 100, "the scores are O(1)"
    assert q64.shape == (f["B"], f["H"]) and s64.shape == (f["B"], f["n_node"] - 1)
    # row 0 is read by nothing; the rows no session names still receive the softmax's term
    assert not np.abs(g64["embedding.weight"][0]).max()
    named = np.union1d(f["seq"][f["seq"] > 0], f["target"])
    if name != "tile_edges_I_1000":
        assert named.max() <= f["n_node"] - 4
    assert np.abs(g64["embedding.weight"][-3:]).min() > 0 or f["H"] == 1
    if f["nonhybrid"]:
        assert not np.abs(g64["linear_transform.weight"]).max() and not np.abs(g64["linear_transform.bias"]).max()


def test_fixtures_cover_what_the_table_claims():
    fx = se.fixture
    f = fx("tiny")
    assert (f["B"], f["T"], f["H"]) == (1, 1, 1) and se.numpy_graph(f)["indeg"].tolist() == [0]
    f = fx("defaults")
    assert (f["B"], f["T"], f["H"], f["step"], f["nonhybrid"]) == (7, 9, 100, 1, False) and len(set(f["lens"])) > 2
    f = fx("limits")
    assert (f["H"], f["step"], f["B"], f["T"]) == (se.LIMITS["hidden"], se.LIMITS["step"], 2, se.LIMITS["len"])
    g = se.numpy_graph(f)
    assert g["n_nodes"].tolist() == [256, 1] and g["indeg"][256] == g["outdeg"][256] == 1 and g["in_idx"][256] == 256
    f = fx("revisits")
    assert [4, 6, 4, 6] in f["sessions"] and [3, 3, 8] in f["sessions"] and [5, 3, 5, 5, 9] in f["sessions"]
    f = fx("shared_items")
    assert all(2 in s for s in f["sessions"]) and (f["target"] == 2).sum() >= 8
    f = fx("len_one_mixed")
    assert (f["lens"] == 1).sum() == 3 and f["lens"].max() == 9
    assert (fx("step_2")["step"], fx("step_3")["step"], fx("nonhybrid")["nonhybrid"]) == (2, 3, True)
    for t in (se.WAVES, se.ROW_TILE, se.SLAB_ROWS):
        for B in (t - 1, t, t + 1):
            assert fx(f"tile_edges_B_{B}")["B"] == B
    for n in se.TILE_NODES:
        f = fx(f"tile_edges_N_{n}")
        assert se.numpy_graph(f)["node_off"][-1] == n == f["lens"].sum() - 1
    for n in se.TILE_ITEMS:
        assert fx(f"tile_edges_I_{n}")["n_node"] - 1 == n
    f = fx("tile_edges_I_1000")
    assert f["target"][0] == 1 and f["target"][1] == 1000
    f = fx("max_batch")
    assert f["B"] == se.LIMITS["batch"] and f["T"] <= 4
    for name in se.NAMES:
        f = fx(name)
        assert f["lens"].max() == f["T"] == f["seq"].shape[0] and f["lens"].min() >= 1
        assert (f["seq"][np.arange(f["T"])[:, None] < f["lens"][None, :]] > 0).all()


# ---- the session graph ---------------------------------------------------------------------------------------------------
def test_the_worked_examples_hold():
    nodes, alias, in_l, out_l = st.edge_lists([5, 3, 5, 5, 9])
    assert nodes == [3, 5, 9] and alias == [1, 0, 1, 1, 2]
    edges = {(u, v) for v, lst in enumerate(in_l) for u in lst}
    assert edges == {(1, 0), (0, 1), (1, 1), (1, 2)} == {(u, v) for u, lst in enumerate(out_l) for v in lst}
    assert [len(x) for x in in_l] == [1, 2, 1] and [len(x) for x in out_l] == [1, 3, 0]
    _, _, A = st.session_graph([5, 3, 5, 5, 9])
    assert A.sum(0).tolist() == [1, 2, 1] and A.sum(1).tolist() == [1, 3, 0]
    _, _, in_l, out_l = st.edge_lists([5, 3, 5, 3])
    assert {(u, v) for v, lst in enumerate(in_l) for u in lst} == {(1, 0), (0, 1)}
    _, _, A = st.session_graph([5, 3, 5, 3])
    assert A.tolist() == [[0, 1], [1, 0]]


@pytest.mark.parametrize("name", se.SCAN + se.BUILDER)
def test_the_edge_lists_equal_the_dense_matrices(name):
    f = se.fixture(name)
    items, alias, A_in, A_out, indeg, outdeg, mask = st.dense_batch(f["seq"], f["lens"])
    g = se.numpy_graph(f)
    assert g["node_off"][-1] == (items > 0).sum() and g["slot_off"][-1] == f["lens"].sum()
    for b in range(f["B"]):
        lo, k = g["node_off"][b], g["n_nodes"][b]
        assert g["nodes"][lo:lo + k].tolist() == items[b, :k].tolist() and (g["node_sess"][lo:lo + k] == b).all()
        assert g["node_cnt"][lo:lo + k].tolist() == [int((alias[b, :f["lens"][b]] == v).sum()) for v in range(k)]
        assert (g["alias"][:f["lens"][b], b] - lo).tolist() == alias[b, :f["lens"][b]].tolist()
        assert (g["alias"][f["lens"][b]:, b] == -1).all()
        dense_in, dense_out = np.zeros((k, k)), np.zeros((k, k))
        for v in range(k):
            row = lo + v
            assert g["indeg"][row] == indeg[b, v] and g["outdeg"][row] == outdeg[b, v]
            ins = g["in_idx"][g["in_start"][row]:g["in_start"][row] + g["indeg"][row]] - lo
            outs = g["out_idx"][g["out_start"][row]:g["out_start"][row] + g["outdeg"][row]] - lo
            assert list(ins) == sorted(ins) and list(outs) == sorted(outs)
            dense_in[v, ins] = 1.0 / max(len(ins), 1)
            dense_out[v, outs] = 1.0 / max(len(outs), 1)
        assert np.array_equal(dense_in, A_in[b, :k, :k]) and np.array_equal(dense_out, A_out[b, :k, :k])
    assert (g["node_sess"][g["node_off"][-1]:] == -1).all()


def test_the_limits_and_tile_constants_are_those_of_the_sources():
    from beta_recsys_amd import srgnn

    text = open(os.path.join(ROOT, "beta-recsys_amd", "csrc", "srgnn.hpp")).read()
    got = {k: int(v) for k, v in re.findall(r"constexpr int (kSrgnn\w+) = (\d+);", text)}
    assert (got["kSrgnnWaves"], got["kSrgnnRowTile"], got["kSrgnnSlabRows"], got["kSrgnnKSlices"]) == (
        se.WAVES, se.ROW_TILE, se.SLAB_ROWS, se.K_SLICES)
    assert {"hidden": got["kSrgnnMaxHidden"], "step": got["kSrgnnMaxStep"], "len": got["kSrgnnMaxLen"],
            "batch": got["kSrgnnMaxBatch"]} == se.LIMITS
    assert (srgnn.MAX_HIDDEN, srgnn.MAX_STEP, srgnn.MAX_LEN, srgnn.MAX_BATCH) == tuple(se.LIMITS.values())
    assert se.LIMITS["batch"] >= 1024
    ncf = open(os.path.join(ROOT, "beta-recsys_amd", "csrc", "ncf.hip")).read()
    assert int(re.search(r"constexpr int kTM = (\d+)", ncf).group(1)) == se.ROW_TILE
    assert int(re.search(r"constexpr int kColsumRows = (\d+);", ncf).group(1)) == se.SLAB_ROWS
    gemm = open(os.path.join(ROOT, "beta-recsys_amd", "csrc", "gemm.hpp")).read()
    assert int(re.search(r"constexpr int kMaxGroup = (\d+);", gemm).group(1)) >= se.K_SLICES
    common = open(os.path.join(ROOT, "beta-recsys_amd", "csrc", "common.hpp")).read()
    block, wave = (int(re.search(rf"constexpr int {k} = (\d+);", common).group(1)) for k in ("kBlock", "kWave"))
    assert block // wave == se.WAVES and block >= se.LIMITS["len"]


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def _shape(n_node=40, hidden=100, step=1, nonhybrid=0):
    from beta_recsys_amd import _lib

    return _lib.SrgnnShape(n_node, hidden, step, nonhybrid, 0)


def test_abi_parameter_count_limits_and_workspace():
    from beta_recsys_amd import _lib

    lib = _lib.load()
    assert lib.hiprec_srgnn_shape_bytes() == ctypes.sizeof(_lib.SrgnnShape) == 24
    for name in ("tiny", "defaults", "limits", "nonhybrid"):
        f = se.fixture(name)
        s = _shape(f["n_node"], f["H"], f["step"], int(f["nonhybrid"]))
        assert lib.hiprec_srgnn_param_floats(ctypes.byref(s)) == st.n_params(f["n_node"], f["H"]) == sum(
            v.size for v in f["w"].values())
    ok = lambda s: lib.hiprec_srgnn_param_floats(ctypes.byref(s))      # noqa: E731
    assert ok(_shape(hidden=128, step=4)) > 0
    for bad, word in ((_shape(hidden=129), "hidden_size"), (_shape(hidden=0), "hidden_size"), (_shape(step=5), "step"),
                      (_shape(step=0), "step"), (_shape(n_node=1), "n_node")):
        assert ok(bad) == -1
        assert word in lib.hiprec_last_error().decode(), lib.hiprec_last_error().decode()
        assert lib.hiprec_srgnn_workspace_bytes(ctypes.byref(bad), 8, 8, 0) == 0
    ws = lambda B, T, R=0: lib.hiprec_srgnn_workspace_bytes(ctypes.byref(_shape()), B, T, R)      # noqa: E731
    base = ws(100, 69)
    assert base > 0 and ws(100, 69, 500) < base and ws(100, 69, 100 * 69) == base and ws(200, 69) > base
    assert ws(se.LIMITS["batch"], se.LIMITS["len"]) > 0 and ws(1, 1) > 0
    for B, T, R in ((0, 4, 0), (se.LIMITS["batch"] + 1, 4, 0), (8, 0, 0), (8, se.LIMITS["len"] + 1, 0), (8, 4, 33), (8, 4, -1)):
        assert ws(B, T, R) == 0
    assert lib.hiprec_srgnn_graph_ints(3, 5, 9) == 3 + 4 + 4 + 15 + 9 * 9
    assert lib.hiprec_srgnn_graph_ints(se.LIMITS["batch"] + 1, 5, 9) == 0


def _config(n_node=40, **kw):
    model = {"optimizer": "adam", "lr": 1e-3, "device_str": "cpu"}
    model.update(kw)
    return {"model": model, "dataset": {"n_node": n_node}, "system": {"run_dir": "/tmp/hiprec_test_runs"}}


def test_config_validation_and_initialisation():
    import beta_recsys_amd as hp

    torch.manual_seed(11)
    m = hp.SRGNN(_config(hidden_size=20, step=2))
    sd = m.state_dict()
    want = st.shapes(40, 20)
    assert list(sd) == list(want) and {k: tuple(v.shape) for k, v in sd.items()} == want
    assert m.flat.numel() == st.n_params(40, 20)
    # one uniform_ call per parameter in state_dict() order on the default generator, bound 1 / sqrt(H)
    torch.manual_seed(11)
    stdv = 1.0 / np.sqrt(20)
    for k, shape in want.items():
        assert torch.equal(sd[k], torch.empty(shape).uniform_(-stdv, stdv)), k
    d = hp.SRGNN(_config())      # the paper's defaults
    assert (d.hidden_size, d.step, d.nonhybrid, d.batch_size, d.l2) == (100, 1, False, 100, 1e-5)
    assert "linear_edge_f" not in " ".join(d.state_dict())
    n = hp.SRGNN(_config(nonhybrid=True, hidden_size=8))
    assert "linear_transform.weight" in n.state_dict() and n.shape.nonhybrid == 1
    for kw in (dict(hidden_size=0), dict(hidden_size=129), dict(step=0), dict(step=5), dict(batch_size=0),
               dict(batch_size=1025), dict(l2=-1.0)):
        with pytest.raises(ValueError):
            hp.SRGNN(_config(**kw))
    with pytest.raises(ValueError):
        hp.SRGNN(_config(n_node=1))
    with pytest.raises(RuntimeError):
        d.query(np.array([[1], [2]]), [2])      # no CPU path
    eng = hp.SRGNNEngine(_config(lr=0.01))
    assert [eng.epoch_lr(e) for e in range(7)] == [0.01 * 0.1 ** (e // 3) for e in range(7)]
    from beta_recsys_amd.srgnn import _checked_batch

    for seq, lens in (([[1, 2], [0, 3]], [2, 2]), ([[1, 2], [3, 0], [0, 0]], [3, 1])):      # a 0 inside a length
        with pytest.raises(ValueError):
            _checked_batch(np.array(seq), lens, "cpu")
    with pytest.raises(ValueError):
        _checked_batch(np.ones((257, 1), dtype=np.int64), [257], "cpu")
    with pytest.raises(ValueError):
        _checked_batch(np.ones((1, 1025), dtype=np.int64), [1] * 1025, "cpu")
    assert _checked_batch(np.array([[1, 2], [3, 0]]), [2, 1], "cpu")[2:] == (2, 2, 3)


def test_evidence_group():
    import __graft_entry__ as entry

    group = entry.EVIDENCE_GROUPS["srgnn"]
    assert sorted(group) == sorted(entry._EVIDENCE_COMMON + ["srgnn.hip", "srgnn.hpp", "ncf.hip", "gemm.hpp"])
    assert all(os.path.exists(os.path.join(entry.CSRC, n)) for n in group)
    assert entry.evidence_group("srgnn_step") == "srgnn" and entry.evidence_group("srgnn") == "srgnn"
    src = open(os.path.join(entry.CSRC, "srgnn.hip")).read()
    for inc in re.findall(r'#include "(\w+\.hpp)"', src):
        assert inc in group, f"srgnn.hip includes {inc}, which the evidence group leaves out"


# ---- the loader ----------------------------------------------------------------------------------------------------------
def _ragged(flat, lens):
    return [a.tolist() for a in np.split(flat, np.cumsum(lens)[:-1])]


def test_session_loader_defaults_are_unchanged():
    from beta_recsys_amd.data import SessionLoader, session_prefixes

    g = load_golden("narm_loader")
    out_seqs, labels = session_prefixes(_ragged(g["seq_flat"], g["seq_lens"]))
    for loader in (SessionLoader(out_seqs, labels, int(g["batch_size"])),
                   SessionLoader(out_seqs, labels, int(g["batch_size"]), shuffle=False, seed=3)):
        assert loader.shuffle is False
        for _ in range(2):
            batches = list(loader)
            assert len(batches) == int(g["n_batches"])
            for k, (seq, target, lens) in enumerate(batches):
                assert np.array_equal(seq.numpy(), g[f"b{k}/seq"]) and np.array_equal(target.numpy(), g[f"b{k}/target"])
                assert lens == g[f"b{k}/lens"].tolist()


def test_shuffle_visits_every_session_once_per_epoch_and_differs_between_epochs():
    from beta_recsys_amd.data import SessionLoader

    rng = np.random.default_rng(4)
    n, batch = 53, 8
    out_seqs = [[1000 * k + j + 1 for j in range(int(rng.integers(1, 7)))] for k in range(n)]      # a session names itself
    labels = [k + 1 for k in range(n)]
    loader = SessionLoader(out_seqs, labels, batch, shuffle=True, seed=7)
    assert len(loader) == 7
    epochs = []
    for _ in range(3):
        order = []
        for seq, target, lens in loader:
            seq, target = seq.numpy(), target.numpy()
            assert seq.shape == (max(lens), len(lens)) and lens == sorted(lens, reverse=True) and len(lens) <= batch
            for b, (lab, ln) in enumerate(zip(target, lens)):
                assert seq[:ln, b].tolist() == out_seqs[lab - 1] and not seq[ln:, b].any()
                order.append(int(lab))
        assert sorted(order) == labels, "every session once per epoch"
        epochs.append(order)
    assert epochs[0] != epochs[1] != epochs[2] and epochs[0] != labels
    again = [int(x) for _, target, _ in SessionLoader(out_seqs, labels, batch, shuffle=True, seed=7) for x in target]
    assert again == epochs[0], "one seed, one run"
    other = [int(x) for _, target, _ in SessionLoader(out_seqs, labels, batch, shuffle=True, seed=8) for x in target]
    assert other != epochs[0]
