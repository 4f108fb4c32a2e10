"""GRU4Rec on the CPU: the fixtures of gru4rec_edges.py see every defect of the restatement and cover what their table
claims; the float32 restatement against the float64 one; the ``SessionParallelLoader`` contract against a brute-force
walk; the ABI of csrc/gru4rec.hip (parameter count, limits, workspace); config validation; the evidence group."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
import torch

import gru4rec_edges as ge
import gru4rec_torch as gt
from helpers import REL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement and its fixtures ------------------------------------------------------------------------------------
def _two_steps(f, defect=None):
    """The fixture's step and a second one on the same ids from the state the first left, with no slot reset (what a
    wrongly stored state shows in): ``(loss 1, grads 1, loss 2, grads 2)``."""
    cfg = ge.cfg_of(f)
    l1, g1, state = gt.grads(f["w"], cfg, ge.batch_of(f), f["state"], f["keeps"], torch.float64, defect)
    again = (f["in_items"], f["targets"], np.zeros_like(f["reset"]), f["samples"])
    l2, g2, _ = gt.grads(f["w"], cfg, again, state, f["keeps"], torch.float64, defect)
    return l1, g1, l2, g2


def _moved(f, defect):
    """The largest relative change of a loss or of a gradient tensor (relative to the tensor's scale)."""
    a, b = _two_steps(f), _two_steps(f, defect)
    out = max(abs(b[0] - a[0]) / abs(a[0]), abs(b[2] - a[2]) / abs(a[2]))
    for g0, g1 in ((a[1], b[1]), (a[3], b[3])):
        for k in g0:
            scale = np.abs(g0[k]).max()
            if scale > 0:
                out = max(out, float(np.abs(g1[k] - g0[k]).max() / scale))
    return out


@pytest.mark.parametrize("defect", gt.DEFECTS)
def test_some_fixture_sees_the_defect(defect):
    worst = {name: _moved(ge.fixture(name), defect) for name in ge.SCAN}
    assert max(worst.values()) > 10 * REL, f"{defect}: no fixture moves by more than {10 * REL:g}: {worst}"


def test_every_defect_is_listed():
    assert len(gt.DEFECTS) == len(set(gt.DEFECTS)) >= 14
    with pytest.raises(ValueError):      # N >= 2
        f = ge.fixture("tiny")
        gt.grads(f["w"], ge.cfg_of(f), (f["in_items"], f["targets"], f["reset"], f["samples"][:0]), f["state"])


@pytest.mark.parametrize("name", ge.NAMES)
def test_fixture_meets_the_margins_and_float32_agrees(name):
    f = ge.fixture(name)
    assert ge.MARGIN == 1e-3 and ge.margins_ok(f)
    lo, hi = ge.elu_margin(f)
    assert 0.3 < hi < 30, "the scores are O(1)"
    if f["loss"] == "bpr-max" and f["elu"] not in (0.0, 1.0):
        assert lo > ge.MARGIN * hi
    l64, g64, s64, l32, g32 = ge.reference(name)
    assert np.isfinite(l64) and abs(l32 - l64) <= REL * abs(l64), (l32, l64)
    assert list(g64) == list(f["w"]) == list(gt.shapes(f["I"], f["layers"], f["D"]))
    assert all(g64[k].shape == f["w"][k].shape and np.isfinite(g64[k]).all() for k in f["w"])
    assert all(np.abs(s).max() > 0 for s in f["state"]) and [s.shape for s in s64] == [(f["B"], H) for H in f["layers"]]
    # every table has rows that no id names (the GPU test asks such rows for an exactly zero gradient)
    for k, rows in ge.untouched_rows(f).items():
        assert rows.size >= 3 and not np.abs(g64[k][rows]).max()


def test_fixtures_cover_what_the_table_claims():
    fx = ge.fixture
    f = fx("tiny")
    assert (f["B"], f["S"], f["layers"], f["D"]) == (1, 1, [1], 0)
    f = fx("defaults")
    assert (f["B"], f["S"], f["layers"], f["D"], f["loss"]) == (7, 5, [100], 0, "bpr-max")
    assert 100 % 16 and 100 % 64 and f["elu"] == 0.5 and f["bpreg"] == 1.0 and f["logq"] == 1.0
    f = fx("limits")
    assert f["layers"] == [ge.LIMITS["hidden"]] * ge.LIMITS["layers"] and f["D"] == ge.LIMITS["embedding"]
    assert f["B"] == 2 and f["S"] == ge.CAND_TILE + 1
    f = fx("stacked")
    assert f["layers"] == [5, 9, 3] and f["D"] == 6
    for t in (ge.LOSS_WAVES, ge.ROW_TILE, ge.SLAB_ROWS):
        for B in (t - 1, t, t + 1):
            g = fx(f"tile_edges_B_{B}")
            assert g["B"] == B and g["layers"] == [3]
    assert sorted(fx(f"tile_edges_N_{S}")["B"] + S for S in ge.TILE_SAMPLES) == [5, ge.CAND_TILE - 1, ge.CAND_TILE,
                                                                                 ge.CAND_TILE + 1]
    f = fx("repeats")
    assert np.bincount(f["in_items"]).max() >= 5 and np.bincount(f["targets"]).max() >= 4
    assert np.bincount(f["samples"]).max() == 2 and set(f["samples"]) & set(f["targets"])
    assert len(set(f["in_items"]) & set(f["targets"])) > 0, "constrained: an input row is a candidate row too"
    assert fx("resets_all")["reset"].all() and not fx("resets_none")["reset"].any()
    assert 0 < fx("resets_mixed")["reset"].sum() < fx("resets_mixed")["B"]
    f = fx("dropout")
    assert f["pe"] == f["ph"] == 0.5 and len(f["keeps"]) == 1 + len(f["layers"]) == 3
    assert [k.shape for k in f["keeps"]] == [(9, 9), (9, 12), (9, 10)] and all(0.2 < k.mean() < 0.8 for k in f["keeps"])
    f = fx("logq")
    assert f["loss"] == "cross-entropy" and f["logq"] == 1.0 and f["alpha"] == 0.5 and len(set(np.round(f["p"], 12))) > 3
    assert {(fx(n)["elu"], fx(n)["bpreg"]) for n in ge.NAMES if n.startswith("elu_")} == {
        (a, b) for a in (0.0, 0.5, 1.0) for b in (0.0, 1.0)}
    f = fx("max_batch")
    assert (f["B"], f["S"]) == (ge.LIMITS["batch"], ge.LIMITS["n_sample"])


def test_the_tile_constants_are_those_of_the_sources():
    text = open(os.path.join(ROOT, "beta-recsys_amd", "csrc", "gru4rec.hpp")).read()
    got = {k: int(v) for k, v in re.findall(r"constexpr int (kGru4rec\w+) = (\d+);", text)}
    assert (got["kGru4recLossWaves"], got["kGru4recRowTile"], got["kGru4recSlabRows"], got["kGru4recCandTile"]) == (
        ge.LOSS_WAVES, ge.ROW_TILE, ge.SLAB_ROWS, ge.CAND_TILE)
    assert {"layers": got["kGru4recMaxLayers"], "hidden": got["kGru4recMaxHidden"], "embedding": got["kGru4recMaxDim"],
            "batch": got["kGru4recMaxBatch"], "n_sample": got["kGru4recMaxSample"]} == ge.LIMITS
    # the tiles are those of the grouped GEMM and of the block size
    ncf = open(os.path.join(ROOT, "beta-recsys_amd", "csrc", "ncf.hip")).read()
    tm, tn = re.search(r"constexpr int kTM = (\d+), kTN = (\d+)", ncf).groups()
    assert (int(tm), int(tn)) == (ge.ROW_TILE, ge.CAND_TILE)
    assert int(re.search(r"constexpr int kColsumRows = (\d+);", ncf).group(1)) == ge.SLAB_ROWS
    common = open(os.path.join(ROOT, "beta-recsys_amd", "csrc", "common.hpp")).read()
    block, wave = (int(re.search(rf"constexpr int {k} = (\d+);", common).group(1)) for k in ("kBlock", "kWave"))
    assert block // wave == ge.LOSS_WAVES


# ---- the loader ----------------------------------------------------------------------------------------------------------
def _sessions():
    rng = np.random.default_rng(5)
    lens = [5, 1, 3, 2, 7, 2, 0, 4, 6, 2, 3, 9, 2, 5, 3, 4]
    return [rng.integers(0, 12, n).tolist() for n in lens]


def _brute_force(sessions, B):
    """The session-parallel walk, event by event: ``[(step, slot, session, position, reset)]`` and the sessions used."""
    kept = [k for k, s in enumerate(sessions) if len(s) >= 2]
    slots = [[kept[b], 0, 1] for b in range(B)]
    nxt, out, step = B, [], 0
    while True:
        for b in range(B):
            if slots[b][1] + 1 >= len(sessions[slots[b][0]]):
                if nxt == len(kept):
                    return out
                slots[b] = [kept[nxt], 0, 1]
                nxt += 1
        for b in range(B):
            out.append((step, b, slots[b][0], slots[b][1], slots[b][2]))
            slots[b][1] += 1
            slots[b][2] = 0
        step += 1


def test_session_parallel_loader_contract():
    import beta_recsys_amd as hp

    sessions, B, S = _sessions(), 3, 4
    with pytest.warns(UserWarning, match="2 sessions"):
        loader = hp.data.SessionParallelLoader(sessions, 12, B, S, 0.5, seed=3)
    walk = _brute_force(sessions, B)
    n_steps = walk[-1][0] + 1
    assert len(loader) == n_steps > 4 and loader.in_items.shape == loader.targets.shape == loader.reset.shape == (n_steps, B)
    assert loader.reset.dtype == np.uint8 and loader.in_items.dtype == np.int64
    seen_pairs = {}
    for step, b, k, at, reset in walk:
        assert loader.in_items[step, b] == sessions[k][at] and loader.targets[step, b] == sessions[k][at + 1]
        assert loader.reset[step, b] == reset == (at == 0), "reset exactly at session starts"
        seen_pairs[(k, at)] = seen_pairs.get((k, at), 0) + 1
    assert set(seen_pairs.values()) == {1}
    # a session that was started before the epoch's end was walked to ITS end, unless it sat in a slot at the last step
    last = {k for step, b, k, at, reset in walk if step == n_steps - 1}
    for k in {k for _, _, k, _, _ in walk} - last:
        assert all((k, at) in seen_pairs for at in range(len(sessions[k]) - 1)), f"session {k} was cut short"
    assert loader.reset[0].all() and loader.reset.sum() == len({k for _, _, k, _, _ in walk})
    # support, event shares
    events = np.concatenate([s for s in sessions if len(s) >= 2])
    assert np.array_equal(loader.support, np.bincount(events, minlength=12))
    assert np.allclose(loader.item_probs, loader.support / loader.support.sum()) and abs(loader.item_probs.sum() - 1) < 1e-12
    # iteration: host tensors without a device; the same seed, the same samples; another epoch, other samples
    steps = list(loader)
    assert len(steps) == n_steps and all(len(s) == 4 for s in steps)
    assert all(t.dtype == d for t, d in zip(steps[0], (torch.int64, torch.int64, torch.uint8, torch.int64)))
    assert tuple(steps[1][3].shape) == (S,) and np.array_equal(steps[2][0].numpy(), loader.in_items[2])
    first = loader.samples.copy()
    again = hp.data.SessionParallelLoader([s for s in sessions if len(s) >= 2], 12, B, S, 0.5, seed=3)
    assert np.array_equal(np.stack([s[3].numpy() for s in again]), first)
    list(loader)
    assert loader.epoch == 2 and not np.array_equal(loader.samples, first), "the samples were not redrawn"
    assert np.array_equal(loader.samples, loader.draw_samples(1)) and np.array_equal(first, loader.draw_samples(0))
    other = hp.data.SessionParallelLoader([s for s in sessions if len(s) >= 2], 12, B, S, 0.5, seed=4)
    assert not np.array_equal(other.draw_samples(0), first)
    with pytest.raises(ValueError):
        hp.data.SessionParallelLoader([[1, 2], [3, 4]], 12, 3, S, 0.5)
    with pytest.raises(IndexError):
        hp.data.SessionParallelLoader([[1, 12], [3, 4], [5, 6]], 12, 3, S, 0.5)


def test_the_sample_histogram_follows_support_to_the_alpha():
    import beta_recsys_amd as hp

    rng = np.random.default_rng(8)
    I, alpha = 10, 0.5
    weights = np.arange(1, I + 1) ** 2.0
    sessions = [rng.choice(I - 1, size=6, p=weights[:-1] / weights[:-1].sum()).tolist() for _ in range(400)]   # item 9: no event
    with warnings.catch_warnings():
        warnings.simplefilter("error")      # nothing is dropped, nothing warns
        loader = hp.data.SessionParallelLoader(sessions, I, 8, 64, alpha, seed=1)
    draws = loader.draw_samples(0).reshape(-1)
    n = draws.size
    assert n > 10000
    want = loader.support.astype(np.float64) ** alpha
    want[loader.support == 0] = 0.0
    want /= want.sum()
    got = np.bincount(draws, minlength=I) / n
    assert got[I - 1] == 0.0, "an item without support was drawn"
    sigma = np.sqrt(want * (1 - want) / n)
    assert (np.abs(got - want) <= 4 * sigma).all(), (got, want)
    flat = loader.support / loader.support.sum()
    assert (np.abs(got - flat) > 4 * sigma).any(), "alpha was ignored"


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def _shape(n_items=40, layers=(100,), emb_dim=0, loss=0):
    from beta_recsys_amd import _lib

    layers = list(layers)
    return _lib.Gru4recShape(n_items, len(layers), (ctypes.c_int32 * 3)(*(layers + [0] * 3)[:3]), emb_dim, loss)


def test_abi_parameter_count_limits_and_workspace():
    from beta_recsys_amd import _lib

    lib = _lib.load()
    assert lib.hiprec_gru4rec_shape_bytes() == ctypes.sizeof(_lib.Gru4recShape) == 32
    for name in ("tiny", "defaults", "limits", "stacked", "dropout"):
        f = ge.fixture(name)
        s = _shape(f["I"], f["layers"], f["D"])
        assert lib.hiprec_gru4rec_param_floats(ctypes.byref(s)) == gt.n_params(f["I"], f["layers"], f["D"]) == sum(
            v.size for v in f["w"].values())
    ok = lambda s: lib.hiprec_gru4rec_param_floats(ctypes.byref(s))      # noqa: E731
    assert ok(_shape(layers=(128, 128, 128), emb_dim=128)) > 0
    for bad, word in ((_shape(layers=(129,)), "layers[0]"), (_shape(layers=(5, 0)), "layers[1]"), (_shape(emb_dim=129), "embedding"),
                      (_shape(emb_dim=-1), "embedding"), (_shape(loss=2), "loss"), (_shape(n_items=0), "n_items")):
        assert ok(bad) == -1
        assert word in lib.hiprec_last_error().decode(), lib.hiprec_last_error().decode()
        assert lib.hiprec_gru4rec_workspace_bytes(ctypes.byref(bad), 8, 8) == 0
    four = _shape()
    four.n_layers = 4
    assert ok(four) == -1 and "len(layers)" in lib.hiprec_last_error().decode()
    # the workspace: limits, 0 beyond them, independent of n_items
    ws = lambda s, B, S: lib.hiprec_gru4rec_workspace_bytes(ctypes.byref(s), B, S)      # noqa: E731
    base = ws(_shape(), 512, 2048)
    assert base > 0 and ws(_shape(n_items=10 ** 8), 512, 2048) == base
    assert ws(_shape(), 1024, 2048) > base and ws(_shape(), 512, 4096) > base
    assert ws(_shape(), ge.LIMITS["batch"], ge.LIMITS["n_sample"]) > 0 and ws(_shape(), 1, 0) > 0
    for B, S in ((0, 4), (ge.LIMITS["batch"] + 1, 4), (8, -1), (8, ge.LIMITS["n_sample"] + 1)):
        assert ws(_shape(), B, S) == 0


def _config(n_items=40, **kw):
    model = {"layers": [100], "loss": "bpr-max", "bpreg": 1.0, "elu_param": 0.5, "logq": 0.0, "n_sample": 2048,
             "sample_alpha": 0.5, "dropout_p_embed": 0.0, "dropout_p_hidden": 0.0, "batch_size": 64, "lr": 1e-3,
             "optimizer": "adam", "device_str": "cpu"}
    model.update(kw)
    return {"model": model, "dataset": {"n_items": n_items}, "system": {"run_dir": "/tmp/hiprec_test_runs"}}


def test_config_validation_and_initialisation():
    import beta_recsys_amd as hp

    torch.manual_seed(11)
    m = hp.GRU4Rec(_config(layers=[20, 30], constrained_embedding=False, embedding=50))
    sd = m.state_dict()
    want = gt.shapes(40, [20, 30], 50)
    assert list(sd) == list(want) and {k: tuple(v.shape) for k, v in sd.items()} == want
    assert m.flat.numel() == gt.n_params(40, [20, 30], 50)
    for k, v in sd.items():
        if "bias" in k or k == "By.weight":
            assert float(v.abs().max()) == 0.0, k
    # Glorot-uniform: inside the bound and close to it, per gate block
    for k, fan in (("Wy.weight", 40 + 30), ("E.weight", 40 + 50), ("G.0.weight_ih", 20 + 50), ("G.0.weight_hh", 20 + 20),
                   ("G.1.weight_ih", 30 + 20), ("G.1.weight_hh", 30 + 30)):
        bound = np.sqrt(6.0 / fan)
        blocks = sd[k].chunk(3, 0) if k.startswith("G.") else [sd[k]]
        for blk in blocks:
            assert 0.9 * bound < float(blk.abs().max()) <= bound, k
    torch.manual_seed(11)
    assert torch.equal(hp.GRU4Rec(_config(layers=[20, 30], constrained_embedding=False, embedding=50)).flat, m.flat)
    c = hp.GRU4Rec(_config())
    assert list(c.state_dict()) == list(gt.shapes(40, [100], 0)) and c.constrained and c.in_width == 100
    W, b = c.item_factors()
    assert tuple(W.shape) == (40, 100) and tuple(b.shape) == (40,)
    for kw in (dict(layers=[]), dict(layers=[1, 2, 3, 4]), dict(layers=[129]), dict(layers=[0]), dict(loss="top1"),
               dict(constrained_embedding=False, embedding=0), dict(constrained_embedding=False, embedding=129),
               dict(n_sample=-1), dict(n_sample=4097), dict(batch_size=0), dict(batch_size=2049), dict(dropout_p_embed=1.0),
               dict(dropout_p_hidden=-0.1), dict(bpreg=-1.0), dict(elu_param=-0.5)):
        with pytest.raises(ValueError):
            hp.GRU4Rec(_config(**kw))
    with pytest.raises(ValueError):
        hp.GRU4Rec(_config(n_items=0))
    with pytest.raises(RuntimeError):
        c.step([1, 2])      # no CPU path
    eng = hp.GRU4RecEngine(_config(loss="cross-entropy", logq=1.0))
    with pytest.raises(ValueError):
        eng.set_item_probs(np.ones(39) / 39)
    assert eng._mask_shapes(8) == [(8, 100), (8, 100)]


def test_evidence_group():
    import __graft_entry__ as entry

    group = entry.EVIDENCE_GROUPS["gru4rec"]
    assert sorted(group) == sorted(entry._EVIDENCE_COMMON + ["gru4rec.hip", "gru4rec.hpp", "ncf.hip", "gemm.hpp"])
    assert all(os.path.exists(os.path.join(entry.CSRC, n)) for n in group)
    assert entry.evidence_group("gru4rec_step") == "gru4rec" and entry.evidence_group("gru4rec") == "gru4rec"
    src = open(os.path.join(entry.CSRC, "gru4rec.hip")).read()
    assert "narm" not in src.lower(), "gru4rec.hip stands apart from narm.hip"
    for inc in re.findall(r'#include "(\w+\.hpp)"', src):
        assert inc in group, f"gru4rec.hip includes {inc}, which the evidence group leaves out"
