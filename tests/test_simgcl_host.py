"""CPU tests of what the SimGCL GPU tests rest on: every named defect of the restatement (tests/simgcl_numpy.py) is visible
to the bounds the GPU tests apply, the fixtures and edge cases keep the share of zeroed uniforms under the cap, and the
restated device draw is what it claims to be."""
import numpy as np
import pytest

import simgcl_edges as edges
import simgcl_numpy as sx
from helpers import REL, float64_oracle, load_golden, to64
from test_oracle_golden_simgcl import CASES, KEYS, sim_batch, sim_graph, sim_hp, sim_meta, sim_params

_CACHE, _REF = {}, {}


def inputs():
    """``{name: (w, graph, hp, batch, noise)}`` of every fixture's first step and every edge case, with the fp64
    restatement's result; computed once."""
    if not _CACHE:
        for case in CASES:
            g = load_golden(case)
            _CACHE[case] = (sim_params(g, "w0"), sim_graph(g), sim_hp(g), sim_batch(g, 0), g["noise"][0])
        for name in edges.CASES:
            c = edges.build(name)
            _CACHE[name] = (c["w"], c["graph"], c["hp"], c["batch"], c["noise"])
    return _CACHE


def fp64(args, defect=None, **hp_over):
    w, graph, hp, batch, noise = args
    with float64_oracle(sx):
        return sx.simgcl_grads(to64(w), graph, dict(hp, **hp_over), batch, noise, defect)


def moved(ref, got):
    """By how many times the GPU tests' bound a loss part or a gradient moved.  Parts and the loss are held to REL of
    themselves, the InfoNCE parts to REL of at least the number of unique rows; here EVERY part gets the floor of the
    largest number of unique rows any case has, which only makes a defect harder to see.  Gradients: REL of scale."""
    worst = 0.0
    for a, b in zip(ref[0] + (ref[1],), got[0] + (got[1],)):
        if not np.isfinite(b):
            return np.inf
        worst = max(worst, abs(a - b) / (REL * max(abs(a), 2.0 * edges.TN + 3)))
    for k in KEYS:
        if not np.isfinite(got[2][k]).all():
            return np.inf
        worst = max(worst, float(np.abs(ref[2][k] - got[2][k]).max() / (REL * np.abs(ref[2][k]).max())))
    return worst


@pytest.mark.parametrize("defect", sx.DEFECTS)
def test_every_named_defect_is_visible(defect):
    """Some fixture or edge case moves a loss part or a gradient by at least 10 x the GPU tests' bound."""
    best, where = 0.0, None
    for name, args in inputs().items():
        if name not in _REF:
            _REF[name] = fp64(args)
        ref = _REF[name]
        m = moved(ref, fp64(args, defect))
        if m > best:
            best, where = m, name
    print(f"{defect}: {best:.3g} x the bound at {where}")
    assert best >= 10, f"{defect} moves nothing by more than {best:.3g} x the bound"


def test_user_view_switch_is_the_named_defect():
    """``user_view = "two_views"`` is the restatement with ``user_view2`` switched on, and differs from the default."""
    args = inputs()["simgcl_adam"]
    a, b = fp64(args, user_view="two_views"), fp64(args, "user_view2")
    assert a[1] == b[1] and all(np.array_equal(a[2][k], b[2][k]) for k in KEYS)
    assert moved(fp64(args), a) >= 10


@pytest.mark.parametrize("case", CASES)
def test_fixtures_keep_the_zeroed_share_under_the_cap(case):
    """Replayed hop by hop from the recorded weights: every fragile element of the fixture carries a zero uniform, and
    they are fewer than 1 % (random data stays near 0.01 %)."""
    g = load_golden(case)
    m, hp = sim_meta(g), sim_hp(g)
    A = sx.dense_adj(sim_graph(g))
    assert float(g["zeroed_share"]) <= sx.ZEROED_CAP
    for s in range(m["n_steps"]):
        w = sim_params(g, f"w{s}")
        E0 = np.concatenate([w[KEYS[0]], w[KEYS[1]]])
        for v in range(2):
            settled, _ = sx.settle_noise(E0, A, m["L"], hp["eps"], g["noise"][s][v])
            assert np.array_equal(settled, g["noise"][s][v]), f"{case} step {s} view {v}: a fragile element kept its noise"
            assert (g["noise"][s][v] == 0).mean() <= sx.ZEROED_CAP


@pytest.mark.parametrize("name", list(edges.CASES))
def test_edge_cases_are_what_they_claim(name):
    c = edges.build(name)
    D, L, eps, nu, ni, extra = edges.CASES[name]
    users, pos, neg = c["batch"]
    assert (np.unique(users).size, np.unique(pos).size) == (nu, ni) == c["n_uniq"]
    assert c["zeroed"] <= sx.ZEROED_CAP
    assert abs(c["min_x"] - extra.get("min_x", -4.0)) < 1e-3
    A = sx.dense_adj(c["graph"])
    iso = np.flatnonzero(np.abs(A).sum(axis=1) == 0)
    assert iso.size == 2 * c["n_iso"]
    parts, loss, grads = fp64((c["w"], c["graph"], c["hp"], c["batch"], c["noise"]))
    assert np.isfinite(loss) and all(np.isfinite(grads[k]).all() for k in KEYS), "no NaN anywhere"
    if nu == 1:
        assert abs(parts[2]) < 1e-12, "one unique row: the InfoNCE part is exactly 0"
    if extra.get("zero_neg"):
        assert set(neg) == {c["I"] - 1} and not np.abs(A[c["U"] + c["I"] - 1]).any()
    elif c["n_iso"]:
        named = set(users) | set(c["U"] + pos) | set(c["U"] + neg)
        assert not named & set(iso), "no batch names an isolated node"
    if eps == 0:
        a = sx.pooled(np.concatenate([c["w"][KEYS[0]], c["w"][KEYS[1]]]), A, L, eps, c["noise"][0])
        assert np.array_equal(a, sx.pooled(np.concatenate([c["w"][KEYS[0]], c["w"][KEYS[1]]]), A, L))


def test_crossed_cases_cover_every_value_the_kernels_branch_on():
    Ds, Ls, es, ns = (set(v[i] for v in edges.CASES.values()) for i in (0, 1, 2, 3))
    ns |= set(v[4] for v in edges.CASES.values())
    assert Ds == {1, 3, 4, 5, 16, 64, 100, 256} and Ls == {1, 2, 3, 4} and es == {0.0, 0.1, 1.0}
    assert ns == {1, edges.TB - 1, edges.TB, edges.TB + 1, 2 * edges.TN + 3}


def test_restated_draw_is_uniform_and_keyed_by_view_hop_and_step():
    L, n, D = 3, 50, 40
    a = sx.device_uniforms(1234, 0, L, n, D)
    assert a.shape == (2, L, n, D) and a.dtype == np.float32
    assert a.min() >= 0 and a.max() < 1 and np.array_equal(a * 16777216, np.round(a * 16777216)), "24-bit fractions in [0, 1)"
    assert abs(a.mean() - 0.5) < 0.01 and abs(a.var() - 1 / 12) < 0.005
    hist = np.histogram(a, bins=16, range=(0, 1))[0] / a.size
    assert np.abs(hist - 1 / 16).max() < 0.01
    flat = a.reshape(2 * L, -1)
    for i in range(2 * L):
        for j in range(i):
            assert abs(np.corrcoef(flat[i], flat[j])[0, 1]) < 0.05, "two (view, hop) pairs share their draw"
    b = sx.device_uniforms(1234, 1, L, n, D)
    c = sx.device_uniforms(1235, 0, L, n, D)
    assert abs(np.corrcoef(a.ravel(), b.ravel())[0, 1]) < 0.05 and abs(np.corrcoef(a.ravel(), c.ravel())[0, 1]) < 0.05
    assert np.array_equal(a, sx.device_uniforms(1234, 0, L, n, D))
    # a row's draw does not depend on how many rows there are (keyed by row * D + column)
    assert np.array_equal(sx.device_uniforms(1234, 0, L, n + 9, D)[:, :, :n], a)
