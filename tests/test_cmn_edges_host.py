"""The inputs of tests/test_cmn_edges_gpu.py hold what they claim, on the CPU: the numbers the kernel derives from each
width, lists at the seams of that width's round, a row lost at a seam moving some gradient by 10x what the GPU test's
bound allows (with the fp64 restatement alone), the fp32 restatement within REL of the fp64 one on every new case (the
sharp and the saturated ones included, where that is not a given), and the sharp / saturated cases' shape.  CPU only;
``pytest -s`` shows the measured margins."""
import numpy as np
import pytest

import cmn_edges as ce
from helpers import assert_scalar_close, assert_tensor_close

MIN_MARGIN = 10.0
NEW_CASES = ce.WIDTH_CASES + [ce.STRIDE_CASE] + ce.SHARP_CASES + [ce.DUPLICATE_CASE, ce.SATURATED_CASE]


def lists_of(c):
    return [c.col[c.rowptr[i]:c.rowptr[i + 1]] for i in range(len(c.rowptr) - 1)]


def test_derived_numbers():
    """Part 1.  The restatement of cmn_lanes_per_row / Dp gives the table's values; with the widths the older tests run,
    every (G, VEC) pair occurs but (1, no vector), which D >= 4 rules out."""
    assert ce.WIDTH_CASES == [4, 8, 10, 12, 30, 50, 65, 68, 130, 132]
    for D in ce.WIDTH_CASES:
        assert ce.derived(D) == ce.DERIVED[D], D
        G, R, vec, Dp, rpi = ce.derived(D)
        assert G * R == 64 and 4 * G >= D and (G == 1 or 2 * G < D) and Dp * rpi == 64 and (Dp == 64 or D <= Dp < 2 * D)
    assert [ce.derived(D)[:3:2] for D in ce.COVERED_ELSEWHERE] == [(2, False), (4, True), (8, True), (16, True),
                                                                    (32, True), (64, True)]
    pairs = {ce.derived(D)[:3:2] for D in tuple(ce.WIDTH_CASES) + ce.COVERED_ELSEWHERE}
    assert pairs == {(g, v) for g in (1, 2, 4, 8, 16, 32, 64) for v in (True, False)} - {(1, False)}
    # the upper k slots of the scatter hold one and two live columns at D = 65 and 130, idle float4 lanes at 68 and 132
    live = {D: [sum(c0 + 64 * k < D for c0 in range(64)) for k in range(4)] for D in (65, 130)}
    assert live == {65: [64, 1, 0, 0], 130: [64, 64, 2, 0]}
    for D in (68, 132):
        G = ce.derived(D)[0]
        assert 4 * (G - 1) >= D and D % 4 == 0


@pytest.mark.parametrize("D", ce.WIDTH_CASES)
def test_width_fixture_layout(D):
    """Lengths from R(D); every length a positive and a negative list; an item on both sides; the hub in most lists; a
    sample's user in its own positive list; no list with a repeat; users nothing refers to; both ReLU layers mixed with
    no pre-activation of the exact evaluation within 1e-4 of its layer's scale from zero."""
    c = ce.fixture(D)
    R = ce.derived(D)[1]
    lengths = ce.width_lengths(D)
    want = {1, R + 1, 4 * R - 1, 4 * R, 4 * R + 1, 8 * R + 1} | ({R - 1} if R > 1 else set())
    assert want <= set(lengths) and len(set(lengths) - want) == 2 and len(set(lengths)) == len(lengths)
    lists = lists_of(c)
    assert [len(x) for x in lists] == lengths
    users, pos, neg = c.triples
    assert len(users) <= 12 and set(pos.tolist()) == set(neg.tolist()) == set(range(len(lengths)))
    assert set(pos.tolist()) & set(neg.tolist())
    U = c.w["user_memory.weight"].shape[0]
    assert U == 8 * R + 40 and all(len(set(x.tolist())) == len(x) for x in lists)
    assert sum(ce.HUB in x for x in lists) >= len(lists) - 3
    assert any(u in lists[p] for u, p in zip(users, pos))
    referred = set(c.col.tolist()) | set(users.tolist())
    assert len(set(range(U)) - referred) >= ce.SPARE_USERS
    for layer, pre in ce.pre_activations(c.w, c.batch).items():
        assert np.abs(pre).min() >= 1e-4 * np.abs(pre).max(), layer
        assert 0.25 <= (pre <= 0).mean() <= 0.75, layer
    a0 = ce.hop_logits(c.w, c.batch, 0, 0)
    print(f"D {D}: hop-0 logits std {np.nanstd(a0):.2f}, {np.nanmin(a0):.2f} .. {np.nanmax(a0):.2f}")
    assert 1.0 <= np.nanstd(a0) <= 3.0


@pytest.mark.parametrize("D", ce.WIDTH_CASES)
def test_seam_rows_are_visible(D):
    """Part 2.  The 4 R + 1 list without its last neighbour (the one row of its last round), and without the first and
    the last neighbour of its last full round; the 8 R + 1 list likewise: some tensor of the fp64 gradient moves by at
    least 10x its tolerance."""
    R = ce.derived(D)[1]
    margins = {(L, row): ce.drop_margin(D, L, row)
               for L, row in ((4 * R + 1, 4 * R), (4 * R + 1, 0), (4 * R + 1, 4 * R - 1), (8 * R + 1, 8 * R),
                              (8 * R + 1, 4 * R))}
    for (L, row), m in margins.items():
        print(f"D {D}: list of {L} without row {row} moves a gradient by {m:.1f} x its tolerance")
    print(f"D {D}: smallest margin {min(margins.values()):.1f}")
    blind = {k: round(m, 2) for k, m in margins.items() if m < MIN_MARGIN}
    assert not blind, f"the gradient bound cannot see these rows at {MIN_MARGIN:g} x: {blind}"


def yardstick_error(c):
    """The fp32 restatement's loss and gradients held to REL of the fp64 ones; returns the worst gradient error in
    units of its tensor's scale."""
    loss64, g64, total64 = ce.exact_grads(c.w, c.batch, c.lam, c.clip)
    floors = ce.term_floors(c.w, c.batch, c.lam, c.clip)
    loss32, total32, g32 = ce.restated32(c)
    assert_scalar_close(loss32, loss64, what=f"{c.key}: fp32 loss")
    assert_scalar_close(total32, total64, what=f"{c.key}: fp32 norm")
    for k in ce.KEYS:
        assert_tensor_close(g32[k], g64[k], what=f"{c.key}: fp32 {k}", scale_floor=floors[k])
    return max(float(np.abs(g32[k] - g64[k]).max()) / max(float(np.abs(g64[k]).max()), floors[k]) for k in ce.KEYS)


@pytest.mark.parametrize("key", NEW_CASES, ids=str)
def test_fp32_restatement_is_a_fair_yardstick(key):
    """Part 3.  ``assert_grads_as_accurate`` gives an implementation twice the fp32 restatement's own error on top of
    REL: on every new case that error is itself below REL of the tensor's scale, and the fp32 loss within REL."""
    worst = yardstick_error(ce.fixture(key))
    print(f"{key}: the fp32 restatement's gradients are within {worst:.2e} of their scale of the exact ones")


@pytest.mark.parametrize("key", NEW_CASES, ids=str)
def test_both_softmax_backward_forms_meet_the_bound(key):
    """The fixtures do not favour one way of writing the softmax's backward: the fp32 restatement with
    delta = do . o (the kernel's form) instead of sum_j p_j dp_j meets the bound the kernel is held to.  (A list whose
    rows share a long common component fails this: see SHARP_Z0_NORM.)"""
    c = ce.fixture(key)
    _, g64, _, g32, floors = ce.reference(key)
    tol = ce.tolerances(g32, g64, floors)
    _, _, alt = ce.restated32(c, delta_from_output=True)
    ratio = {k: float(np.abs(alt[k] - g64[k]).max()) / tol[k] for k in ce.KEYS}
    worst = max(ratio, key=ratio.get)
    print(f"{key}: the other form is within {ratio[worst]:.2f} x the bound ({worst})")
    assert ratio[worst] <= 1.0


def test_saturation_threshold_the_restatement_holds():
    """Part 3, the saturated case: the fp32 restatement holds REL at every |x| from just past 30 to 80."""
    for x in ce.SATURATED_SCAN:
        worst = yardstick_error(ce.saturated_fixture(x))
        print(f"|x| = {x:g}: fp32 restatement within {worst:.2e} of scale")


@pytest.mark.parametrize("D,shape", ce.SHARP_CASES)
def test_sharp_logits_have_the_stated_shape(D, shape):
    """Part 4.  One list of 4 R x 3 + 1 rows on both sides of sample 0; hop-0 logits ascending / descending / flat with
    one late peak on either side, spread 60 .. 80, |logit| <= 40."""
    c = ce.fixture((D, shape))
    R = ce.derived(D)[1]
    L = 12 * R + 1
    u, p, n, pn, pl, nn_, nl = c.batch
    assert pl.tolist() == nl.tolist() == [L, L] and np.array_equal(pn[0], nn_[0]) and p[0] != n[0]
    assert len(set(pn[0].tolist())) == L and u[0] not in pn[0]
    for side in (0, 1):
        a = ce.hop_logits(c.w, c.batch, side, 0)
        a1 = ce.hop_logits(c.w, c.batch, side, 1)
        for b in (0, 1):
            row = np.roll(a[b], -(R + 1)) if c.batch[1 + side][b] == 2 else a[b]   # item 2's list is the rotated one
            spread = row.max() - row.min()
            print(f"D {D} {shape} side {side} sample {b}: hop-0 logits {row.min():.2f} .. {row.max():.2f}, hop-1 spread "
                  f"{np.nanmax(a1[b]) - np.nanmin(a1[b]):.1f}")
            assert 60.0 <= spread <= 80.0 and np.abs(row).max() <= 40.0
            if shape == "ascending":
                assert (np.diff(row) > 0).all()
            elif shape == "descending":
                assert (np.diff(row) < 0).all()
            else:
                peak = int(np.argmax(row))
                rest = np.delete(row, peak)
                assert peak == L - 3 and 8 * R <= peak < 12 * R and rest.max() - rest.min() < 1e-3


def test_stride_and_duplicate_layout():
    c = ce.fixture(ce.STRIDE_CASE)
    users, pos, neg = c.triples
    assert c.D == 8 and len(users) == 1030 > ce.MAX_BLOCKS and c.w["user_memory.weight"].shape[0] == 40
    assert len(c.rowptr) - 1 <= 6 and set(np.diff(c.rowptr).tolist()) == {1, 2, 3, 4, 5}
    assert (pos[0], neg[0]) != (pos[1024], neg[1024]) or users[0] != users[1024]
    c = ce.fixture(ce.DUPLICATE_CASE)
    u, p, n, pn, pl, nn_, nl = c.batch
    assert c.D == 20 and len(u) == 3 and c.triples is None
    first = pn[0, :pl[0]].tolist()
    rep = first[-1]
    assert first.count(rep) == 3 and len(set(first)) == len(first) - 2
    assert set(nn_[1, :nl[1]].tolist()) == {int(nn_[1, 0])} and nl[1] > 1


def test_saturated_case():
    """Part 4.  x <= -30 on one sample and >= +30 on the other; the exact loss finite, the exact gradient of the
    x <= -30 sample alone non-zero."""
    c = ce.fixture(ce.SATURATED_CASE)
    x = ce.score_differences(c.w, c.batch)
    print(f"saturated: x = {x.tolist()}")
    assert x.min() <= -30.0 and x.max() >= 30.0
    u, p, n, pn, pl, nn_, nl = c.batch
    assert (p[1], n[1], u[1]) == (n[0], p[0], u[0])
    loss64, g64, _, _, _ = ce.reference(ce.SATURATED_CASE)
    assert np.isfinite(loss64) and loss64 > 0.5 * 27.0
    b = int(np.argmin(x))
    one = tuple(a[b:b + 1] for a in c.batch)
    _, g_one, _ = ce.exact_grads(c.w, one, 0.0, c.clip)
    assert all(np.isfinite(v).all() for v in g_one.values())
    assert float(np.abs(g_one["user_output.weight"]).max()) > 1e-3 and float(np.abs(g_one["out.weight"]).max()) > 1e-3
