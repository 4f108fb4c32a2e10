"""The inputs of tests/test_t2v_edges_gpu.py hold what they claim, on the CPU: the live columns of every slot at each
width, unit counts that leave waves idle, the triple astride the trip boundary, every stated collision, one lost unit
and one lost column moving the loss or some gradient by 10x what the GPU test's bound allows (with the fp64 restatement
alone), the fp32 restatement within REL of the fp64 one on every new case, and the hand-derived backward of the
restatement against torch's autograd in fp64, with shared and with independent item tables.  CPU only; ``pytest -s``
shows the measured margins."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import t2v_edges as te
from helpers import assert_scalar_close, assert_tensor_close, load_golden
from test_oracle_golden_t2v import CASES

MIN_MARGIN = 10.0
NEW_CASES = te.WIDTH_KEYS + list(te.NAMED_CASES)
KEYS = te.KEYS


def test_width_layout():
    """The live columns of the four slots ``lane + 64 k``; none of the new widths is one the goldens or
    tests/test_t2v_gpu.py run; the shapes of a width: 1, 3, 4, 5 units, n_neg == 0 on independent tables, and an
    ordinary count with shared and with independent tables."""
    assert te.WIDTH_CASES == (1, 3, 63, 65, 129, 193, 255)
    for D in te.WIDTH_CASES:
        assert te.live_columns(D) == te.LIVE[D] and sum(te.LIVE[D]) == D, D
    assert te.LIVE[65] == [64, 1, 0, 0] and te.LIVE[193] == [64, 64, 64, 1] and te.LIVE[255] == [64, 64, 64, 63]
    golden = {int(load_golden(case)["meta"][2]) for case in CASES}
    assert golden <= set(te.COVERED_ELSEWHERE) and not set(te.WIDTH_CASES) & set(te.COVERED_ELSEWHERE)
    units = [B * (1 + n) for _, B, n in te.WIDTH_SHAPES]
    assert {1, 3, 4, 5} < set(units) and max(units) > 4 * te.WAVES_PER_BLOCK
    assert all(not shared for shared, _, n in te.WIDTH_SHAPES if n == 0)
    assert {(shared, n > 0) for shared, _, n in te.WIDTH_SHAPES} == {(False, False), (True, True), (False, True)}
    assert all(B < te.BATCH_SIZE for _, B, _ in te.WIDTH_SHAPES)


@pytest.mark.parametrize("key", te.WIDTH_KEYS, ids=str)
def test_width_fixture_layout(key):
    """Tables of a few dozen rows with rows no batch names; negatives of shape [B, n_neg], [B, 0] included; the shared
    cases carry item_emb2 as a copy of item_emb1; logits O(1)."""
    D, shared, B, n_neg = key
    c = te.fixture(key)
    assert (c.D, c.shared, c.batch_size) == (D, shared, te.BATCH_SIZE) and te.n_units(c) == B * (1 + n_neg)
    assert [a.shape for a in c.batch] == [(B,)] * 3 + [(B, n_neg)] * 3
    assert c.w[te.UE].shape == (te.USERS, D) and c.w[te.E1].shape == c.w[te.E2].shape == (te.ITEMS, D)
    assert np.array_equal(c.w[te.E1], c.w[te.E2]) == shared
    assert max(a.max(initial=0) for a in (c.batch[0], c.batch[3])) < te.USERS - te.SPARE
    assert max(a.max(initial=0) for a in c.batch[1:3] + c.batch[4:]) < te.ITEMS - te.SPARE
    assert (c.batch[1] != c.batch[2]).all()
    pos, neg = te.logits(c)
    assert 0.05 < np.abs(pos).max() < 8.0 and (neg.size == 0 or np.abs(neg).max() < 8.0)


def test_stride_layout():
    """8196 units at D = 65 on 2048 blocks of 4 waves: triple 2730 has two units in the first trip and one in the
    second, triple 2731 lies in the second; units q and 8192 + q run on one wave."""
    c = te.fixture(te.STRIDE_CASE)
    B, n_neg = c.batch[3].shape
    assert (c.D, B, n_neg, c.shared, te.TRIP) == (65, 2732, 2, True, 8192) and te.n_units(c) == 8196
    assert -(-te.n_units(c) // te.WAVES_PER_BLOCK) > te.MAX_BLOCKS and c.batch_size > B
    assert [te.unit_of(q, n_neg) for q in range(te.TRIP - 2, te.TRIP + 4)] == [
        (2730, -1), (2730, 0), (2730, 1), (2731, -1), (2731, 0), (2731, 1)]
    assert [te.unit_of(q, n_neg) for q in range(4)] == [(0, -1), (0, 0), (0, 1), (1, -1)]
    assert (c.w[te.UE].shape[0], c.w[te.E1].shape[0]) == (1500, 1200)
    assert np.bincount(np.concatenate([c.batch[0], c.batch[3].ravel()])).max() <= 20


def test_saturated_and_collision_cases():
    """Positive and negative logits beyond +-30 with both signs; every collision the atomics must absorb, by name."""
    c = te.fixture(te.SATURATED_CASE)
    pos, neg = te.logits(c)
    print(f"saturated: positive logits {pos.min():.2f} .. {pos.max():.2f}, negative {neg.min():.2f} .. {neg.max():.2f}")
    assert pos.max() >= 30 and pos.min() <= -30 and neg.max() >= 30 and neg.min() <= -30 and not c.shared
    assert abs(min(pos.max(), -pos.min(), neg.max(), -neg.min()) - te.SATURATED_X) < 0.05
    assert np.isfinite(te.reference(te.SATURATED_CASE).loss64)
    for shared in (True, False):
        c = te.fixture(("collisions", shared))
        pu, p1, p2, nu, n1, n2 = c.batch
        assert c.shared == shared and nu.shape == (8, 3)
        assert (p1 == p2).tolist() == [True, False, False, False, False, True, False, False]
        assert nu[1, 0] == pu[1] and n2[2, 0] == p1[2] and n2[3, 1] == p2[3]
        assert all(a[4, 0] == a[4, 2] for a in (nu, n1, n2))
        assert nu[5, 0] == pu[5] and n2[5, 0] == p1[5] == p2[5] == n2[5, 1] and all(a[5, 0] == a[5, 2] for a in (nu, n1, n2))
        c = te.fixture(("hot", shared))
        assert c.batch[3].shape == (64, 3) and all(len(np.unique(a)) == 1 for a in c.batch) and c.batch_size > 64


def yardstick_error(c):
    """The fp32 restatement's loss and gradients held to REL of the fp64 ones, with the bias floors; returns the worst
    gradient error in units of its tensor's scale."""
    r = te.reference_of(c)
    floor = te.floor_fn(c)
    assert_scalar_close(r.loss32, r.loss64, what=f"{c.key}: fp32 loss")
    worst = 0.0
    for k in KEYS:
        assert_tensor_close(r.g32[k], r.g64[k], what=f"{c.key}: fp32 {k}", scale_floor=floor(k))
        scale = max(float(np.abs(r.g64[k]).max()), floor(k))
        worst = max(worst, float(np.abs(r.g32[k] - r.g64[k]).max()) / scale if scale else 0.0)
    if c.shared:
        assert not r.g64[te.E2].any() and not r.g32[te.E2].any()
    return worst


@pytest.mark.parametrize("key", NEW_CASES, ids=str)
def test_fp32_restatement_is_a_fair_yardstick(key):
    """``assert_grads_as_accurate`` gives an implementation twice the fp32 restatement's own error on top of REL: on
    every new case that error is itself below REL of the tensor's scale, and the fp32 loss within REL."""
    worst = yardstick_error(te.fixture(key))
    print(f"{key}: the fp32 restatement's gradients are within {worst:.2e} of their scale of the exact ones")


def test_saturation_threshold_the_restatement_holds():
    """The fp32 restatement holds REL at every magnitude from just past 30 to 80 (past 88 its exp(-x) is inf and its
    sigmoid the right 0.0: numpy's overflow warning is silenced)."""
    for x in te.SATURATED_SCAN:
        with np.errstate(over="ignore"):
            worst = yardstick_error(te.saturated_fixture(x))
        print(f"|logit| >= {x:g}: fp32 restatement within {worst:.2e} of scale")


def torch_grads(c):
    """The loss of triple2vec.py:36-92 in torch.float64 -- for each of the user, the first and the second item: the
    row against the sum of the other two plus its bias under logsigmoid, and the negatives' rows (users by u', both
    item tables by i2', the first item's bias by i1') against the row under logsigmoid(-.), summed and divided by
    3 x batch_size -- differentiated by autograd.  ``shared``: item_emb2 is item_emb1 and gets no gradient."""
    w = {k: torch.tensor(c.w[k], dtype=torch.float64, requires_grad=True) for k in KEYS}
    pu, p1, p2, nu, n1, n2 = (torch.from_numpy(np.asarray(a)) for a in c.batch)
    first, second = w[te.E1], w[te.E1] if c.shared else w[te.E2]
    bu, bi = w[te.UB][:, 0], w[te.IB][:, 0]
    rows = {"u": w[te.UE][pu], "1": first[p1], "2": second[p2]}
    total = 0.0
    for me, bias, neg_rows, neg_bias in (("u", bu[pu], w[te.UE][nu], bu[nu]), ("1", bi[p1], first[n2], bi[n1]),
                                         ("2", bi[p2], second[n2], bi[n2])):
        others = sum(v for k, v in rows.items() if k != me)
        total = total + F.logsigmoid((rows[me] * others).sum(1) + bias).sum()
        total = total + F.logsigmoid(-((neg_rows * rows[me][:, None, :]).sum(2) + neg_bias)).sum()
    loss = -total / (3 * c.batch_size)
    loss.backward()
    return float(loss.detach()), {k: (np.zeros(c.w[k].shape) if w[k].grad is None else w[k].grad.numpy()) for k in KEYS}


@pytest.mark.parametrize("key", NEW_CASES, ids=str)
def test_restatement_backward_matches_autograd(key):
    """The restatement's backward is derived by hand: in fp64 it agrees with autograd on the reference's forward to
    1e-12 of each tensor's scale, on every new fixture."""
    c, r = te.fixture(key), te.reference(key)
    loss, g = torch_grads(c)
    assert_scalar_close(loss, r.loss64, 1e-12, what=f"{key}: loss")
    worst = 0.0
    for k in KEYS:
        assert_tensor_close(r.g64[k], g[k], 1e-12, what=f"{key}: {k}")
        worst = max(worst, float(np.abs(r.g64[k] - g[k]).max()) / max(float(np.abs(g[k]).max()), 1e-300))
    print(f"{key}: fp64 restatement within {worst:.1e} of scale of autograd")


def check_units(key, units, what):
    """Every unit removed alone moves some gradient tensor (or the loss) by MIN_MARGIN x its tolerance; its last live
    column alone moves the row tensor it shows best in by as much.  Returns the two smallest margins."""
    whole, column = {}, {}
    for t, j in units:
        grad, loss, cols = te.unit_margins(key, t, j)
        whole[(t, j)] = max(grad, loss)
        column[(t, j)] = max(cols.values())
    blind = {u: round(m, 2) for u, m in whole.items() if m < MIN_MARGIN}
    assert not blind, f"{what}: the bound cannot see these units at {MIN_MARGIN:g} x: {blind}"
    return min(whole.values()), column


@pytest.mark.parametrize("D", te.WIDTH_CASES)
def test_width_cases_see_every_term(D):
    """Every unit (the positive group or negative j of a triple) of every shape of the width, and column D - 1 of the
    unit of each shape that shows it best, with the fp64 restatement alone."""
    smallest, smallest_col = np.inf, np.inf
    for key in te.WIDTH_KEYS:
        if key[0] != D:
            continue
        _, _, B, n_neg = key
        m, column = check_units(key, [(t, j) for t in range(B) for j in range(-1, n_neg)], f"{key}")
        smallest = min(smallest, m)
        assert max(column.values()) >= MIN_MARGIN, f"{key}: column {D - 1} is blind: {column}"
        smallest_col = min(smallest_col, max(column.values()))
    print(f"D {D}: smallest margins: one unit {smallest:.1f}, column {D - 1} {smallest_col:.1f}")


def test_stride_case_sees_every_second_trip_unit():
    """The four units of the second trip and their wave partners, units 0 .. 3."""
    c = te.fixture(te.STRIDE_CASE)
    n_neg = c.batch[3].shape[1]
    units = [te.unit_of(q, n_neg) for q in list(range(4)) + list(range(te.TRIP, te.n_units(c)))]
    m, _ = check_units(te.STRIDE_CASE, units, "stride")
    print(f"stride: smallest margin of one unit {m:.1f}")
