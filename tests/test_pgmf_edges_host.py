"""The inputs of tests/test_pgmf_edges_gpu.py hold what they claim, on the CPU: the live columns of every slot at each
width, block counts at the seams of the finish kernel's unrolling, the kinds of the triples that share a wave across the
trip boundary, one lost triple / one lost block of grad v / one lost column moving the loss or some gradient by 10x what
the GPU test's bound allows (with the fp64 restatement alone), the fp32 restatement within REL of the fp64 one on every
new case, and the hand-derived backward of the restatement against torch's autograd in fp64.  CPU only; ``pytest -s``
shows the measured margins."""
import numpy as np
import pytest
import torch

import pgmf_edges as pe
from helpers import REL, assert_scalar_close, assert_tensor_close, load_golden
from oracle import pgmf_numpy as pn
from test_oracle_golden_pgmf import CASES

MIN_MARGIN = 10.0
NEW_CASES = pe.WIDTH_KEYS + list(pe.NAMED_CASES)
KEYS = pe.KEYS


def test_width_layout():
    """The live columns of the four slots ``lane + 64 k``; none of the new widths is one the goldens or
    tests/test_pgmf_gpu.py run."""
    assert pe.WIDTH_CASES == (1, 3, 63, 65, 129, 193, 255)
    for D in pe.WIDTH_CASES:
        assert pe.live_columns(D) == pe.LIVE[D] and sum(pe.LIVE[D]) == D, D
    assert pe.LIVE[65] == [64, 1, 0, 0] and pe.LIVE[193] == [64, 64, 64, 1] and pe.LIVE[255] == [64, 64, 64, 63]
    golden = {int(load_golden(case)["meta"][2]) for case in CASES}
    assert golden <= set(pe.COVERED_ELSEWHERE) and not set(pe.WIDTH_CASES) & set(pe.COVERED_ELSEWHERE)
    assert min(pe.COVERED_ELSEWHERE) == 8 and {1, 3} < set(pe.WIDTH_CASES)


def test_finish_kernel_seams():
    """The block counts ceil(B / 4) of every width: 1, n_slices - 1 .. + 1, 4 n_slices - 1 .. + 1; with them both the
    unrolled loop and the remainder loop of the fold are entered, and 4 n_slices blocks run the unrolled loop alone.
    D = 1 and 3 (n_slices 1024 and 341) keep the small counts: remainder loop only."""
    assert pe.width_batch_sizes(255) == [4, 12, 16, 20, 60, 64, 68]
    assert pe.width_batch_sizes(1) == pe.width_batch_sizes(3) == [1, 2, 3, 4, 5]
    for D in pe.WIDTH_CASES:
        ns = pe.FINISH_THREADS // D
        sizes = pe.width_batch_sizes(D)
        blocks = [pe.n_blocks(B) for B in sizes]
        split = {nb: pe.finish_split(D, nb) for nb in blocks}
        assert all(s[0] == ns and s[1] * 4 + s[2] == nb for nb, s in split.items()), D
        print(f"D {D}: n_slices {ns}, batches {sizes}, (unrolled, remainder) bodies "
              f"{[split[nb][1:] for nb in blocks]}")
        if D in (1, 3):
            assert max(blocks) == 2 and all(s[1] == 0 for s in split.values())
            continue
        assert blocks == sorted({1, ns - 1, ns, ns + 1, 4 * ns - 1, 4 * ns, 4 * ns + 1}), D
        assert any(s[1] > 0 for s in split.values()) and any(s[2] > 0 for s in split.values())
        assert split[4 * ns][1:] == (ns, 0) and split[4 * ns - 1][1:] == (ns - 1, 3)
        assert split[4 * ns + 1][1:] == (ns, 1) and split[1][1:] == (0, 1)
        assert all(B == 4 * nb for B, nb in zip(sizes, blocks))


@pytest.mark.parametrize("D", pe.WIDTH_CASES)
def test_width_fixture_layout(D):
    """Tables of a few dozen rows with rows no triple names; pos != neg; no pre-activation of the exact evaluation
    within GATE_MARGIN of zero; every block of four holds a triple with an open ReLU; about a quarter of the triples
    have both closed and about half have one closed."""
    kinds_all = []
    for B in pe.width_batch_sizes(D):
        c = pe.fixture((D, B))
        u, p, q = c.batch
        assert c.D == D and len(u) == len(p) == len(q) == B and c.w[pe.V].shape == (1, D)
        assert c.w[pe.UM].shape == (pe.USERS, D) and c.w[pe.IM].shape == (pe.ITEMS, D)
        assert u.max() < pe.USERS - pe.SPARE and max(p.max(), q.max()) < pe.ITEMS - pe.SPARE and (p != q).all()
        pp, pq = pe.pre_activations(c.w, c.batch)
        assert min(np.abs(pp).min(), np.abs(pq).min()) >= pe.GATE_MARGIN
        kind = pe.kinds(c.w, c.batch)
        for first in range(0, B, 4):
            assert (kind[first:first + 4] != "closed").any(), (D, B, first)
        kinds_all.append(kind)
    kind = np.concatenate(kinds_all)
    closed, one = (kind == "closed").mean(), np.isin(kind, ("pos_only", "neg_only")).mean()
    print(f"D {D}: {len(kind)} triples, both ReLUs closed {closed:.2f}, one closed {one:.2f}")
    if len(kind) >= 100:
        assert 0.1 <= closed <= 0.4 and 0.3 <= one <= 0.85


def test_stride_layout():
    """TRIP + 6 triples at D = 65: triples w and TRIP + w run on one wave, and for w = 0 .. 5 they are (open, open),
    (both closed, open), (open, both closed), (only s+ open, only s- open), (both closed, both closed),
    (pos == neg, open), read off the fp64 pre-activations; a row receives a few terms only."""
    c = pe.fixture(pe.STRIDE_CASE)
    u, p, q = c.batch
    B = len(u)
    assert (c.D, B, pe.TRIP) == (65, 4096 + 6, 4096) and pe.n_blocks(B) == pe.MAX_BLOCKS
    assert (c.w[pe.UM].shape[0], c.w[pe.IM].shape[0]) == (1500, 1200)
    kind = pe.kinds(c.w, c.batch)
    for wv, pair in enumerate(pe.STRIDE_PAIRS):
        for t, want in zip((wv, pe.TRIP + wv), pair):
            if want == "same_item":
                assert p[t] == q[t] and kind[t] == "open"
            else:
                assert kind[t] == want and p[t] != q[t], (t, kind[t], want)
    assert len(pe.STRIDE_PAIRS) == B - pe.TRIP and (p != q).sum() == B - 1
    pp, pq = pe.pre_activations(c.w, c.batch)
    assert min(np.abs(pp).min(), np.abs(pq).min()) >= pe.GATE_MARGIN
    assert np.bincount(u).max() <= 12 and np.bincount(np.concatenate([p, q])).max() <= 24


def test_gate_saturation_and_collision_cases():
    """Every triple of the closed case has both ReLUs closed: the exact loss is -log(0.5 + 1e-12) + lambda |v| and
    every gradient but v's lambda term is exactly 0.0.  The saturated case reaches |x| = 32 with both signs and keeps a
    gradient on the x = -32 side.  The collision cases collide as stated."""
    c = pe.fixture(pe.CLOSED_CASE)
    assert len(c.batch[0]) == 37 and (pe.kinds(c.w, c.batch) == "closed").all()
    r = pe.reference(pe.CLOSED_CASE)
    v64 = c.w[pe.V].astype(np.float64)
    norm = float(np.sqrt((v64 ** 2).sum()))
    assert abs(r.loss64 - (-np.log(0.5 + float(pn.EPS)) + c.lam * norm)) < 1e-14
    assert not r.g64[pe.UM].any() and not r.g64[pe.IM].any() and not r.g32[pe.UM].any() and not r.g32[pe.IM].any()
    assert np.abs(r.g64[pe.V] - c.lam * v64 / norm).max() < 1e-18

    c = pe.fixture(pe.SATURATED_CASE)
    x = pe.score_differences(c.w, c.batch)
    print(f"saturated: x from {x.min():.3f} to {x.max():.3f}, |x| >= 30 on {(np.abs(x) >= 30).sum()} of {len(x)}")
    assert x.min() <= -30.0 and x.max() >= 30.0 and abs(np.abs(x).max() - pe.SATURATED_X) < 1e-3 and c.clip == pe.NO_CLIP
    r = pe.reference(pe.SATURATED_CASE)
    assert np.isfinite(r.loss64) and r.loss64 > 27.0 / len(x)
    _, g_one = pe.terms(c, int(np.argmin(x)))
    assert all(np.isfinite(v).all() for v in g_one.values()) and float(np.abs(g_one[pe.UM]).max()) > 1e-4

    c = pe.fixture(pe.SAME_ITEM_CASE)
    u, p, q = c.batch
    assert (p[::2] == q[::2]).all() and (p[1::2] != q[1::2]).all()
    assert (pe.kinds(c.w, c.batch)[::2] == "open").any() and (pe.score_differences(c.w, c.batch)[::2] == 0.0).all()
    c = pe.fixture(pe.ONE_USER_CASE)
    assert len(c.batch[0]) == 37 and len(set(c.batch[0].tolist())) == 1
    assert np.count_nonzero(np.abs(pe.reference(pe.ONE_USER_CASE).g64[pe.UM]).max(axis=1)) == 1
    c = pe.fixture(pe.HOT_CASE)
    assert len(c.batch[0]) == 64 and all(len(set(a.tolist())) == 1 for a in c.batch)
    assert (pe.kinds(c.w, c.batch) == "open").all()


def test_clip_is_active():
    """The clip is active on every case that carries one, so that ``clip=True`` checks a scaled gradient -- but on the
    all-closed case, whose whole gradient is the lambda term of norm lambda: there the inactive clip is what is run."""
    for key in NEW_CASES:
        c, r = pe.fixture(key), pe.reference(key)
        if key == pe.CLOSED_CASE:
            assert r.coef64 == 1.0 and abs(r.total64 - c.lam) < 1e-15
        elif c.clip != pe.NO_CLIP:
            assert r.coef64 < 0.95, (key, r.total64)


def yardstick_error(c):
    """The fp32 restatement's loss, norm and gradients held to REL of the fp64 ones; returns the worst gradient error
    in units of its tensor's scale."""
    r = pe.reference_of(c)
    assert_scalar_close(r.loss32, r.loss64, what=f"{c.key}: fp32 loss")
    assert_scalar_close(r.total32, r.total64, what=f"{c.key}: fp32 norm")
    for k in KEYS:
        assert_tensor_close(r.g32[k], r.g64[k], what=f"{c.key}: fp32 {k}")
        assert_tensor_close(r.g32_clipped[k], r.g64[k] * r.coef64, what=f"{c.key}: clipped fp32 {k}")
    return max(float(np.abs(r.g32[k] - r.g64[k]).max()) / max(float(np.abs(r.g64[k]).max()), 1e-300) for k in KEYS)


@pytest.mark.parametrize("key", NEW_CASES, ids=str)
def test_fp32_restatement_is_a_fair_yardstick(key):
    """``assert_grads_as_accurate`` gives an implementation twice the fp32 restatement's own error on top of REL: on
    every new case that error is itself below REL of the tensor's scale, and the fp32 loss and norm are within REL."""
    worst = yardstick_error(pe.fixture(key))
    print(f"{key}: the fp32 restatement's gradients are within {worst:.2e} of their scale of the exact ones")


def test_saturation_threshold_the_restatement_holds():
    """The fp32 restatement holds REL at every |x| from just past 30 to 80."""
    for x in pe.SATURATED_SCAN:
        worst = yardstick_error(pe.saturated_fixture(x))
        print(f"|x| = {x:g}: fp32 restatement within {worst:.2e} of scale")


def torch_grads(c):
    """relu(v . (u * i)), mean(-log(sigmoid(s+ - s-) + eps)) + lambda sqrt(sum v^2) in torch.float64, differentiated
    by autograd.  eps is the fp32 1e-12 the restatement (and the kernel) adds."""
    w = {k: torch.tensor(c.w[k], dtype=torch.float64, requires_grad=True) for k in KEYS}
    u, p, q = (torch.from_numpy(np.asarray(a)) for a in c.batch)
    v = w[pe.V][0]
    sp = torch.relu((w[pe.UM][u] * w[pe.IM][p]) @ v)
    sn = torch.relu((w[pe.UM][u] * w[pe.IM][q]) @ v)
    loss = (-torch.log(torch.sigmoid(sp - sn) + float(pn.EPS))).mean() + c.lam * torch.sqrt((v * v).sum())
    loss.backward()
    return float(loss.detach()), {k: w[k].grad.numpy() for k in KEYS}


@pytest.mark.parametrize("key", NEW_CASES, ids=str)
def test_restatement_backward_matches_autograd(key):
    """The restatement's backward is derived by hand: in fp64 it agrees with autograd on the same forward to 1e-12 of
    each tensor's scale, on every new fixture."""
    c, r = pe.fixture(key), pe.reference(key)
    loss, g = torch_grads(c)
    assert_scalar_close(loss, r.loss64, 1e-12, what=f"{key}: loss")
    worst = 0.0
    for k in KEYS:
        assert_tensor_close(r.g64[k], g[k], 1e-12, what=f"{key}: {k}")
        worst = max(worst, float(np.abs(r.g64[k] - g[k]).max()) / max(float(np.abs(g[k]).max()), 1e-300))
    print(f"{key}: fp64 restatement within {worst:.1e} of scale of autograd")


def check_triples(key, triples, what):
    """Every triple of ``triples`` removed alone: an open ReLU -> some gradient tensor moves by MIN_MARGIN x its
    tolerance, both closed -> the loss does.  Returns the smallest margin."""
    c = pe.fixture(key)
    kind = pe.kinds(c.w, c.batch)
    margins = {}
    for t in triples:
        grad, _, loss = pe.removal_margins(key, t)
        same_item = c.batch[1][t] == c.batch[2][t]     # pos == neg: every update of the triple cancels, the loss stays
        margins[t] = loss if kind[t] == "closed" or same_item else grad
    blind = {t: round(m, 2) for t, m in margins.items() if m < MIN_MARGIN}
    assert not blind, f"{what}: the bound cannot see these triples at {MIN_MARGIN:g} x: {blind}"
    return min(margins.values())


def check_blocks(key, firsts, what):
    """Grad v without one block's four triples moves by MIN_MARGIN x its tolerance."""
    B = len(pe.fixture(key).batch[0])
    margins = {f: pe.removal_margins(key, np.arange(f, min(f + 4, B)))[1] for f in firsts}
    blind = {f: round(m, 2) for f, m in margins.items() if m < MIN_MARGIN}
    assert not blind, f"{what}: the bound on grad v cannot see these blocks at {MIN_MARGIN:g} x: {blind}"
    return min(margins.values())


@pytest.mark.parametrize("D", pe.WIDTH_CASES)
def test_width_cases_see_every_term(D):
    """Every triple, every block's partial of grad v and the last live column (D - 1) of a triple's updates, at every
    batch size of the width, with the fp64 restatement alone."""
    smallest = {"triple": np.inf, "block": np.inf, "column": np.inf}
    for B in pe.width_batch_sizes(D):
        key = (D, B)
        c = pe.fixture(key)
        smallest["triple"] = min(smallest["triple"], check_triples(key, range(B), f"D {D} B {B}"))
        smallest["block"] = min(smallest["block"], check_blocks(key, range(0, B, 4), f"D {D} B {B}"))
        # the last live column: for each of the four places it is written (the user's row, the items' rows, grad v)
        # the triple of the batch that shows its loss best
        kind = pe.kinds(c.w, c.batch)
        cols = [pe.column_margin(key, t, D - 1) for t in range(B) if kind[t] != "closed"]
        best = {k: max(m[k] for m in cols) for k in KEYS}
        assert min(best.values()) >= MIN_MARGIN, f"D {D} B {B}: column {D - 1} is blind: {best}"
        smallest["column"] = min(smallest["column"], min(best.values()))
    print(f"D {D}: smallest margins: one triple {smallest['triple']:.1f}, one block of grad v {smallest['block']:.1f}, "
          f"column {D - 1} {smallest['column']:.1f}")


def test_stride_case_sees_every_second_trip_term():
    """The six triples of the second trip and their wave partners, and the two blocks of grad v that run a second trip."""
    key = pe.STRIDE_CASE
    n = len(pe.STRIDE_PAIRS)
    triples = list(range(n)) + list(range(pe.TRIP, pe.TRIP + n))
    m_t = check_triples(key, triples, "stride")
    # blocks 0 and 1 hold the second trip: what they would lose with it, and with their first trip
    m_b = check_blocks(key, [pe.TRIP, pe.TRIP + 4, 0, 4], "stride")
    print(f"stride: smallest margins: one triple {m_t:.1f}, one block's trip of grad v {m_b:.1f}")
