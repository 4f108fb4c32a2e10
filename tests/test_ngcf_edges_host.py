"""The inputs of tests/test_ngcf_edges_gpu.py hold what they claim, on the CPU: the forms csrc/ngcf.hip picks from each
width chain, the layout of every fixture (rows without edges, the hub row, the user / item seam inside a tile, mixed
signs, the clamp case's two populations), the fp32 restatement within REL of the fp64 one on every case and within a
third of the kernel's bound under other orders of its sums, a defect of each kind moving some asserted quantity by 10x what the GPU test's bound allows (with the fp64 restatement alone), and
the oracle's eps branch of the normalize backward against torch autograd.  CPU only; ``pytest -s`` shows the measured
margins."""
import numpy as np
import pytest

import ngcf_edges as ne
from helpers import assert_scalar_close, assert_tensor_close
from oracle import ngcf_numpy as onp

MIN_MARGIN = 10.0
F, U3 = "fused", "unfused"


def test_form_table():
    """``forms`` (the limits of csrc/ngcf.hip and sliced_width restated) gives the table written out by hand; every
    pair of (forward hop, backward) forms occurs, and slice widths 4, 2 and 0."""
    assert sorted(ne.FORM_TABLE) == sorted(ne.ALL_CASES)
    for key in ne.ALL_CASES:
        assert ne.forms(ne.fixture(key)) == ne.FORM_TABLE[key], key
    literal = {"w32_16_8": ((F, U3), "fused", 4), "w48_48_20": ((F, U3), "fused", 4),
               "w128_64_16": ((F, F), "per_hop", 4), "w64x5": ((F, F, F, F), "fused", 4),
               "w16x6": ((F,) * 5, "per_hop", 4), "w16x7": ((F,) * 6, "per_hop", 4),
               "w100_200_256": ((U3, U3), "per_hop", 4), "w10_6_12": ((U3, U3), "per_hop", 2),
               "w7_5_3": ((U3, U3), "per_hop", 0), "w16_18_16": ((U3, U3), "per_hop", 0),
               "hub16": ((F, F), "fused", 4), "hub10": ((U3, U3), "per_hop", 2)}
    for key, want in literal.items():
        assert ne.FORM_TABLE[key] == want, key
    pairs = {(f, bwd) for fwd, bwd, _ in ne.FORM_TABLE.values() for f in fwd}
    assert pairs == {(F, "fused"), (F, "per_hop"), (U3, "fused"), (U3, "per_hop")}
    assert {w for _, _, w in ne.FORM_TABLE.values()} == {4, 2, 0}
    # the shapes the issue names
    assert ne.fixture("w64x5").dims == [64] * 5 and 4 * 4 == ne.MAX_GROUP            # a group of exactly 16 problems
    assert len(ne.fixture("w16x7").dims) - 1 == ne.MAX_LAYERS
    assert ne.fixture("w128_64_16").dims[:2] == [ne.HOP_MAX_IN, ne.HOP_MAX_OUT]       # the largest fused forward
    assert max(ne.fixture("w100_200_256").dims) == ne.MAX_WIDTH
    assert [ne.sliced_width(66, d) for d in ne.fixture("w16_18_16").dims[:-1]] == [4, 2]
    c = ne.fixture("w10_6_12")
    assert (c.U + c.I) % 2 == 1 and all(((c.U + c.I) * d) % 4 for d in c.dims[:-1])   # bi_mul's scalar tail
    for key in ne.WIDTH_CASES:
        c = ne.fixture(key)
        assert 40 <= c.U + c.I <= 100 and len(c.batch[0]) <= 32


@pytest.mark.parametrize("key", ne.ALL_CASES)
def test_fixture_layout(key):
    """Both leaky-ReLU layers of every hop mix signs, with no pre-activation of the exact evaluation within 1e-4 of its
    layer's scale from zero; the batch is in range; the masks keep about 1 - p."""
    c = ne.fixture(key)
    N = c.U + c.I
    assert c.adj.shape == (N, N) and list(c.w) == list(onp.keys(len(c.dims) - 1))
    users, pos, neg = c.batch
    assert users.max() < c.U and max(pos.max(), neg.max()) < c.I and min(users.min(), pos.min(), neg.min()) >= 0
    for l, pres in enumerate(ne.pre_activations(c.w, c.adj, c.masks, c.drop)):
        for name, pre in zip(("sum_pre", "bi_pre"), pres):
            assert np.abs(pre).min() >= 1e-4 * np.abs(pre).max(), (l, name)
            assert 0.05 <= (pre <= 0).mean() <= 0.95, (l, name, float((pre <= 0).mean()))
    for l, p in enumerate(c.drop):
        assert (c.masks is None or c.masks[l] is None) == (p == 0)
        if p:
            assert c.masks[l].shape == (N, c.dims[l + 1]) and abs(c.masks[l].mean() - (1 - p)) < 0.1


def test_tile_and_batch_layout():
    assert {c.U + c.I for c in map(ne.fixture, ne.TILE_CASES)} == {9, 17, 64, 65}
    for key in ne.TILE_CASES:
        c = ne.fixture(key)
        assert c.dims == [16, 16, 16] and c.U % ne.HOP_ROWS != 0, "the user / item seam lies inside a 16-row tile"
    c = ne.fixture("one_user")
    users, pos, neg = c.batch
    assert len(set(users.tolist())) == 1 and set(pos.tolist()) | set(neg.tolist()) == {4, 9} and (pos == neg).sum() == 1
    assert c.dims == [32, 16, 8] and c.drop == [0.5, 0.3]
    c = ne.fixture("one_triple")
    assert len(c.batch[0]) == 1 and c.batch_size == 8 and c.drop == [0.5, 0.3]
    c = ne.fixture(ne.DROPPED_ROW_CASE)
    assert not c.masks[1][c.batch[0][0]].any() and not c.masks[0][c.U + c.batch[1][0]].any()
    ref = ne.reference(ne.DROPPED_ROW_CASE)
    off = c.dims[0] + c.dims[1]
    assert not ref.all64_train[c.batch[0][0], off:].any() and ref.all64_train[c.batch[0][1], off:].any()


@pytest.mark.parametrize("key", list(ne.GRAPH_CASES))
def test_graph_fixture_layout(key):
    """D^-1 A without the identity: at least three users and two items are rows without edges, one of each in the
    batch; the hub row is longer than a window of 16 chunks at lane_slots 16; and the host's builder, at the group
    count of a 256-CU device, lists the hub as a spill row and the edgeless nodes as empty rows in both graphs, under
    the factored form (``auto``) and with values."""
    from beta_recsys_amd.lightgcn import sliced_graph_host

    c = ne.fixture(key)
    N = c.U + c.I
    empty = ne.empty_rows(c)
    assert (empty < c.U).sum() >= 3 and (empty >= c.U).sum() >= 2 and c.adj.diagonal().max() == 0.0
    users, pos, neg = c.batch
    assert set(users.tolist()) & set(empty.tolist()) and (set((c.U + pos).tolist()) & set(empty.tolist()))
    assert len(np.setdiff1d(empty, np.concatenate([users, c.U + pos, c.U + neg]))) >= 3, "untouched edgeless nodes"
    hub = c.U + ne.HUB
    lens = np.diff(c.adj.indptr)
    assert lens[hub] == ne.HUB_USERS > ne.WINDOW_SLOTS and N <= 1400 and np.allclose(c.adj.sum(1)[lens > 0], 1.0)
    w = ne.slice_width(N, c.dims)
    n_groups = max(8, 256 // (max(c.dims[:-1]) // w) // 8 * 8)
    for graph in (c.adj, c.adj.T.tocsr()):
        for factor in (True, False):
            host = sliced_graph_host(graph.indptr, graph.indices, graph.data, None, n_groups, 512, factor=factor)
            assert host is not None and (("row_scale" in host) == factor)
            print(f"{key}: factored {factor}: lane_slots {host['lane_slots']}, spill rows {host['spill_row'].tolist()}, "
                  f"{host['empty_row'].size} empty rows")
            assert hub in host["spill_row"] and np.array_equal(host["empty_row"], empty)


def test_clamp_case_has_two_populations():
    """At least a quarter of the rows on each side of eps, none within 1e-3 relative of it, in fp32 and in fp64."""
    c = ne.fixture(ne.CLAMP_CASE)
    assert c.dims == [16, 16, 16] and c.masks is None
    N = c.U + c.I
    for dt in (np.float32, np.float64):
        nrm = ne.last_norms(c.w, c.adj, dt).astype(np.float64)
        below, above = int((nrm < ne.EPS).sum()), int((nrm >= ne.EPS).sum())
        nearest = float(np.abs(nrm / ne.EPS - 1.0).min())
        print(f"clamp {np.dtype(dt).name}: {below} rows below eps, {above} above, nearest {nearest:.3%} away")
        assert below >= N / 4 and above >= N / 4 and nearest >= 1e-3
    g = ne.reference(ne.CLAMP_CASE).g64
    print("clamp: last hop's gradient scales", {k: f"{np.abs(v).max():.2e}" for k, v in g.items() if ".1." in k})
    assert np.abs(g["GC_weights.1.weight"]).max() > 1e6


@pytest.mark.parametrize("key", ne.ALL_CASES)
def test_local_restatement_is_the_oracle(key):
    """``ne.restate`` without a defect is ``oracle.ngcf_numpy`` in both precisions."""
    c, ref = ne.fixture(key), ne.reference(key)
    for dt, loss, g in ((np.float64, ref.loss64, ref.g64), (np.float32, ref.loss32, ref.g32)):
        mine_loss, mine, _ = ne.restate(c, dt)
        assert_scalar_close(mine_loss, loss, 1e-6 if dt == np.float32 else 1e-13, what=f"{key} loss")
        for k in g:
            assert np.array_equal(mine[k], g[k]), (key, k)
    assert np.array_equal(ne.restate(c, train=False)[2], ref.all64)
    assert np.array_equal(ne.restate(c)[2], ref.all64_train)


@pytest.mark.parametrize("key", ne.ALL_CASES)
def test_fp32_restatement_is_a_fair_yardstick(key):
    """``assert_as_accurate_as_reference`` gives an implementation twice the fp32 restatement's own error on top of
    REL: on every case that error is itself below REL of the tensor's scale (or its ``terms`` floor), and the fp32 loss
    within REL.  A condition on the inputs."""
    ref = ne.reference(key)
    assert_scalar_close(ref.loss32, ref.loss64, what=f"{key}: fp32 loss")
    worst = 0.0
    for k in ref.g64:
        floor = ref.terms.get(k, 0.0)
        assert_tensor_close(ref.g32[k], ref.g64[k], what=f"{key}: fp32 {k}", scale_floor=floor)
        worst = max(worst, float(np.abs(ref.g32[k] - ref.g64[k]).max()) / max(float(np.abs(ref.g64[k]).max()), floor))
    print(f"{key}: the fp32 restatement's gradients are within {worst:.2e} of their scale of the exact ones")


@pytest.mark.parametrize("key", ne.ALL_CASES)
def test_another_summation_order_meets_the_bound(key):
    """The fixtures do not favour one order of the sums over nodes and edges: the fp32 oracle on ORDERS random
    renumberings of the nodes stays within ORDER_SHARE of the bound the kernel is held to.  (A third: the kernel's
    order is one more, and its MFMA tiles and atomics are not numpy's blocked sums.)"""
    ratios = [ne.other_order_ratio(key, s) for s in range(ne.ORDERS)]
    worst, what = max(ratios)
    print(f"{key}: {ne.ORDERS} other orders of the fp32 sums are within {worst:.2f} x the bound ({what})")
    assert worst <= ne.ORDER_SHARE


@pytest.mark.parametrize("key", ne.ALL_CASES)
def test_defects_are_visible(key):
    """Every defect the case's shape has moves the loss, a gradient or the eval-mode table by at least 10x its bound."""
    c = ne.fixture(key)
    claimed = [d for d in ne.DEFECTS if ne.applies(c, d)]
    assert claimed
    blind = {}
    for d in claimed:
        m, what = ne.defect_margin(key, d)
        print(f"{key}: {d} moves {what} by {m:.3g} x its bound")
        if not m >= MIN_MARGIN:
            blind[d] = (round(m, 2), what)
    assert not blind, f"{key}: the bounds cannot see these defects at {MIN_MARGIN:g} x: {blind}"


def test_every_defect_is_claimed_somewhere():
    claims = {d: [k for k in ne.ALL_CASES if ne.applies(ne.fixture(k), d)] for d in ne.DEFECTS}
    assert all(claims.values()), claims
    assert set(claims["spill_lost"]) == set(claims["empty_stale"]) == set(ne.GRAPH_CASES)
    assert set(claims["w2_second"]) == {"w10_6_12", "hub10"} and claims["cols64"] == ["w100_200_256"]
    assert ne.CLAMP_CASE in claims["big_inverted"] and {"n9", "n17", "n65"} <= set(claims["tile_rows"])
    # the clamp case sees the inverted selection in its gradients, not only in the loss or the table (which the
    # selection does not enter)
    m, what = ne.defect_margin(ne.CLAMP_CASE, "big_inverted")
    assert what not in ("loss", "all") and m >= MIN_MARGIN


@pytest.mark.parametrize("key", [ne.CLAMP_CASE, ne.DROPPED_ROW_CASE])
def test_oracle_eps_branch_matches_autograd(key):
    """``ngcf_grads(dt=float64)`` against torch autograd (CPU, float64, F.normalize, F.leaky_relu, torch.sparse.mm) to
    1e-12 of every tensor's scale: rows below eps, above it, and of norm exactly 0, which no golden reaches."""
    import torch
    import torch.nn.functional as Fn

    c, ref = ne.fixture(key), ne.reference(key)
    L, U = len(c.dims) - 1, c.U
    w = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in c.w.items()}
    co = c.adj.tocoo()
    adj = torch.sparse_coo_tensor(torch.tensor(np.vstack([co.row, co.col]), dtype=torch.int64),
                                  torch.tensor(co.data, dtype=torch.float64), co.shape)
    ego = torch.cat([w["user_embedding.weight"], w["item_embedding.weight"]], 0)
    outs = [ego]
    for l in range(L):
        side = torch.sparse.mm(adj, ego)
        s = Fn.leaky_relu(Fn.linear(side, w[f"GC_weights.{l}.weight"], w[f"GC_weights.{l}.bias"]))
        b = Fn.leaky_relu(Fn.linear(ego * side, w[f"Bi_weights.{l}.weight"], w[f"Bi_weights.{l}.bias"]))
        ego = s + b
        if c.masks is not None and c.masks[l] is not None:
            ego = ego * torch.tensor(c.masks[l].astype(np.float64) / (1.0 - c.drop[l]))
        outs.append(Fn.normalize(ego, p=2, dim=1))
    allv = torch.cat(outs, 1)
    users, pos, neg = (torch.tensor(x) for x in c.batch)
    u, p, n = allv[users], allv[U + pos], allv[U + neg]
    reg = (0.5 * (u ** 2).sum() + 0.5 * (p ** 2).sum() + 0.5 * (n ** 2).sum()) / c.batch_size
    loss = -Fn.logsigmoid((u * p).sum(1) - (u * n).sum(1)).mean() + c.decay * reg
    loss.backward()
    assert_scalar_close(float(loss.detach()), ref.loss64, 1e-12, what=f"{key}: loss")
    assert_tensor_close(allv.detach().numpy(), ref.all64_train, 1e-12, f"{key}: all")
    for k in ref.g64:
        assert_tensor_close(w[k].grad.numpy(), ref.g64[k], 1e-12, f"{key}: {k}")
    nrm = ne.last_norms(c.w, c.adj, np.float64, c.masks, c.drop)
    print(f"{key}: {(nrm == 0).sum()} rows of norm 0, {((nrm > 0) & (nrm < ne.EPS)).sum()} below eps, "
          f"{(nrm >= ne.EPS).sum()} above")
    assert (nrm < ne.EPS).any() and (nrm >= ne.EPS).any()
