"""Pin tests/tisasrec_numpy.py against golden vectors captured from the real reference's TiSASRecEngine by
``tools/gen_golden_tisasrec.py``, and the host-side parts of the TiSASRec mirror.  CPU only.

One tolerance differs from tests/test_oracle_golden_sasrec.py, for a quantity SASRec does not have on its own:
``attention_layers.{b}.K_w.bias``.  A key bias cancels in the softmax, so that tensor's exact gradient is zero while the
terms it sums are not; ``tisasrec_edges.key_bias_floor`` holds it to REL of the scale of those terms (SASRec's key bias
is a third of ``in_proj_bias`` and rides on the scale of the other two thirds)."""
import contextlib
import io

import numpy as np
import pytest
import torch

import tisasrec_edges as te
import tisasrec_numpy as tn
from helpers import REL, assert_grads_as_accurate, assert_scalar_close, assert_step_close
from helpers import copy_state, float64_oracle, load_golden, to64

CASES = ["tisasrec_adam", "tisasrec_sgd_h1", "tisasrec_rmsprop_drop"]
STATE_NAMES = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg",), "sgd": ()}
STATE_TAGS = {"exp_avg": "m", "exp_avg_sq": "v", "square_avg": "v"}
# A flipped byte must move a gradient by MORE THAN TWICE what the GPU test's bound allows: a correct kernel may itself
# sit one bound away from the exact gradient, so a move of 2 x is what is certain to land outside the bound.
MIN_MARGIN = 2.0


def meta(g):
    """(I, T, D, H, blocks, B, steps, seed, time_span)"""
    return tuple(int(x) for x in g["meta"])


def hyper(g):
    """(optimizer, lr, l2_emb, dropout rate)"""
    return str(g["optimizer"]), float(g["lr"]), float(g["l2_emb"]), float(g["dropout_rate"])


def tis_keys(g):
    return tn.keys(meta(g)[4])


def tis_params(case, g, step, tag="w"):
    """Tensor set ``tag`` (w / g / m / v) of the reference after ``step`` steps (w after 0 steps: the initial weights)."""
    if step == 0 and tag == "w":
        return {k: g[f"w0/{k}"].astype(np.float32).copy() for k in tis_keys(g)}
    s = load_golden(f"{case}_s{step}")
    return {k: s[f"{tag}/{k}"].astype(np.float32).copy() for k in tis_keys(g)}


def tis_batch(g, s):
    """(seq, time_matrix, pos, neg) of step ``s``."""
    return g["seq"][s], g["time_matrix"][s], g["pos"][s], g["neg"][s]


def tis_keep(g, s):
    if float(g["dropout_rate"]) == 0.0:
        return None
    return [g[f"keep{s}/{i}"] for i in range(tn.N_FIXED + 3 * meta(g)[4])]


def tis_opt_state(case, g, step):
    opt = str(g["optimizer"])
    st = tn.new_opt_state(tis_params(case, g, 0), opt)
    st["step"] = step
    if step > 0:
        for name in STATE_NAMES[opt]:
            st[name] = tis_params(case, g, step, STATE_TAGS[name])
    return st


def exact_grads(w, batch, H, l2, keep, p):
    """``(loss64, g64, floor)``: the fp64 evaluation and the scale floor of ``K_w.bias`` (see the module docstring)."""
    with float64_oracle(tn):
        loss, g64, cache = tn.tisasrec_grads(to64(w), batch, H, l2, keep, p, with_cache=True)
    return loss, g64, te.key_bias_floor(cache)


def tis_band(w_prev, st_prev, g_ref, opt, lr, floor, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel of its scale of g_ref (``floor``: the scale
    floor of ``exact_grads`` -- Adam / RMSprop normalise K_w.bias's gradient, which is rounding noise around an exact
    zero, into updates of size lr whose sign no implementation shares with another)."""
    outs = []
    for sign in (+1.0, -1.0):
        w, st = {k: v.copy() for k, v in w_prev.items()}, copy_state(st_prev)
        gp = {k: (g_ref[k] + np.float32(sign * rel * max(float(np.abs(g_ref[k]).max()), floor(k)))).astype(np.float32)
              for k in w}
        tn.opt_step(w, gp, st, opt, lr)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in w_prev}


def unused_rows(tm, span):
    return sorted(set(range(span + 1)) - set(np.unique(tm).tolist()))


@pytest.mark.parametrize("case", CASES)
def test_numpy_restatement_matches_reference(case):
    """Every step in isolation from the reference's own weights and optimizer state: the loss, every gradient (in fp32
    as accurate as the reference against the fp64 evaluation), the time-table rows no pair selects exactly zero (in the
    reference's gradient too), the new weights."""
    g = load_golden(case)
    opt, lr, l2, p = hyper(g)
    H, span = meta(g)[3], meta(g)[8]
    for s in range(meta(g)[6]):
        w, st = tis_params(case, g, s), tis_opt_state(case, g, s)
        batch, keep = tis_batch(g, s), tis_keep(g, s)
        loss, grads = tn.tisasrec_grads(w, batch, H, l2, keep, p)
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        g_ref = tis_params(case, g, s + 1, "g")
        loss64, g64, floor = exact_grads(w, batch, H, l2, keep, p)
        assert_scalar_close(loss64, g["losses"][s], what=f"fp64 loss step {s}")
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}", floor_fn=floor)
        assert float(np.abs(grads["item_emb.weight"][0]).max()) == 0.0
        rows = unused_rows(batch[1], span)
        assert rows
        for k in ("time_matrix_K_emb.weight", "time_matrix_V_emb.weight"):
            assert float(np.abs(grads[k][rows]).max()) == 0.0 == float(np.abs(g_ref[k][rows]).max())
        band = tis_band(w, st, g_ref, opt, lr, floor)
        w_prev = {k: v.copy() for k, v in w.items()}
        tn.opt_step(w, grads, st, opt, lr)
        w_ref = tis_params(case, g, s + 1)
        for k in w:
            assert_step_close(w_prev[k], w[k], w_ref[k], band[k], what=f"weights {k} step {s}")


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_within_the_reference_own_error(case):
    """The fp64 evaluation against the reference's fp32 gradients: their distance is the reference's own rounding,
    at most REL of each tensor's scale (of its terms' scale for K_w.bias)."""
    g = load_golden(case)
    _, _, l2, p = hyper(g)
    worst = 0.0
    for s in range(meta(g)[6]):
        _, g64, floor = exact_grads(tis_params(case, g, s), tis_batch(g, s), meta(g)[3], l2, tis_keep(g, s), p)
        g_ref = tis_params(case, g, s + 1, "g")
        for k in g_ref:
            worst = max(worst, float(np.abs(g_ref[k] - g64[k]).max() / max(np.abs(g64[k]).max(), floor(k))))
    print(f"{case}: the reference's gradients are within {worst:.2e} of their scale of the exact ones")
    assert worst <= REL


@pytest.mark.parametrize("case", CASES)
def test_fixtures_hold_what_the_kernels_can_get_wrong(case):
    g = load_golden(case)
    I, T, D, H, nb, B, steps, _, span = meta(g)
    _, _, l2, p = hyper(g)
    for s in range(steps):
        seq, tm, pos, neg = tis_batch(g, s)
        real = (seq != 0).sum(1)
        assert (real == T).any() and (real == 1).any() and ((T - real) * 2 >= T).any()
        assert ((seq == 0) & (pos != 0)).any()
        assert set(seq.ravel().tolist()) & set(pos.ravel().tolist()) & set(neg.ravel().tolist()) - {0}
        assert tm.dtype == np.int32 and tm.shape == (B, T, T)
        assert tm.min() == 0 and tm.max() == span and unused_rows(tm, span)
        assert np.array_equal(tm, np.stack([tn.time_relation(t, span) for t in g["time_seq"][s]]))
        with float64_oracle(tn):
            _, _, cache = tn.tisasrec_grads(to64(tis_params(case, g, s)), (seq, tm, pos, neg), H, l2, tis_keep(g, s), p,
                                            with_cache=True)
        for c in cache["blocks"]:
            assert np.abs(c["pre1"]).min() >= 1e-4 * np.abs(c["pre1"]).max()
            assert 0.25 <= (c["pre1"] <= 0).mean() <= 0.75
    w0 = tis_params(case, g, 0)
    assert all(float(np.abs(w0[k]).max()) > 0 for k in w0 if k.endswith("bias") or k.endswith("emb.weight"))
    if p > 0:
        assert g["replay_ok"].all()        # what "torch_cpu" is documented to do rests on this
        assert len(tis_keep(g, 0)) == 5 + 3 * nb
        assert [k.size for k in tis_keep(g, 0)] == [int(np.prod(s)) for s in te.mask_shapes(D, H, T, B, nb)]


def test_padded_query_rows_are_uniform_in_the_restatement():
    """A padded query row attends uniformly over ALL positions, future ones included -- and nothing reads its output:
    zeroing those rows of the probabilities changes neither the features nor any gradient."""
    case = "tisasrec_adam"
    g = load_golden(case)
    I, T, D, H, nb, B, _, _, span = meta(g)
    w, batch = tis_params(case, g, 0), tis_batch(g, 0)
    with float64_oracle(tn):
        feats, cache = tn.tisasrec_forward(to64(w), batch[0], batch[1], H)
    pad = batch[0] == 0
    assert pad.any()
    for c in cache["blocks"]:
        rows = c["prob"][np.broadcast_to(pad[:, None, :], (B, H, T))]
        assert np.array_equal(rows, np.full(rows.shape, 1.0 / T))
        assert float(np.abs(c["o"][pad]).max()) > 0          # the reference does compute something there


def model_config(I, D, H, T, nb, span, p=0.0, B=8, l2=0.0, optimizer="adam", lr=1e-3, device="cpu"):
    return {"model": {"n_users": 64, "n_items": I, "emb_dim": D, "maxlen": T, "time_span": span, "num_blocks": nb,
                      "num_heads": H, "dropout_rate": p, "batch_size": B, "l2_emb": l2, "optimizer": optimizer, "lr": lr,
                      "device_str": device},
            "system": {"run_dir": "/tmp/hiprec_test_runs"}}


def build_engine(cfg):
    import beta_recsys_amd as hp

    with contextlib.redirect_stdout(io.StringIO()):
        return hp.TiSASRecEngine(cfg)


def test_constructor_weights_for_a_torch_seed():
    """Seed 2020: the mirror's state dict equals the reference's key for key (``_spec`` order is the golden
    ``state_dict`` order), shape for shape and bit for bit."""
    g = load_golden("tisasrec_init")
    I, T, D, H, nb, seed, span = (int(x) for x in g["meta"])
    torch.manual_seed(seed)
    eng = build_engine(model_config(I, D, H, T, nb, span, p=0.2))
    sd = eng.model.state_dict()
    assert tuple(sd) == tn.keys(nb) == tuple(n for n, _ in eng.model.named_parameters())
    assert tuple(sd) == tuple(k[2:] for k in g if k.startswith("w/")) == tuple(n for n, _ in eng.model._spec)
    for k, v in sd.items():
        assert tuple(v.shape) == g[f"w/{k}"].shape == tn.shapes(I, T, span, D, nb)[k], k
        assert np.array_equal(v.numpy(), g[f"w/{k}"]), k
    assert float(sd["item_emb.weight"][0].abs().max()) == 0.0
    assert eng.num_batch == 64 // 8 and eng.optimizer.name == "adam"
    for case in CASES:
        gc = load_golden(case)
        assert tuple(k[3:] for k in gc if k.startswith("w0/")) == tn.keys(meta(gc)[4])


def test_state_dict_round_trip(tmp_path):
    I, T, D, H, nb, span = 30, 10, 64, 2, 2, 12
    eng = build_engine(model_config(I, D, H, T, nb, span))
    path = str(tmp_path / "tisasrec.pt")
    eng.save_checkpoint(path)
    sd = torch.load(path)
    want = tn.shapes(I, T, span, D, nb)
    assert tuple(sd) == tn.keys(nb)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert sd["attention_layers.1.K_w.weight"].shape == (D, D) and sd["time_matrix_V_emb.weight"].shape == (span + 1, D)
    other = build_engine(model_config(I, D, H, T, nb, span))
    with contextlib.redirect_stdout(io.StringIO()):
        other.resume_checkpoint(path)
    assert torch.equal(other.model.flat, eng.model.flat)


def test_plumbing_and_limits():
    import ctypes

    import __graft_entry__ as ge
    from beta_recsys_amd import _lib, compat

    assert compat.MIRRORS["beta_rec.models.tisasrec"] == "tisasrec"
    assert ge.EVIDENCE_GROUPS["tisasrec"] == ge._EVIDENCE_COMMON + ["tisasrec.hip", "seqrec.hip", "seqrec.hpp",
                                                                    "ncf.hip", "gemm.hpp"]
    assert ge.evidence_group("tisasrec_step") == "tisasrec" and ge.evidence_group("sasrec_step") == "sasrec"
    for bad, word in ((dict(D=48, H=2), "head width"), (dict(D=256, H=4), "emb_dim"), (dict(D=64, H=2, T=300), "maxlen"),
                      (dict(span=257), "time_span")):
        kw = dict(I=20, D=64, H=2, T=10, nb=1, span=8)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            build_engine(model_config(**kw))
    lib = _lib.load()
    shape = _lib.TisasrecShape(20, 64, 2, 10, 8, 2, 0)
    assert lib.hiprec_tisasrec_shape_bytes() == ctypes.sizeof(_lib.TisasrecShape)
    eng = build_engine(model_config(20, 64, 2, 10, 2, 8))
    assert lib.hiprec_tisasrec_param_floats(ctypes.byref(shape)) == eng.model.flat.numel()
    assert lib.hiprec_tisasrec_workspace_bytes(ctypes.byref(shape), 4, 10) > 4 * 2 * 9 * 40 * 64
    for bad, word in ((_lib.TisasrecShape(20, 48, 2, 10, 8, 1, 0), b"head width"),
                      (_lib.TisasrecShape(20, 64, 2, 10, 257, 1, 0), b"time_span"),
                      (_lib.TisasrecShape(20, 64, 2, 257, 8, 1, 0), b"maxlen")):
        assert lib.hiprec_tisasrec_param_floats(ctypes.byref(bad)) == -1
        assert word in lib.hiprec_last_error()
        assert lib.hiprec_tisasrec_workspace_bytes(ctypes.byref(bad), 4, 10) == 0
    rc = lib.hiprec_tisasrec_grad(ctypes.byref(shape), None, None, None, None, None, None, 4, 10, 0.0, None, 1.0, None,
                                  None, None, 0, None, 0, None)
    assert rc == -1
    with pytest.raises(RuntimeError):                                                               # no CPU path
        eng.train_single_batch((np.zeros(2), np.ones((2, 10)), np.ones((2, 10)), None, np.ones((2, 10)), np.ones((2, 10))))


def test_workspace_holds_no_gathered_tensor():
    """At the reference's default shape (dim 64, 2 heads, 2 blocks, maxlen 150, time_span 128, batch 128) the whole
    workspace is smaller than ONE gathered [B, T, T, D] fp32 tensor, of which the reference keeps several."""
    import ctypes

    from beta_recsys_amd import _lib

    B, T, D = 128, 150, 64
    shape = _lib.TisasrecShape(3416, D, 2, T, 128, 2, 0)
    need = _lib.load().hiprec_tisasrec_workspace_bytes(ctypes.byref(shape), B, T)
    print(f"workspace {need / 2 ** 20:.0f} MiB, one gathered tensor {B * T * T * D * 4 / 2 ** 20:.0f} MiB")
    assert 0 < need < B * T * T * D * 4


def test_time_relation_equals_the_double_loop():
    from beta_recsys_amd.data import time_relation

    rng = np.random.default_rng(5)
    for span in (1, 7, 256):
        ts = rng.integers(0, 3 * span + 2, (4, 13))
        ts[1, :5] = 0
        got = time_relation(ts, span)
        assert got.dtype == np.int32 and got.shape == (4, 13, 13)
        for b in range(4):
            assert np.array_equal(got[b], tn.time_relation(ts[b], span))
            assert np.array_equal(time_relation(ts[b], span), got[b])
        assert got.max() == span and got.min() == 0


def test_time_sequence_sampler():
    from beta_recsys_amd.data import TimeSequenceSampler, time_relation

    rng = np.random.default_rng(3)
    n_items, T, B, span = 50, 8, 16, 6
    user_train = {}
    for u, n in enumerate([1, 2, 3, 8, 9, 20, 30, 5, 12]):
        items = (rng.permutation(n_items)[:n] + 1).tolist()
        times = (1 + np.cumsum(rng.integers(0, 4, n))).tolist()
        user_train[u] = [[i, t] for i, t in zip(items, times)]
    s = TimeSequenceSampler(user_train, len(user_train), n_items, B, T, span, seed=7)
    again = TimeSequenceSampler(user_train, len(user_train), n_items, B, T, span, seed=7)
    seen_users = set()
    for _ in range(20):
        batch = s.next_batch()
        assert len(batch) == 6
        for a, b in zip(batch, again.next_batch()):
            assert np.array_equal(a, b)
        users, seq, time_seq, tm, pos, neg = batch
        assert users.shape == (B,) and seq.shape == pos.shape == neg.shape == time_seq.shape == (B, T)
        assert seq.dtype == np.int64 and tm.shape == (B, T, T) and tm.dtype == np.int32
        assert np.array_equal(tm, time_relation(time_seq, span)) and tm.max() <= span
        for b, u in enumerate(users):
            items = [p[0] for p in user_train[int(u)]]
            times = [p[1] for p in user_train[int(u)]]
            assert len(items) >= 2
            n = min(T, len(items) - 1)
            for a in (seq, pos, neg, time_seq):
                assert (a[b, :T - n] == 0).all()
            assert seq[b, T - n:].tolist() == items[-n - 1:-1]
            assert time_seq[b, T - n:].tolist() == times[-n - 1:-1]
            assert pos[b, T - n:].tolist() == items[-n:]
            assert (neg[b, T - n:] >= 1).all() and (neg[b, T - n:] <= n_items).all()
            assert not set(neg[b, T - n:].tolist()) & set(items)
            assert np.array_equal(tm[b], tn.time_relation(time_seq[b], span))
            seen_users.add(int(u))
    assert 0 not in seen_users and seen_users == set(range(1, len(user_train)))
    s.close()
    with pytest.raises(ValueError):
        TimeSequenceSampler({0: [[1, 1]]}, 1, 5, 2, 4, 3)
    with pytest.raises(ValueError):
        TimeSequenceSampler({0: [[1, 1], [2]]}, 1, 5, 2, 4, 3)


@pytest.mark.parametrize("D,H,T,B,nb,span,p", te.EDGE_SHAPES)
def test_edge_fixture_layout(D, H, T, B, nb, span, p):
    """Sequence 0 is full length, the last one all padding, the others left-padded; the matrix holds 0 and the clamp;
    every mask drops and keeps."""
    w, (seq, tm, pos, neg), keep = te.edge_fixture(D, H, T, B, nb, span, p)
    assert (seq[0] != 0).all() and (pos[0] != 0).all()
    assert not seq[B - 1].any() and not pos[B - 1].any()
    real = seq != 0
    assert (real[:, 1:] >= real[:, :-1]).all(), "padding is on the left"
    if B > 2:
        assert 0 < real[1].sum() < T
    assert tm.min() == 0 and tm.max() == span and tm.dtype == np.int32
    assert [k.shape for k in keep] == te.mask_shapes(D, H, T, B, nb) and len(keep) == 5 + 3 * nb
    for k in keep:
        assert k.dtype == np.uint8 and abs(float(k.mean()) - (1 - p)) < 0.05
    assert float(np.abs(w["item_emb.weight"][0]).max()) == 0.0


@pytest.mark.parametrize("D,H,T,B,nb,span,p", te.VISIBLE_SHAPES)
def test_one_flipped_time_mask_byte_is_visible(D, H, T, B, nb, span, p):
    """The edge inputs used on the GPU can see ONE misplaced byte of the time-K mask and of the time-V mask: on the fp64
    restatement, flipping a single byte at every seam position of the attention tiles (sequence 0, the last head's first
    column) moves some gradient by MIN_MARGIN x what the GPU test's gradient bound allows."""
    w, batch, keep = te.edge_fixture(D, H, T, B, nb, span, p)
    _, g64, g32, floor = te.reference(w, batch, H, te.L2, keep, p)
    tol = te.tolerances(g32, g64, floor)
    keep = [k.reshape(s) for k, s in zip(keep, te.mask_shapes(D, H, T, B, nb))]
    col = (H - 1) * (D // H)
    margins = {}
    for i, j in te.seam_positions(T):
        for name, mask in (("time-K", 3), ("time-V", 4)):
            margins[name, i, j] = te.flip_margin(w, batch, H, te.L2, keep, p, g64, tol, mask, (0, i, j, col))
    for (name, i, j), m in margins.items():
        print(f"D {D} H {H} T {T}: {name} byte ({i}, {j}) moves a gradient by {m:.1f} x its tolerance")
    blind = {k: round(m, 2) for k, m in margins.items() if m < MIN_MARGIN}
    assert not blind, f"the gradient bound cannot see these bytes at {MIN_MARGIN:g} x: {blind}"
