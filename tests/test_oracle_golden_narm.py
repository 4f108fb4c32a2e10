"""Pin tests/narm_numpy.py against golden vectors captured from the real reference's NARMEngine by
``tools/gen_golden_narm.py``, and the host-side parts of the NARM mirror: the session loader, the constructor, the
registration, and the checks that a wrong implementation would be VISIBLE on the inputs the GPU tests use.  CPU only."""
import numpy as np
import pytest
import torch

import narm_edges as ne
import narm_numpy as nn_
from helpers import REL, assert_grads_as_accurate, assert_scalar_close, assert_step_close
from helpers import copy_state, float64_oracle, load_golden, to64

CASES = ["narm_adam", "narm_sgd_l2", "narm_rmsprop_drop"]
STATE_NAMES = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg",), "sgd": ()}
STATE_TAGS = {"exp_avg": "m", "exp_avg_sq": "v", "square_avg": "v"}
MIN_MARGIN = 2.0      # a wrong implementation must move some gradient by more than this many GPU-test bounds


def meta(g):
    """(I, T, D, H, layers, B, steps, seed)"""
    return tuple(int(x) for x in g["meta"])


def hyper(g):
    """(optimizer, lr, lr_dc_step, lr_dc, (dropout_input, dropout_hidden))"""
    return (str(g["optimizer"]), float(g["lr"]), int(g["lr_dc_step"]), float(g["lr_dc"]),
            (float(g["dropout_input"]), float(g["dropout_hidden"])))


def step_lr(g, s):
    _, lr, dc_step, dc, _ = hyper(g)
    return nn_.step_lr(lr, dc, dc_step, s)


def narm_params(case, g, step, tag="w"):
    """Tensor set ``tag`` (w / g / m / v) of the reference after ``step`` steps (w after 0 steps: the initial weights)."""
    keys = nn_.keys(meta(g)[4])
    if step == 0 and tag == "w":
        return {k: g[f"w0/{k}"].astype(np.float32).copy() for k in keys}
    s = load_golden(f"{case}_s{step}")
    return {k: s[f"{tag}/{k}"].astype(np.float32).copy() for k in keys}


def narm_batch(g, s):
    return g["seq"][s], g["target"][s], g["lens"][s]


def narm_keep(g, s):
    if not any(hyper(g)[4]):
        return None
    return [g[f"keep{s}/{i}"] for i in range(2)]


def narm_opt_state(case, g, step):
    opt = str(g["optimizer"])
    st = nn_.new_opt_state(narm_params(case, g, 0), opt)
    st["step"] = step
    if step > 0:
        for name in STATE_NAMES[opt]:
            st[name] = narm_params(case, g, step, STATE_TAGS[name])
    return st


def exact_grads(w, batch, keep, p, **variant):
    with float64_oracle(nn_):
        return nn_.narm_grads(to64(w), batch, keep, p, **variant)


def narm_band(w_prev, st_prev, g_ref, opt, lr, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel of its scale of g_ref
    (helpers.optimizer_band's rule on this model's keys)."""
    outs = []
    for sign in (+1.0, -1.0):
        w, st = {k: v.copy() for k, v in w_prev.items()}, copy_state(st_prev)
        gp = {k: (g_ref[k] + np.float32(sign * rel * float(np.abs(g_ref[k]).max()))).astype(np.float32) for k in w}
        nn_.opt_step(w, gp, st, opt, lr)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in w_prev}


def model_config(I, D, H, L, B, p=(0.0, 0.0), optimizer="adam", lr=1e-3, lr_dc_step=80, lr_dc=0.1, device="cpu"):
    return {"dataset": {"n_items": I},
            "model": {"hidden_size": H, "n_layers": L, "embedding_dim": D, "dropout_input": p[0], "dropout_hidden": p[1],
                      "batch_size": B, "optimizer": optimizer, "lr": lr, "lr_dc_step": lr_dc_step, "lr_dc": lr_dc,
                      "device_str": device},
            "system": {"run_dir": "/tmp/hiprec_narm_runs"}}


def golden_config(g, device="cpu"):
    I, T, D, H, L, B, _, _ = meta(g)
    opt, lr, dc_step, dc, p = hyper(g)
    return model_config(I, D, H, L, B, p, opt, lr, dc_step, dc, device)


@pytest.mark.parametrize("case", CASES)
def test_numpy_restatement_matches_reference(case):
    """Every step in isolation from the reference's own weights and optimizer state, at the epoch's learning rate: the
    loss, every gradient (in fp32 as accurate as the reference against the fp64 evaluation), the new weights."""
    g = load_golden(case)
    opt, _, _, _, p = hyper(g)
    for s in range(meta(g)[6]):
        w, st = narm_params(case, g, s), narm_opt_state(case, g, s)
        batch, keep = narm_batch(g, s), narm_keep(g, s)
        loss, grads = nn_.narm_grads(w, batch, keep, p)
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        g_ref = narm_params(case, g, s + 1, "g")
        loss64, g64 = exact_grads(w, batch, keep, p)
        assert_scalar_close(loss64, g["losses"][s], what=f"fp64 loss step {s}")
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}")
        assert float(np.abs(grads["emb.weight"][0]).max()) == 0.0
        assert float(np.abs(g_ref["emb.weight"][0]).max()) == 0.0
        lr = step_lr(g, s)
        assert lr == float(g["lrs"][s]) or abs(lr - float(g["lrs"][s])) <= 1e-12 * lr
        band = narm_band(w, st, g_ref, opt, lr)
        w_prev = {k: v.copy() for k, v in w.items()}
        nn_.opt_step(w, grads, st, opt, lr)
        w_ref = narm_params(case, g, s + 1)
        for k in w:
            assert_step_close(w_prev[k], w[k], w_ref[k], band[k], what=f"weights {k} step {s}")


def test_the_adam_fixture_pins_the_schedule():
    g = load_golden("narm_adam")
    assert [float(x) for x in g["lrs"]] == pytest.approx([1e-2, 1e-2, 1e-3], rel=1e-12)
    assert step_lr(g, 2) == pytest.approx(float(g["lr"]) / 10, rel=1e-12)


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_within_the_reference_own_error(case):
    g = load_golden(case)
    p = hyper(g)[4]
    worst = 0.0
    for s in range(meta(g)[6]):
        _, g64 = exact_grads(narm_params(case, g, s), narm_batch(g, s), narm_keep(g, s), p)
        g_ref = narm_params(case, g, s + 1, "g")
        for k in g_ref:
            worst = max(worst, float(np.abs(g_ref[k] - g64[k]).max() / np.abs(g64[k]).max()))
    print(f"{case}: the reference's gradients are within {worst:.2e} of their scale of the exact ones")
    assert worst <= REL


@pytest.mark.parametrize("case", CASES)
def test_fixtures_hold_what_the_kernels_can_get_wrong(case):
    g = load_golden(case)
    I, T, D, H, L, B, steps, _ = meta(g)
    for s in range(steps):
        seq, target, lens = narm_batch(g, s)
        assert seq.shape == (T, B) and (lens == T).any() and (lens == 1).any()
        assert any((seq[:lens[b], b] == 0).any() for b in range(B)), "no 0 inside a session's length"
        assert any((seq[:lens[b], b] == i).sum() >= 2 and sum(i in seq[:lens[c], c] for c in range(B)) >= 2
                   for b in range(B) for i in set(seq[:lens[b], b].tolist()) - {0})
        assert any(target[b] in seq[:lens[b], b] for b in range(B))
        assert len(set(target.tolist())) < B
        with float64_oracle(nn_):
            _, c = nn_.narm_forward(to64(narm_params(case, g, s)), seq, lens, narm_keep(g, s), hyper(g)[4])
        sg = c["s"][np.arange(T)[:, None] < lens[None, :]]
        assert float(np.abs(np.log(sg) - np.log1p(-sg)).max()) <= 6.0
    if any(hyper(g)[4]):
        assert g["replay_ok"].all()


# ---- the session loader ------------------------------------------------------------------------------------------------
def _ragged(flat, lens):
    return [a.tolist() for a in np.split(flat, np.cumsum(lens)[:-1])]


def test_session_prefixes_and_loader_are_the_reference_bit_for_bit():
    from beta_recsys_amd.data import SessionLoader, session_prefixes

    g = load_golden("narm_loader")
    sequences = _ragged(g["seq_flat"], g["seq_lens"])
    out_seqs, labels = session_prefixes(sequences)
    assert out_seqs == _ragged(g["out_flat"], g["out_lens"])
    assert labels == g["labels"].tolist()
    loader = SessionLoader(out_seqs, labels, int(g["batch_size"]))
    n = int(g["n_batches"])
    assert len(loader) == n and len(out_seqs) % int(g["batch_size"]) != 0
    for epoch in range(2):                                   # re-iterable: one loader serves every epoch
        batches = list(loader)
        assert len(batches) == n
        for k, (seq, target, lens) in enumerate(batches):
            assert seq.dtype == torch.int64 and target.dtype == torch.int64 and isinstance(lens, list)
            assert np.array_equal(seq.numpy(), g[f"b{k}/seq"]), f"batch {k} ids"
            assert np.array_equal(target.numpy(), g[f"b{k}/target"]), f"batch {k} labels"
            assert lens == g[f"b{k}/lens"].tolist()
    assert any(len(set(g[f"b{k}/lens"].tolist())) < len(g[f"b{k}/lens"]) for k in range(n)), "no ties in length"
    with pytest.raises(ValueError):
        SessionLoader(out_seqs, labels[:-1], 5)
    with pytest.raises(ValueError):
        SessionLoader([[1], []], [2, 3], 5)


# ---- constructor, registration -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_constructor_reproduces_the_reference_weights(case):
    """Same torch seed, same constructed weights (the fixture's ``winit``: before the tool's bias perturbation), same
    ``state_dict`` keys, shapes and order; checkpoints load in both directions."""
    import beta_recsys_amd as hp

    g = load_golden(case)
    torch.manual_seed(meta(g)[7])
    model = hp.NARM(golden_config(g))
    sd = model.state_dict()
    keys = nn_.keys(meta(g)[4])
    assert tuple(sd) == keys == tuple(n for n, _ in model.named_parameters())
    I, _, D, H, L = meta(g)[:5]
    for k, shape in nn_.shapes(I, D, H, L).items():
        assert tuple(sd[k].shape) == shape
        assert np.array_equal(sd[k].numpy(), g[f"winit/{k}"]), k
    model.load_state_dict({k: torch.from_numpy(g[f"w0/{k}"]) for k in keys})
    assert np.array_equal(model.flat.numpy(), np.concatenate([g[f"w0/{k}"].ravel() for k in keys]))
    ref_like = {k: torch.zeros(shape) for k, shape in nn_.shapes(I, D, H, L).items()}
    for k, v in model.state_dict().items():                  # the other direction: a reference module's load_state_dict
        ref_like[k].copy_(v)


def test_config_limits():
    import beta_recsys_amd as hp

    for bad in (dict(H=129), dict(D=129), dict(L=5), dict(L=0), dict(I=1)):
        kw = dict(I=10, D=8, H=8, L=1, B=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            hp.NARM(model_config(**kw))
    with pytest.raises(ValueError):
        hp.NARM(model_config(10, 8, 8, 1, 2, p=(1.0, 0.0)))
    hp.NARM(model_config(10, 100, 100, 4, 2))


def test_registration():
    import __graft_entry__ as ge
    from beta_recsys_amd import compat

    assert compat.MIRRORS["beta_rec.models.narm"] == "narm"
    assert ge.EVIDENCE_GROUPS["narm"] == ge._EVIDENCE_COMMON + ["narm.hip", "seqrec.hip", "seqrec.hpp", "ncf.hip",
                                                                "gemm.hpp"]
    assert ge.evidence_group("narm_step") == "narm"


# ---- visibility: a wrong implementation must show on the inputs the GPU tests use ---------------------------------------
def _inputs():
    """(name, weights, batch, keep, p, reference fp32 gradients) of every fixture step and every edge shape."""
    for case in CASES:
        g = load_golden(case)
        for s in range(meta(g)[6]):
            yield (f"{case} step {s}", narm_params(case, g, s), narm_batch(g, s), narm_keep(g, s), hyper(g)[4],
                   narm_params(case, g, s + 1, "g"))
    for shape in ne.SHAPES:
        w, batch, keep = ne.synthetic(shape)
        yield ne.shape_id(shape), w, batch, keep, shape[6], nn_.narm_grads(w, batch, keep, shape[6])[1]


def _margin(g_wrong, g_ref, g64):
    """Largest distance of a wrong gradient from the exact one, in units of the GPU tests' bound for that tensor."""
    return max(float(np.abs(g_wrong[k] - g64[k]).max() /
                     (REL * np.abs(g64[k]).max() + 2.0 * np.abs(g_ref[k] - g64[k]).max() + 1e-300)) for k in g64)


def test_wrong_last_state_and_wrong_mask_are_visible():
    """``h_T`` taken at ``T - 1`` instead of ``lens - 1`` (visible wherever a session is shorter than T), and the mask
    taken from ``lens`` instead of ``seq > 0`` (visible wherever a 0 sits inside a length)."""
    seen_short = seen_zero = 0
    for name, w, batch, keep, p, g_ref in _inputs():
        seq, _, lens = batch
        T, B = seq.shape
        _, g64 = exact_grads(w, batch, keep, p)
        if (np.asarray(lens) < T).any():
            seen_short += 1
            m = _margin(exact_grads(w, batch, keep, p, ht_at_last=True)[1], g_ref, g64)
            print(f"{name}: h_T at T - 1 moves a gradient by {m:.1f} bounds")
            assert m > MIN_MARGIN, name
        if any((seq[:lens[b], b] == 0).any() for b in range(B)):
            seen_zero += 1
            m = _margin(exact_grads(w, batch, keep, p, mask_from_lens=True)[1], g_ref, g64)
            print(f"{name}: the mask from lens moves a gradient by {m:.1f} bounds")
            assert m > MIN_MARGIN, name
    assert seen_short >= 9 + len(ne.SHAPES) - 1 and seen_zero >= 9 + 4


def test_one_flipped_keep_byte_is_visible():
    """The first and last element of each mask, and the first and last position inside a session's length.  Input-mask
    bytes at ``t >= lens[b]`` are never read: flipping one changes nothing, and they are the only bytes exempt."""
    checked = 0
    for name, w, batch, keep, p, g_ref in _inputs():
        if keep is None:
            continue
        seq, _, lens = batch
        T, B = seq.shape
        D, H = w["emb.weight"].shape[1], w["a_1.weight"].shape[0]
        _, g64 = exact_grads(w, batch, keep, p)
        b_short = int(np.argmax((np.asarray(lens) < T) & (np.asarray(lens) >= 2)))
        spots = [(0, 0), (0, T * B * D - 1), (1, 0), (1, B * 2 * H - 1),
                 (0, (0 * B + b_short) * D), (0, ((int(lens[b_short]) - 1) * B + b_short) * D + D - 1)]
        for i, e in spots:
            flipped = [k.copy() for k in keep]
            flipped[i][e] ^= 1
            _, g_f = exact_grads(w, batch, flipped, p)
            if i == 0:
                t, b = (e // D) // B, (e // D) % B
                if t >= lens[b]:
                    assert all(np.array_equal(g_f[k], g64[k]) for k in g64), f"{name}: a byte beyond a length was read"
                    continue
                if seq[t, b] == 0:
                    continue                                  # the padding row is zero: nothing to keep or drop
            m = _margin(g_f, g_ref, g64)
            print(f"{name}: mask {i} byte {e} moves a gradient by {m:.1f} bounds")
            assert m > MIN_MARGIN, f"{name} mask {i} byte {e}"
            checked += 1
    assert checked >= 4 * 4
