"""Pin tests/sasrec_numpy.py against golden vectors captured from the real reference's SASRecEngine by
``tools/gen_golden_sasrec.py``, and the host-side parts of the SASRec mirror.  CPU only."""
import contextlib
import io

import numpy as np
import pytest
import torch

import sasrec_numpy as sn
from helpers import REL, assert_grads_as_accurate, assert_scalar_close, assert_step_close
from helpers import copy_state, float64_oracle, load_golden, to64

CASES = ["sasrec_adam", "sasrec_sgd_h1", "sasrec_rmsprop_drop"]
STATE_NAMES = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg",), "sgd": ()}
STATE_TAGS = {"exp_avg": "m", "exp_avg_sq": "v", "square_avg": "v"}


def meta(g):
    """(I, T, D, H, blocks, B, steps, seed)"""
    return tuple(int(x) for x in g["meta"])


def hyper(g):
    """(optimizer, lr, l2_emb, dropout rate)"""
    return str(g["optimizer"]), float(g["lr"]), float(g["l2_emb"]), float(g["dropout_rate"])


def sas_keys(g):
    return sn.keys(meta(g)[4])


def sas_params(case, g, step, tag="w"):
    """Tensor set ``tag`` (w / g / m / v) of the reference after ``step`` steps (w after 0 steps: the initial weights)."""
    if step == 0 and tag == "w":
        return {k: g[f"w0/{k}"].astype(np.float32).copy() for k in sas_keys(g)}
    s = load_golden(f"{case}_s{step}")
    return {k: s[f"{tag}/{k}"].astype(np.float32).copy() for k in sas_keys(g)}


def sas_batch(g, s):
    return g["seq"][s], g["pos"][s], g["neg"][s]


def sas_keep(g, s):
    if float(g["dropout_rate"]) == 0.0:
        return None
    return [g[f"keep{s}/{i}"] for i in range(1 + 3 * meta(g)[4])]


def sas_opt_state(case, g, step):
    opt = str(g["optimizer"])
    st = sn.new_opt_state(sas_params(case, g, 0), opt)
    st["step"] = step
    if step > 0:
        for name in STATE_NAMES[opt]:
            st[name] = sas_params(case, g, step, STATE_TAGS[name])
    return st


def exact_grads(w, batch, H, l2, keep, p):
    with float64_oracle(sn):
        return sn.sasrec_grads(to64(w), batch, H, l2, keep, p)


def sas_band(w_prev, st_prev, g_ref, opt, lr, rel=REL):
    """Forward-error band of one optimizer step for a gradient within rel of its scale of g_ref
    (helpers.optimizer_band's rule on this model's keys)."""
    outs = []
    for sign in (+1.0, -1.0):
        w, st = {k: v.copy() for k, v in w_prev.items()}, copy_state(st_prev)
        gp = {k: (g_ref[k] + np.float32(sign * rel * float(np.abs(g_ref[k]).max()))).astype(np.float32) for k in w}
        sn.opt_step(w, gp, st, opt, lr)
        outs.append(w)
    return {k: np.abs(outs[0][k].astype(np.float64) - outs[1][k].astype(np.float64)) for k in w_prev}


@pytest.mark.parametrize("case", CASES)
def test_numpy_restatement_matches_reference(case):
    """Every step in isolation from the reference's own weights and optimizer state: the loss, every gradient (in fp32
    as accurate as the reference against the fp64 evaluation), the new weights."""
    g = load_golden(case)
    opt, lr, l2, p = hyper(g)
    H = meta(g)[3]
    for s in range(meta(g)[6]):
        w, st = sas_params(case, g, s), sas_opt_state(case, g, s)
        batch, keep = sas_batch(g, s), sas_keep(g, s)
        loss, grads = sn.sasrec_grads(w, batch, H, l2, keep, p)
        assert_scalar_close(loss, g["losses"][s], what=f"loss step {s}")
        g_ref = sas_params(case, g, s + 1, "g")
        loss64, g64 = exact_grads(w, batch, H, l2, keep, p)
        assert_scalar_close(loss64, g["losses"][s], what=f"fp64 loss step {s}")
        assert_grads_as_accurate(grads, g_ref, g64, what=f"grad step {s}")
        assert float(np.abs(grads["item_emb.weight"][0]).max()) == 0.0
        band = sas_band(w, st, g_ref, opt, lr)
        w_prev = {k: v.copy() for k, v in w.items()}
        sn.opt_step(w, grads, st, opt, lr)
        w_ref = sas_params(case, g, s + 1)
        for k in w:
            assert_step_close(w_prev[k], w[k], w_ref[k], band[k], what=f"weights {k} step {s}")


@pytest.mark.parametrize("case", CASES)
def test_fp64_restatement_within_the_reference_own_error(case):
    """The fp64 evaluation against the reference's fp32 gradients: their distance is the reference's own rounding,
    at most REL of each tensor's scale."""
    g = load_golden(case)
    _, _, l2, p = hyper(g)
    worst = 0.0
    for s in range(meta(g)[6]):
        _, g64 = exact_grads(sas_params(case, g, s), sas_batch(g, s), meta(g)[3], l2, sas_keep(g, s), p)
        g_ref = sas_params(case, g, s + 1, "g")
        for k in g_ref:
            worst = max(worst, float(np.abs(g_ref[k] - g64[k]).max() / np.abs(g64[k]).max()))
    print(f"{case}: the reference's gradients are within {worst:.2e} of their scale of the exact ones")
    assert worst <= REL


@pytest.mark.parametrize("case", CASES)
def test_fixtures_hold_what_the_kernels_can_get_wrong(case):
    g = load_golden(case)
    I, T, D, H, nb, B, steps, _ = meta(g)
    _, _, l2, p = hyper(g)
    for s in range(steps):
        seq, pos, neg = sas_batch(g, s)
        real = (seq != 0).sum(1)
        assert (real == T).any() and (real == 1).any() and ((T - real) * 2 >= T).any()
        assert ((seq == 0) & (pos != 0)).any()
        assert set(seq.ravel().tolist()) & set(pos.ravel().tolist()) & set(neg.ravel().tolist()) - {0}
        with float64_oracle(sn):
            _, _, cache = sn.sasrec_grads(to64(sas_params(case, g, s)), (seq, pos, neg), H, l2, sas_keep(g, s), p,
                                          with_cache=True)
        for c in cache["blocks"]:
            assert np.abs(c["pre1"]).min() >= 1e-4 * np.abs(c["pre1"]).max()
            assert 0.25 <= (c["pre1"] <= 0).mean() <= 0.75
    w0 = sas_params(case, g, 0)
    assert all(float(np.abs(w0[k]).max()) > 0 for k in w0 if k.endswith("bias"))
    if p > 0:
        assert g["replay_ok"].all()        # what "torch_cpu" is documented to do rests on this


def test_padded_keys_are_attended_to_in_the_restatement():
    """S3: no key-padding mask.  A bias on the keys shifts every score of a row alike and cancels in the softmax, so the
    padded keys show in the WEIGHT they take from the real ones: against the counterfactual with a key-padding mask the
    loss of a left-padded batch moves, that of fully real sequences does not."""
    g = load_golden("sasrec_adam")
    I, T, D, H, nb, B, _, _ = meta(g)
    w = sas_params("sasrec_adam", g, 0)
    batch = sas_batch(g, 0)
    base = sn.sasrec_loss(w, batch, H, 0.0)
    assert abs(sn.sasrec_loss(w, batch, H, 0.0, mask_padded_keys=True) - base) > 1e-3 * abs(base)
    full = tuple(a[:1] for a in batch)                       # row 0 is fully real
    assert (full[0] != 0).all()
    assert sn.sasrec_loss(w, full, H, 0.0, mask_padded_keys=True) == sn.sasrec_loss(w, full, H, 0.0)
    w2 = {k: v.copy() for k, v in w.items()}
    w2["attention_layers.0.in_proj_bias"][D:2 * D] += 0.5
    assert_scalar_close(sn.sasrec_loss(w2, batch, H, 0.0), base, what="a key bias cancels in the softmax")


def model_config(I, D, H, T, nb, p=0.0, B=8, l2=0.0, optimizer="adam", lr=1e-3, device="cpu"):
    return {"model": {"n_users": 64, "n_items": I, "emb_dim": D, "maxlen": T, "num_blocks": nb, "num_heads": H,
                      "dropout_rate": p, "batch_size": B, "l2_emb": l2, "optimizer": optimizer, "lr": lr,
                      "device_str": device},
            "system": {"run_dir": "/tmp/hiprec_test_runs"}}


def build_engine(cfg):
    import beta_recsys_amd as hp

    with contextlib.redirect_stdout(io.StringIO()):
        return hp.SASRecEngine(cfg)


def test_constructor_weights_for_a_torch_seed():
    """Seed 2020: the mirror's state dict equals the reference's key for key, shape for shape and bit for bit."""
    g = load_golden("sasrec_init")
    I, T, D, H, nb, seed = (int(x) for x in g["meta"])
    torch.manual_seed(seed)
    eng = build_engine(model_config(I, D, H, T, nb, p=0.2))
    sd = eng.model.state_dict()
    assert tuple(sd) == sn.keys(nb) == tuple(n for n, _ in eng.model.named_parameters())
    assert tuple(sd) == tuple(k[2:] for k in g if k.startswith("w/"))
    for k, v in sd.items():
        assert tuple(v.shape) == g[f"w/{k}"].shape == sn.shapes(I, T, D, nb)[k], k
        assert np.array_equal(v.numpy(), g[f"w/{k}"]), k
    assert float(sd["item_emb.weight"][0].abs().max()) == 0.0
    assert eng.num_batch == 64 // 8 and eng.optimizer.name == "adam"


def test_state_dict_round_trip(tmp_path):
    """What save_checkpoint writes is a plain state dict with the reference's keys and shapes, and loads back."""
    I, T, D, H, nb = 30, 10, 64, 2, 2
    eng = build_engine(model_config(I, D, H, T, nb))
    path = str(tmp_path / "sasrec.pt")
    eng.save_checkpoint(path)
    sd = torch.load(path)
    want = sn.shapes(I, T, D, nb)
    assert tuple(sd) == sn.keys(nb)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert sd["forward_layers.1.conv2.weight"].shape == (D, D, 1)
    assert sd["attention_layers.0.in_proj_weight"].shape == (3 * D, D)
    other = build_engine(model_config(I, D, H, T, nb))
    with contextlib.redirect_stdout(io.StringIO()):
        other.resume_checkpoint(path)
    assert torch.equal(other.model.flat, eng.model.flat)
    # a reference-made dict (plain tensors under the same keys) loads too
    ref_like = {k: torch.full(s, 0.5) for k, s in want.items()}
    other.model.load_state_dict(ref_like)
    assert float(other.model.flat.min()) == 0.5 == float(other.model.flat.max())


def test_plumbing_and_limits():
    import ctypes

    import __graft_entry__ as ge
    from beta_recsys_amd import _lib, compat

    assert compat.MIRRORS["beta_rec.models.sasrec"] == "sasrec"
    assert ge.EVIDENCE_GROUPS["sasrec"] == ge._EVIDENCE_COMMON + ["sasrec.hip", "seqrec.hip", "seqrec.hpp",
                                                                  "ncf.hip", "gemm.hpp"]
    assert ge.evidence_group("sasrec_step") == "sasrec"
    for bad, word in ((dict(D=48, H=2), "head width"), (dict(D=256, H=4), "emb_dim"), (dict(D=64, H=2, T=300), "maxlen")):
        kw = dict(I=20, D=64, H=2, T=10, nb=1)
        kw.update(bad)
        with pytest.raises(ValueError, match=word):
            build_engine(model_config(**kw))
    lib = _lib.load()
    shape = _lib.SasrecShape(20, 64, 2, 10, 2)
    assert lib.hiprec_sasrec_shape_bytes() == ctypes.sizeof(_lib.SasrecShape)
    eng = build_engine(model_config(20, 64, 2, 10, 2))
    assert lib.hiprec_sasrec_param_floats(ctypes.byref(shape)) == eng.model.flat.numel()
    assert lib.hiprec_sasrec_workspace_bytes(ctypes.byref(shape), 4, 10) > 4 * 2 * 9 * 40 * 64
    assert lib.hiprec_sasrec_param_floats(ctypes.byref(_lib.SasrecShape(20, 48, 2, 10, 1))) == -1
    assert b"head width" in lib.hiprec_last_error()
    rc = lib.hiprec_sasrec_grad(ctypes.byref(shape), None, None, None, None, None, 4, 10, 0.0, None, 1.0, None, None,
                                None, 0, None, 0, None)
    assert rc == -1
    with pytest.raises(RuntimeError):
        eng.train_single_batch((np.zeros(2), np.ones((2, 10)), np.ones((2, 10)), np.ones((2, 10))))   # no CPU path


def test_sequence_sampler():
    from beta_recsys_amd.data import SequenceSampler

    rng = np.random.default_rng(3)
    n_items, T, B = 50, 8, 16
    user_train = {u: (rng.permutation(n_items)[:n] + 1).tolist() for u, n in enumerate([1, 2, 3, 8, 9, 20, 30, 5, 12])}
    s = SequenceSampler(user_train, len(user_train), n_items, B, T, seed=7)
    again = SequenceSampler(user_train, len(user_train), n_items, B, T, seed=7)
    seen_users = set()
    for _ in range(20):
        users, seq, pos, neg = s.next_batch()
        for a, b in zip((users, seq, pos, neg), again.next_batch()):
            assert np.array_equal(a, b)
        assert users.shape == (B,) and seq.shape == pos.shape == neg.shape == (B, T) and seq.dtype == np.int64
        for b, u in enumerate(users):
            items = user_train[int(u)]
            assert len(items) >= 2
            n = min(T, len(items) - 1)
            assert (seq[b, :T - n] == 0).all() and (pos[b, :T - n] == 0).all() and (neg[b, :T - n] == 0).all()
            assert seq[b, T - n:].tolist() == items[-n - 1:-1]
            assert pos[b, T - n:].tolist() == items[-n:]            # the item after seq at every real position
            assert (neg[b, T - n:] >= 1).all() and (neg[b, T - n:] <= n_items).all()
            assert not set(neg[b, T - n:].tolist()) & set(items)
            seen_users.add(int(u))
    assert 0 not in seen_users and seen_users == set(range(1, len(user_train)))
    s.close()
    with pytest.raises(ValueError):
        SequenceSampler({0: [1]}, 1, 5, 2, 4)
