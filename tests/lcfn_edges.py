"""Edge fixtures of the LCFN kernels (csrc/lcfn.hip): the smallest shapes at which each path can go wrong, held to the
fp64 restatement (tests/lcfn_numpy.py) with the fp32 restatement on the CPU standing in for "the reference's own error".

The seams come from what the library exports, not from copied numbers: the project / expand row tile
(``hiprec_lcfn_tile_rows``), the slot cap (``hiprec_lcfn_max_slots``; ``project_slots`` lowers it so that a table of a few
tiles already takes several rounds per slot), the loss stage's triples per block, and the MFMA granules of the kernels
(4 along the reduction, 16 along a tile edge: ``lcfn_numpy.TILE``).

A case: name -> dict(U, I, Fu, Fi, D, L, B, and optionally slots, batch="same" | None, zero_tables, zero_column,
train_filters).
"""
import numpy as np

import lcfn_numpy as lx
from helpers import REL, assert_as_accurate_as_reference, assert_scalar_close, float64_oracle, to64

LAMDA = 0.02


def seams():
    from beta_recsys_amd import _lib

    lib = _lib.load()
    return {"tile": int(lib.hiprec_lcfn_tile_rows()), "max_slots": int(lib.hiprec_lcfn_max_slots()),
            "triples": int(lib.hiprec_lcfn_loss_triples_per_block()), "max_dim": _lib.LCFN_MAX_DIM,
            "max_freq": _lib.LCFN_MAX_FREQ, "max_width": _lib.LCFN_MAX_WIDTH, "max_layers": _lib.LCFN_MAX_LAYERS}


def cases():
    s = seams()
    T, K = s["tile"], s["triples"]
    top = s["max_width"] // s["max_dim"] - 1          # the deepest model at the widest table
    return {
        # F in {1, 3, 4, 5, 16, 17, 33, 256}, D in {1, 8, 15, 16, 33, 64, 128}, n around the row tile
        "f1_3_d1_below_tile_b1": dict(U=T - 1, I=T, Fu=1, Fi=3, D=1, L=1, B=1),
        "f4_5_d8_above_tile": dict(U=T + 1, I=2 * T + 5, Fu=4, Fi=5, D=8, L=2, B=K + 1),
        "f16_17_d15": dict(U=2 * T + 6, I=T + 13, Fu=16, Fi=17, D=15, L=1, B=2 * K + 1),
        "f33_max_d16": dict(U=9 * T + 12, I=9 * T + 2, Fu=33, Fi=s["max_freq"], D=16, L=1, B=K + 3),
        "d33_deepest": dict(U=T + 18, I=T + 8, Fu=5, Fi=3, D=33, L=s["max_layers"], B=K + 2),
        "d64_f17_l2": dict(U=3 * T + 4, I=3 * T - 6, Fu=17, Fi=4, D=64, L=2, B=3 * K + 1),
        "widest_table": dict(U=T + 8, I=T + 5, Fu=3, Fi=5, D=s["max_dim"], L=top, B=K + 1),
        # more than one round of partial slots: 6 and 4 tiles over 2 slots
        "slot_rounds": dict(U=5 * T + 3, I=3 * T + 1, Fu=5, Fi=4, D=8, L=1, B=K + 2, slots=2),
        "repeated_triple": dict(U=T + 1, I=T - 1, Fu=4, Fi=5, D=8, L=1, B=K + 2, batch="same"),
        "zero_tables": dict(U=T + 1, I=T - 1, Fu=4, Fi=5, D=8, L=1, B=K + 2, zero_tables=True),
        "zero_column": dict(U=T + 1, I=T - 1, Fu=4, Fi=5, D=8, L=2, B=K + 2, zero_column=True),
        "train_f4_5_d8": dict(U=T + 1, I=2 * T + 5, Fu=4, Fi=5, D=8, L=2, B=K + 1, train_filters=True),
        "train_d64_f17": dict(U=3 * T + 4, I=3 * T - 6, Fu=17, Fi=4, D=64, L=2, B=3 * K + 1, train_filters=True),
    }


def make_case(name):
    c = dict(cases()[name])
    rng = np.random.default_rng(sum(name.encode()))
    U, I, D, L, B = c["U"], c["I"], c["D"], c["L"], c["B"]
    # bases with columns of unit scale (as eigenvectors are), tables large enough that every layer matters
    P = (rng.normal(size=(U, c["Fu"])) / np.sqrt(U)).astype(np.float32)
    Q = (rng.normal(size=(I, c["Fi"])) / np.sqrt(I)).astype(np.float32)
    if c.get("zero_column"):
        P[:, -1] = 0
        Q[:, 0] = 0
    w = {lx.KEYS[0]: rng.normal(0, 0.5, (U, D)).astype(np.float32), lx.KEYS[1]: rng.normal(0, 0.5, (I, D)).astype(np.float32)}
    if c.get("zero_tables"):
        w = {k: np.zeros_like(v) for k, v in w.items()}
    for k in range(L):
        w[f"user_filters.{k}"] = rng.normal(1, 0.2, c["Fu"]).astype(np.float32)
        w[f"item_filters.{k}"] = rng.normal(1, 0.2, c["Fi"]).astype(np.float32)
        w[f"transformers.{k}"] = (np.eye(D) + rng.normal(0, 0.5 / np.sqrt(D), (D, D))).astype(np.float32) * np.float32(4.0)
    if c.get("batch") == "same":
        batch = tuple(np.full(B, v, dtype=np.int64) for v in (U - 1, I - 1, 0))
    else:
        batch = (rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B))
        batch[0][-1], batch[1][-1], batch[2][-1] = U - 1, I - 1, I - 1      # the last rows of the last tiles take part
    c.update(name=name, P=P, Q=Q, w=w, batch=batch, hp={"L": L, "lamda": LAMDA}, train_filters=bool(c.get("train_filters")))
    return c


def restated(case, defect=None, fp64=True):
    """``((bpr, reg), loss, grads)`` of the restatement in fp64 (or fp32)."""
    if not fp64:
        return lx.lcfn_grads(case["w"], (case["P"], case["Q"]), case["hp"], case["batch"], defect, case["train_filters"])
    with float64_oracle(lx):
        return lx.lcfn_grads(to64(case["w"]), (case["P"], case["Q"]), case["hp"], case["batch"], defect,
                             case["train_filters"])


def check_step(case, loss, parts, grads, what=""):
    """Loss and both parts at REL of the fp64 value; every gradient within REL of the scale of the fp64 gradient plus
    twice the fp32 restatement's own distance from it; nothing NaN."""
    parts64, loss64, g64 = restated(case)
    _, _, g32 = restated(case, fp64=False)
    print(f"{what}: loss {loss!r} vs {loss64!r}; parts {parts} vs {parts64}")
    assert_scalar_close(loss, loss64, what=f"{what} loss")
    for got, ref, name in zip(parts, parts64, ("bpr", "reg")):
        assert_scalar_close(got, ref, what=f"{what} {name}")
    keys = lx.all_keys(case["L"]) if case["train_filters"] else lx.KEYS
    for k in keys:
        got = np.asarray(grads[k].cpu().numpy() if hasattr(grads[k], "cpu") else grads[k])
        assert np.isfinite(got).all(), f"{what} grad {k} is not finite"
        err, own = np.abs(got.reshape(g64[k].shape) - g64[k]).max(), np.abs(g32[k] - g64[k]).max()
        print(f"  grad {k}: err vs fp64 {err:.3e} (fp32 restatement's {own:.3e}) of scale {np.abs(g64[k]).max():.3e}")
        assert_as_accurate_as_reference(got.reshape(g64[k].shape), g32[k], g64[k], REL, f"{what} grad {k}")
    return g64
