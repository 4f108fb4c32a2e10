"""Fixtures of the GRU4Rec tests, shared by tests/test_gru4rec_host.py (which shows on the CPU that they see every defect
of ``gru4rec_torch.DEFECTS`` and cover what this table claims) and the GPU tests (which run csrc/gru4rec.hip on those very
inputs).  No tests here.

| name               | what it is there for                                                                            |
|--------------------|-------------------------------------------------------------------------------------------------|
| tiny               | B 1, S 1, H 1: one slot, one negative, nothing to choose                                        |
| defaults           | B 7, S 5, layers [100], constrained, bpr-max with elu 0.5 and bpreg 1: 100 is ragged against    |
|                    | every 16, 32 and 64 tile; logq is set and must be IGNORED by bpr-max                            |
| limits             | layers [128, 128, 128], embedding 128, B 2, S 65: every width limit, N one candidate tile + 3   |
| stacked            | layers [5, 9, 3], embedding 6: three different widths, unconstrained                            |
| tile_edges_B_<B>   | B one under, at and one over the 4 rows of a loss workgroup, the 64 rows of a GEMM tile and the |
|                    | 128 rows of a column-sum slab (``TILE_BATCHES``), H 3                                           |
| tile_edges_N_<S>   | B 5 and S such that N is 63 / 64 / 65 (the GEMM's candidate tile and the loss wave's 64 lanes), |
|                    | and S 0 (in-batch negatives alone)                                                              |
| repeats            | one item as input of many slots, one as target of many, one twice among the samples, one sample |
|                    | equal to rows' own target: every row-atomic path must sum, and an equal id is still a negative  |
| resets_all/none/mixed | the reset byte against a non-zero stored state                                               |
| dropout            | both rates 0.5 with explicit masks, two layers                                                  |
| logq               | cross-entropy with logq 1 and sample_alpha 0.5                                                  |
| xe                 | cross-entropy without a shift, two layers, constrained                                          |
| elu_<a>_bpreg_<b>  | elu_param 0 / 0.5 / 1 crossed with bpreg 0 / 1                                                  |
| max_batch          | B 2048, S 4096, layers [128]: the batch limits (grid-stride loops, 16 column-sum slabs)         |

Weights are at unit scale (every pre-activation and every score is O(1), so no term vanishes); every fixture carries a
non-zero stored state, and ids are drawn from ``0 .. I - 4`` so that the last three rows of every table are named by no id.

Where ``elu_param`` is not 0 or 1 the ELU's derivative jumps at 0, so every ``|R|`` of such a fixture is further than
``MARGIN`` = 1e-3 of ``max |R|`` from 0 in float64; ``fixture`` moves to the next seed until that holds.  The bound is
never loosened."""
import functools

import numpy as np
import torch

import gru4rec_torch as gt

MARGIN = 1e-3
# csrc/gru4rec.hpp: kGru4recLossWaves, kGru4recRowTile, kGru4recSlabRows, kGru4recCandTile
LOSS_WAVES, ROW_TILE, SLAB_ROWS, CAND_TILE = 4, 64, 128, 64
LIMITS = {"layers": 3, "hidden": 128, "embedding": 128, "batch": 2048, "n_sample": 4096}      # kGru4recMax*
TILE_BATCHES = tuple(sorted({t + o for t in (LOSS_WAVES, ROW_TILE, SLAB_ROWS) for o in (-1, 0, 1)}))
TILE_SAMPLES = (0, CAND_TILE - 1 - 5, CAND_TILE - 5, CAND_TILE + 1 - 5)      # with B 5

BPR = dict(loss="bpr-max", bpreg=1.0, elu=1.0, logq=0.0, alpha=0.5)
XE = dict(loss="cross-entropy", bpreg=0.0, elu=0.0, logq=0.0, alpha=0.5)
SPECS = {
    "tiny": dict(BPR, layers=[1], D=0, B=1, S=1),
    "defaults": dict(BPR, layers=[100], D=0, B=7, S=5, elu=0.5, logq=1.0),
    "limits": dict(BPR, layers=[128, 128, 128], D=128, B=2, S=CAND_TILE + 1),
    "stacked": dict(BPR, layers=[5, 9, 3], D=6, B=6, S=4),
    "repeats": dict(BPR, layers=[6], D=0, B=8, S=6),
    "resets_all": dict(XE, layers=[4, 3], D=0, B=5, S=3),
    "resets_none": dict(XE, layers=[4, 3], D=0, B=5, S=3),
    "resets_mixed": dict(BPR, layers=[4, 3], D=5, B=5, S=3),
    "dropout": dict(BPR, layers=[12, 10], D=9, B=9, S=4, pe=0.5, ph=0.5),
    "logq": dict(XE, layers=[8], D=0, B=6, S=7, logq=1.0),
    "xe": dict(XE, layers=[10, 7], D=0, B=6, S=5),
    "max_batch": dict(XE, layers=[128], D=0, B=2048, S=4096, I=3000),
}
SPECS.update({f"elu_{a}_bpreg_{b}": dict(BPR, layers=[7], D=0, B=6, S=5, elu=float(a), bpreg=float(b))
              for a in ("0", "0.5", "1") for b in ("0", "1")})
SPECS.update({f"tile_edges_B_{B}": dict(BPR, layers=[3], D=0, B=B, S=2) for B in TILE_BATCHES})
SPECS.update({f"tile_edges_N_{S}": dict(BPR, layers=[3], D=0, B=5, S=S) for S in TILE_SAMPLES})
NAMES = tuple(SPECS)
# the fixtures the defect scan runs on (float64 on the CPU: the large ones add nothing there)
SCAN = ("defaults", "stacked", "repeats", "resets_mixed", "dropout", "logq", "xe", "elu_0.5_bpreg_1")


def cfg_of(f):
    return {k: f[k] for k in ("layers", "D", "loss", "bpreg", "elu", "logq", "alpha", "pe", "ph", "p")}


def _weights(rng, I, layers, D):
    w = {}
    for k, shape in gt.shapes(I, layers, D).items():
        if "bias" in k or k == "By.weight":
            scale = 0.5
        elif k == "Wy.weight":
            scale = 1.0 / np.sqrt(layers[-1])          # h is O(1) per unit: scores are O(1)
        elif k == "E.weight":
            scale = 1.0
        elif k == "G.0.weight_ih" and not D:
            scale = 1.0                                # its input rows are Wy's: 1 / sqrt(H_last) per entry
        else:
            scale = 1.0 / np.sqrt(shape[1])
        w[k] = (rng.standard_normal(shape) * scale).astype(np.float32)
    return w


def _build(name, seed):
    s = dict(SPECS[name])
    s.setdefault("pe", 0.0)
    s.setdefault("ph", 0.0)
    B, S, layers, D = s["B"], s["S"], s["layers"], s["D"]
    I = s.setdefault("I", 2 * B + S + 8)
    rng = np.random.default_rng(seed)
    f = dict(s, name=name, w=_weights(rng, I, layers, D), keeps=None)
    named = I - 3                                       # the last three rows are in no batch
    f["in_items"] = rng.integers(0, named, B)
    f["targets"] = rng.integers(0, named, B)
    f["samples"] = rng.integers(0, named, S)
    f["reset"] = (rng.random(B) < 0.4).astype(np.uint8)
    f["state"] = [(rng.uniform(-0.8, 0.8, (B, H))).astype(np.float32) for H in layers]
    support = rng.integers(1, 50, I)
    f["p"] = support / support.sum()
    if name == "resets_all":
        f["reset"][:] = 1
    if name == "resets_none":
        f["reset"][:] = 0
    if name == "resets_mixed":
        f["reset"][:] = [1, 0, 0, 1, 0]
    if name == "repeats":
        f["in_items"][:] = [3, 3, 1, 3, 3, 2, 3, 0]
        f["targets"][:] = [5, 4, 5, 5, 6, 5, 1, 0]
        f["samples"][:] = [7, 5, 7, 2, 9, 4]            # 7 twice; 5 and 4 are rows' own targets
    if s["pe"] or s["ph"]:
        shapes = [(B, gt.in_width(s))] + [(B, H) for H in layers]
        f["keeps"] = [(rng.random(sh) >= 0.5).astype(np.uint8) for sh in shapes]
    return f


def batch_of(f):
    return f["in_items"], f["targets"], f["reset"], f["samples"]


def elu_margin(f):
    """``(smallest |R|, largest |R|)`` of the fixture's score block in float64."""
    R = np.abs(gt.scores_R(f["w"], cfg_of(f), batch_of(f), f["state"], f["keeps"]))
    return float(R.min()), float(R.max())


def margins_ok(f):
    if f["loss"] != "bpr-max" or f["elu"] in (0.0, 1.0):
        return True
    lo, hi = elu_margin(f)
    return lo > MARGIN * hi


@functools.lru_cache(maxsize=None)
def fixture(name):
    """The fixture ``name`` from its own seed, or from the first seed after it at which ``margins_ok`` holds."""
    seed = 1000 * (NAMES.index(name) + 1)
    for k in range(200):
        f = _build(name, seed + k)
        if margins_ok(f):
            f["seed"] = seed + k
            return f
    raise AssertionError(f"{name}: the ELU margin does not hold at any of 200 seeds")


@functools.lru_cache(maxsize=None)
def reference(name):
    """``(loss64, grads64, state64, loss32, grads32)`` of the restatement; computed once, shared, never changed."""
    f = fixture(name)
    args = (f["w"], cfg_of(f), batch_of(f), f["state"], f["keeps"])
    l64, g64, s64 = gt.grads(*args, dtype=torch.float64)
    l32, g32, _ = gt.grads(*args, dtype=torch.float32)
    return l64, g64, s64, l32, g32


def untouched_rows(f):
    """Per table the rows no id of the step names."""
    cand = np.concatenate([f["targets"], f["samples"]])
    used = {"By.weight": cand}
    if f["D"]:
        used["Wy.weight"], used["E.weight"] = cand, f["in_items"]
    else:
        used["Wy.weight"] = np.concatenate([cand, f["in_items"]])
    return {k: np.setdiff1d(np.arange(f["I"]), ids) for k, ids in used.items()}
