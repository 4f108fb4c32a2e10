"""ORACLE tooling (test infrastructure): capture the UltraGCN golden vectors from the REAL reference.

Runs only where the reference tree exists (REFERENCE_ROOT, default: where oracle/gen_golden.py looks); the reference itself never
travels -- only the small .npz fixtures written to tests/golden/ug_*.npz do.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_ultragcn.py

Imports ``beta_rec.models.ultragcn`` and ``beta_rec.data.base_data`` with the same two in-process shims
``oracle/gen_golden.py`` uses (a recording ``tensorboardX`` stand-in; the numpy aliases removed in numpy 1.24) and drives
the reference's own ``UltraGCNEngine`` / ``BaseData.create_constraint_mat`` on seeded synthetic inputs.  Prints, per
fixture, the largest |score| (the tests' sigmoid().log() vs softplus argument needs < 20) and the share of neighbour
table entries whose id ``torch.topk`` leaves open (ties; tests/test_oracle_golden_ultragcn.py caps it at 10 %).
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle.gen_golden import REF as _DEFAULT_REF  # noqa: E402  (where oracle/gen_golden.py finds the reference)

REF = os.environ.get("REFERENCE_ROOT", _DEFAULT_REF)


def import_reference():
    sys.dont_write_bytecode = True
    tb = types.ModuleType("tensorboardX")

    class SummaryWriter:
        def __init__(self, *a, **k):
            self.scalars = []

        def add_scalar(self, tag, value, step=None):
            self.scalars.append((tag, float(value), step))

    tb.SummaryWriter = SummaryWriter
    sys.modules["tensorboardX"] = tb
    for name, typ in (("int", int), ("long", int), ("float", float), ("bool", bool)):
        if not hasattr(np, name):
            setattr(np, name, typ)
    sys.path.insert(0, REF)
    from beta_rec.data.base_data import BaseData
    from beta_rec.models.ultragcn import UltraGCNEngine
    from beta_rec.utils.constants import DEFAULT_ITEM_COL, DEFAULT_USER_COL

    return UltraGCNEngine, BaseData, DEFAULT_USER_COL, DEFAULT_ITEM_COL


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def interactions(rng, U, I, per_user):
    """A 0/1 interaction list in which every user and every item occurs; item popularity is skewed so that the degrees
    (and with them the entries of Omega) differ from item to item."""
    pop = 1.0 / np.arange(1, I + 1) ** 0.7
    pop /= pop.sum()
    pairs = set()
    for u in range(U):
        n = int(rng.integers(max(1, per_user // 2), per_user * 2))
        for i in rng.choice(I, size=min(n, I), replace=False, p=pop):
            pairs.add((u, int(i)))
    for i in range(I):                      # items nobody drew
        if not any(p[1] == i for p in pairs):
            pairs.add((int(rng.integers(0, U)), i))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    return pairs[:, 0], pairs[:, 1]


def reference_constraints(BaseData, ucol, icol, U, I, users, items):
    """BaseData.create_constraint_mat (base_data.py:410-431) run on a stand-in that has the three attributes it reads."""
    import pandas as pd

    stub = types.SimpleNamespace(n_users=U, n_items=I, train=pd.DataFrame({ucol: users, icol: items}))
    return BaseData.create_constraint_mat(stub)


def open_share(train_mat, K, nbr, sim):
    """Share of the non-zero table entries whose id the reference's topk does not determine (tests' rule 1)."""
    import ultragcn_numpy as ug

    om = ug.omega_matrix(np.asarray(train_mat.todense()))
    srt = -np.sort(-om, axis=1)
    excluded = srt[:, K] if om.shape[1] > K else np.zeros(om.shape[0], dtype=np.float32)
    nz = sim != 0
    left = np.concatenate([np.full((sim.shape[0], 1), np.inf, dtype=np.float32), sim[:, :-1]], axis=1)
    right = np.concatenate([sim[:, 1:], excluded[:, None]], axis=1)
    determined = nz & (sim != left) & (sim != right)
    return 1.0 - determined.sum() / max(1, nz.sum())


def reference_rounding(out, n_steps, hp, nbr, sim):
    """Largest distance, relative to the tensor's scale, of a captured gradient from the fp64 restatement's."""
    import ultragcn_numpy as ug
    from helpers import float64_oracle, to64

    worst = 0.0
    for s in range(n_steps):
        w = {k: out[f"w{s}/{k}"] for k in ug.KEYS}
        with float64_oracle(ug):
            _, g64 = ug.ug_grads(to64(w), out["users"][s], out["pos"][s], out["neg"][s], hp, out["beta_u"], out["beta_i"],
                                 nbr, sim)
        for k in ug.KEYS:
            worst = max(worst, float(np.abs(out[f"g{s + 1}/{k}"] - g64[k]).max() / np.abs(g64[k]).max()))
    return worst


def config_for(U, I, D, B, K, optimizer, lr, train_mat, beta_uD, beta_iD, hp):
    model = dict(n_users=U, n_items=I, emb_dim=D, batch_size=B, regs=[1e-5], optimizer=optimizer, lr=lr,
                 device_str="cpu", train_mat=train_mat, constraint_mat={"beta_uD": beta_uD, "beta_iD": beta_iD},
                 ii_neighbor_num=K, **hp)
    return {"model": model, "system": {"run_dir": "/tmp/hiprec_golden_runs"}}


DEFAULT_HP = {"w1": 1e-7, "w2": 1.0, "w3": 1e-7, "w4": 1.0, "negative_weight": 200.0, "gamma": 1e-4, "lambda": 1e-3}


def fixture(ref, name, U, I, D, B, N, K, optimizer, lr, n_steps, seed, scale, per_user, hp=None, hot=None):
    Engine, BaseData, ucol, icol = ref
    hp = dict(DEFAULT_HP, **(hp or {}))
    rng = np.random.default_rng(seed)
    tu, ti = interactions(rng, U, I, per_user)
    train_mat, beta_uD, beta_iD = reference_constraints(BaseData, ucol, icol, U, I, tu, ti)
    torch.manual_seed(seed)
    eng = quiet(Engine, config_for(U, I, D, B, K, optimizer, lr, train_mat, beta_uD, beta_iD, hp))
    with torch.no_grad():
        # the reference's init (std 1e-3) keeps every score within 1e-4 of zero, where every sigmoid is 0.5; scaled
        # tables spread the scores over several units
        eng.model.user_embeds.weight.mul_(scale)
        eng.model.item_embeds.weight.mul_(scale)
    nbr, sim = eng.model.ii_neighbor_mat.numpy().copy(), eng.model.ii_constraint_mat.numpy().copy()
    out = {"meta": np.array([U, I, D, B, N, K, n_steps, seed], dtype=np.int64), "optimizer": np.array(optimizer),
           "lr": np.array(lr), "hp_names": np.array(sorted(hp)), "hp": np.array([hp[k] for k in sorted(hp)]),
           "train_users": tu, "train_items": ti,
           "beta_u": np.asarray(beta_uD, dtype=np.float32).reshape(-1), "beta_i": np.asarray(beta_iD, dtype=np.float32).reshape(-1),
           "ii_neighbor_mat": nbr, "ii_constraint_mat": sim}
    for k, v in eng.model.state_dict().items():
        out[f"w0/{k}"] = v.detach().numpy().copy()
    seen = []
    orig_step = eng.optimizer.step

    def capturing_step(*a, **k):
        seen.append({n: p.grad.detach().numpy().copy() for n, p in eng.model.named_parameters()})
        return orig_step(*a, **k)

    eng.optimizer.step = capturing_step
    if hot:
        # many terms on few rows: positives from n_pairs training pairs (repeated (u, p)), negatives Zipf(skew)
        n_pairs, skew = hot
        few = rng.choice(len(tu), size=n_pairs, replace=False)
        pick = few[rng.integers(0, len(few), size=(n_steps, B))]
        pz = 1.0 / np.arange(1, I + 1) ** skew
        neg = rng.permutation(I)[rng.choice(I, size=(n_steps, B, N), p=pz / pz.sum())]
    else:
        pick = rng.integers(0, len(tu), size=(n_steps, B))
        neg = rng.integers(0, I, size=(n_steps, B, N))
    users, pos = tu[pick], ti[pick]
    out["users"], out["pos"], out["neg"] = users, pos, neg
    losses, max_score = [], 0.0
    for s in range(n_steps):
        with torch.no_grad():
            Uw, Vw = eng.model.user_embeds.weight, eng.model.item_embeds.weight
            ids = np.concatenate([pos[s][:, None], neg[s], nbr[pos[s]]], axis=1)
            sc = (Uw[torch.from_numpy(users[s])][:, None, :] * Vw[torch.from_numpy(ids)]).sum(-1)
            max_score = max(max_score, float(sc.abs().max()))
        losses.append(eng.train_single_batch((torch.from_numpy(users[s]), torch.from_numpy(pos[s]),
                                              torch.from_numpy(neg[s]))))
        for k, v in eng.model.state_dict().items():
            out[f"w{s + 1}/{k}"] = v.detach().numpy().copy()
        for k, v in seen[-1].items():
            out[f"g{s + 1}/{k}"] = v
        for pname, p in eng.model.named_parameters():
            pst = eng.optimizer.state.get(p, {})
            for sk, tag in (("exp_avg", "m"), ("exp_avg_sq", "v"), ("square_avg", "v")):
                if sk in pst:
                    out[f"{tag}{s + 1}/{pname}"] = pst[sk].detach().numpy().copy()
    own = reference_rounding(out, n_steps, hp, nbr, sim)
    with torch.no_grad():
        out["predict_users"], out["predict_items"] = users[0], neg[0][:, 0]
        out["predict_scores"] = eng.model.predict(users[0], neg[0][:, 0]).numpy().copy()   # with the FINAL weights
    out["losses"] = np.array(losses, dtype=np.float64)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    assert max_score < 20.0, f"{name}: |score| reaches {max_score}"
    share = open_share(train_mat, K, nbr, sim)
    assert share <= 0.10, f"{name}: topk leaves {share:.1%} of the table entries open; change the matrix"
    # the tests hold an implementation to 1e-5 of a gradient's scale AGAINST THESE VECTORS: that only means something
    # while the reference's own fp32 rounding (its distance from the fp64 gradient) stays well inside that bound
    assert own <= 1e-5 / 3, f"{name}: the reference's own gradient is {own:.2e} of its scale from the exact one"
    print(f"{name}: losses {losses}  max|s| {max_score:.2f}  open table entries {share:.2%}  "
          f"reference's own rounding {own:.2e} of scale  {os.path.getsize(path) / 1024:.0f} KiB")


def init_fixture(ref):
    """Seeded construction: initial weights and the Omega tables."""
    Engine, BaseData, ucol, icol = ref
    out = {}
    for tag, (U, I, D, K, seed, per_user) in {"a": (25, 18, 4, 3, 3, 5), "b": (60, 50, 64, 10, 2020, 8)}.items():
        rng = np.random.default_rng(seed)
        tu, ti = interactions(rng, U, I, per_user)
        train_mat, beta_uD, beta_iD = reference_constraints(BaseData, ucol, icol, U, I, tu, ti)
        torch.manual_seed(seed)
        eng = quiet(Engine, config_for(U, I, D, 8, K, "adam", 1e-3, train_mat, beta_uD, beta_iD, DEFAULT_HP))
        out[f"{tag}/meta"] = np.array([U, I, D, K, seed], dtype=np.int64)
        out[f"{tag}/train_users"], out[f"{tag}/train_items"] = tu, ti
        out[f"{tag}/beta_u"] = np.asarray(beta_uD, dtype=np.float32).reshape(-1)
        out[f"{tag}/beta_i"] = np.asarray(beta_iD, dtype=np.float32).reshape(-1)
        out[f"{tag}/ii_neighbor_mat"] = eng.model.ii_neighbor_mat.numpy().copy()
        out[f"{tag}/ii_constraint_mat"] = eng.model.ii_constraint_mat.numpy().copy()
        for k, v in eng.model.state_dict().items():
            out[f"{tag}/w/{k}"] = v.detach().numpy().copy()
        share = open_share(train_mat, K, out[f"{tag}/ii_neighbor_mat"], out[f"{tag}/ii_constraint_mat"])
        assert share <= 0.10, f"ug_init {tag}: topk leaves {share:.1%} of the table entries open"
        print(f"ug_init {tag}: open table entries {share:.2%}")
    np.savez_compressed(os.path.join(OUT, "ug_init.npz"), **out)


def main():
    ref = import_reference()
    # ultragcn_default.json values at a toy size
    fixture(ref, "ug_adam", 40, 30, 16, 32, 20, 5, "adam", 0.05, 3, 21, scale=700.0, per_user=6)
    # width that is not a multiple of 64, odd N, K 3, constant negative weight (w4 = 0)
    fixture(ref, "ug_sgd_d100", 40, 30, 100, 24, 7, 3, "sgd", 0.05, 3, 22, scale=420.0, per_user=6,
            hp={"w4": 0.0, "w3": 0.02})
    # many terms colliding on few rows: 40 distinct (u, p) pairs, Zipf(0.6) negatives -- as hot as the reference's own fp32
    # sums allow (a row hit by n terms is off by ~sqrt(n) eps there; see the check at the end of fixture())
    fixture(ref, "ug_rmsprop_hot", 300, 200, 64, 256, 50, 10, "rmsprop", 1e-3, 2, 23, scale=480.0, per_user=10, hot=(40, 0.6))
    init_fixture(ref)


if __name__ == "__main__":
    main()
