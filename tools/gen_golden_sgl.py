"""ORACLE tooling (test infrastructure): capture the SGL golden vectors from the REAL reference.

Runs only where the reference tree exists (REFERENCE_ROOT, default: where oracle/gen_golden.py looks); the reference itself
never travels -- only the small .npz fixtures written to tests/golden/sgl_*.npz do.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_sgl.py

Builds the reference's own ``SGLEngine`` (beta_rec/models/sgl.py) on seeded synthetic interactions, lets its
``sub_mat_refresher`` draw the sub-graphs from ``np.random.seed(numpy_seed)`` and calls its ``train_single_batch`` three
times.  numpy 2 has removed ``np.mat``, which the reference still calls: the tool shims ``np.mat = np.asmatrix``.  The
loss parts of a step come from one more call of ``eng.model(...)`` before it (the forward draws nothing), the fp64
gradients from a double copy of the same module on the same inputs.

Asserted per step; a fixture that misses it is drawn again from another seed: the reference's fp32 gradients lie within
REL / 3 of the fp64 ones' scale (the GPU test allows REL of scale plus twice that distance).
"""
import contextlib
import copy
import io
import os
import sys
import types

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle.gen_golden import REF as _DEFAULT_REF  # noqa: E402  (where oracle/gen_golden.py finds the reference)

REF = os.environ.get("REFERENCE_ROOT", _DEFAULT_REF)
KEYS = ("user_embedding", "item_embedding")


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
    if not hasattr(np, "mat"):
        np.mat = np.asmatrix          # removed in numpy 2; sgl.py:269 / :584 still call it
    sys.path.insert(0, REF)
    from beta_rec.models.sgl import SGLEngine

    return SGLEngine


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def interactions(rng, U, I, per_user):
    """Unique (user, item) pairs with Zipf item degrees, in a shuffled order; every user and item keeps an edge."""
    pop = 1.0 / np.arange(1, I + 1) ** 0.8
    pop /= pop.sum()
    pairs = {(u % U, i) for u, i in enumerate(rng.permutation(I))} | {(u, int(rng.integers(0, I))) for u in range(U)}
    for u in range(U):
        n = int(rng.integers(max(1, per_user // 2), per_user * 2))
        for i in rng.choice(I, size=min(n, I), replace=False, p=pop):
            pairs.add((u, int(i)))
    pairs = np.array(sorted(pairs), dtype=np.int64)[rng.permutation(len(pairs))]
    return pairs[:, 0].copy(), pairs[:, 1].copy()


def norm_adj_of(eu, ei, U, I):
    """D^-1/2 A D^-1/2 of the whole training graph as a scipy CSR matrix in fp32 (what the reference's data layer passes)."""
    N = U + I
    A = sp.csr_matrix((np.ones(eu.size, dtype=np.float32), (eu, ei + U)), shape=(N, N))
    A = A + A.T
    d = np.power(np.asarray(A.sum(1)).flatten(), -0.5)
    d[np.isinf(d)] = 0.0
    return sp.diags(d).dot(A).dot(sp.diags(d)).tocsr().astype(np.float32)


class Loader:
    """What the reference reads of its train loader: ``dataset.user_tensor`` / ``dataset.pos_item_tensor``."""

    def __init__(self, users, items):
        self.dataset = types.SimpleNamespace(user_tensor=torch.from_numpy(users), pos_item_tensor=torch.from_numpy(items))


def sub_names(aug_type, L):
    return ["sub%d" % v for v in (1, 2)] if aug_type != 2 else ["sub%d%d" % (v, k) for k in range(1, L + 1) for v in (1, 2)]


def fixture(Engine, name, seed, **kw):
    from helpers import REL

    for attempt in range(20):
        out = one_fixture(Engine, REL, seed + 1000 * attempt, **kw)
        if isinstance(out, dict):
            break
        print(f"{name}: seed {seed + 1000 * attempt} rejected ({out})")
    else:
        raise SystemExit(f"{name}: no seed met the conditions")
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: losses {out['losses']}  parts {out['parts'][0]}  reference's own rounding "
          f"{float(out['own_rounding']):.2e} of scale  {os.path.getsize(path) / 1024:.0f} KiB")


def one_fixture(Engine, REL, seed, ssl_mode, aug_type, optimizer, lr, L, pretrain=0, hot=False, refresh_at=None,
                U=37, I=53, D=24, B=16, n_steps=3, regs=1e-3, ssl_reg=0.1, ssl_temp=0.2, ssl_ratio=0.4):
    rng = np.random.default_rng(seed)
    eu, ei = interactions(rng, U, I, 6)
    adj = norm_adj_of(eu, ei, U, I)
    coo = adj.tocoo()
    torch.manual_seed(seed)
    model = dict(n_users=U, n_items=I, emb_dim=D, n_layers=L, regs=regs, ssl_reg=ssl_reg, ssl_temp=ssl_temp,
                 ssl_mode=ssl_mode, ssl_ratio=ssl_ratio, aug_type=aug_type, is_subgraph=True, pretrain=pretrain,
                 norm_adj=adj, optimizer=optimizer, lr=lr, device_str="cpu", batch_size=B)
    eng = quiet(Engine, {"model": model, "system": {"run_dir": "/tmp/hiprec_golden_runs"}})
    eng.model.train()
    loader = Loader(eu, ei)
    pick = rng.integers(0, eu.size, size=(n_steps, B))
    if hot:          # half the rows of every batch repeat one user and one item
        pick[:, : B // 2] = pick[:, :1]
    users, pos = eu[pick], ei[pick]
    neg = rng.integers(0, I, size=(n_steps, B))

    def weights():
        return {k: v.detach().numpy().copy() for k, v in eng.model.state_dict().items()}

    assert tuple(weights()) == KEYS
    out = {"meta": np.array([U, I, D, L, B, n_steps, seed, aug_type, int(pretrain)], dtype=np.int64),
           "ssl_mode": np.array(ssl_mode), "optimizer": np.array(optimizer), "lr": np.array(lr),
           "hp": np.array([regs, ssl_reg, ssl_temp, ssl_ratio], dtype=np.float64),
           "inter_user": eu, "inter_item": ei, "adj_row": coo.row.astype(np.int64), "adj_col": coo.col.astype(np.int64),
           "adj_val": coo.data.astype(np.float32), "users": users, "pos": pos, "neg": neg,
           "torch_seed": np.array(seed), "numpy_seed": np.array(seed + 7)}
    for k, v in weights().items():
        out[f"w0/{k}"] = v
    np.random.seed(seed + 7)
    refresh_of_step, subs = [], []
    sub = None
    own, losses, parts_all = 0.0, [], []
    for s in range(n_steps):
        if s == 0 or s == refresh_at:
            sub = eng.sub_mat_refresher(loader)
            r = len(subs)
            for nm in sub_names(aug_type, L):
                out[f"sub{r}/{nm}/idx"] = np.asarray(sub["adj_indices_" + nm], dtype=np.int32)
                out[f"sub{r}/{nm}/val"] = np.asarray(sub["adj_values_" + nm], dtype=np.float32)
            subs.append(sub)
        refresh_of_step.append(len(subs) - 1)
        batch = tuple(torch.from_numpy(a[s]) for a in (users, pos, neg))
        state = np.random.get_state()[1].copy()
        with torch.no_grad():
            sl, emb, ssl = eng.model(sub, *batch)
        parts_all.append([float(sl), float(emb), float(ssl)])
        # the same forward in fp64 on the same inputs: a double copy of the module
        m64 = copy.deepcopy(eng.model).double()
        m64.adj_mat = m64.adj_mat.double()
        m64.device = eng.model.device
        sub64 = {k: (np.asarray(v, dtype=np.float64) if k.startswith("adj_values") else v) for k, v in sub.items()
                 if k.startswith("adj_")}
        sl64, emb64, ssl64 = m64(sub64, *batch)
        (sl64 + emb64 + ssl64).backward()
        g64 = {k: p.grad.detach().numpy().copy() for k, p in m64.named_parameters()}
        loss = eng.train_single_batch(sub, batch)
        assert np.array_equal(np.random.get_state()[1], state), "a training step drew from numpy"
        grads = {k: p.grad.detach().numpy().copy() for k, p in eng.model.named_parameters()}
        for k in KEYS:
            own = max(own, float(np.abs(grads[k] - g64[k]).max() / np.abs(g64[k]).max()))
        if own > REL / 3:
            return f"reference's own rounding {own:.2e}"
        loss64 = float((sl64 + emb64 + ssl64).detach())
        if abs(loss - loss64) > 1e-5 * abs(loss):
            return f"loss {loss} vs fp64 {loss64}"
        losses.append(loss)
        for k, v in weights().items():
            out[f"w{s + 1}/{k}"] = v
        for k in KEYS:
            out[f"g{s + 1}/{k}"] = grads[k]
            out[f"g64_{s + 1}/{k}"] = g64[k]
        for pname, p in eng.model.named_parameters():
            pst = eng.optimizer.state.get(p, {})
            for sk, tag in (("exp_avg", "m"), ("exp_avg_sq", "v"), ("square_avg", "v")):
                if sk in pst:
                    out[f"{tag}{s + 1}/{pname}"] = pst[sk].detach().numpy().copy()
    out["refresh_of_step"] = np.array(refresh_of_step, dtype=np.int64)
    out["losses"], out["parts"] = np.array(losses, dtype=np.float64), np.array(parts_all, dtype=np.float64)
    out["own_rounding"] = np.array(own)
    # the reference's predict reads the tables of the LAST training forward: the weights before the last step
    out["predict_users"], out["predict_items"] = users[0], neg[0]
    out["predict_scores_stale"] = eng.model.predict(users[0], neg[0]).numpy().copy()
    return out


def main():
    Engine = import_reference()
    fixture(Engine, "sgl_both_edge_adam", 41, ssl_mode="both_side", aug_type=1, optimizer="adam", lr=0.01, L=2)
    fixture(Engine, "sgl_user_walk_sgd", 42, ssl_mode="user_side", aug_type=2, optimizer="sgd", lr=0.05, L=3)
    fixture(Engine, "sgl_item_edge_rmsprop", 43, ssl_mode="item_side", aug_type=1, optimizer="rmsprop", lr=1e-3, L=1,
            ssl_temp=0.5)
    fixture(Engine, "sgl_pretrain_adam", 44, ssl_mode="both_side", aug_type=1, optimizer="adam", lr=0.01, L=2, pretrain=1)
    fixture(Engine, "sgl_hot_sgd", 45, ssl_mode="both_side", aug_type=1, optimizer="sgd", lr=0.05, L=2, hot=True)
    fixture(Engine, "sgl_refresh_walk_adam", 46, ssl_mode="both_side", aug_type=2, optimizer="adam", lr=0.01, L=2,
            refresh_at=2)


if __name__ == "__main__":
    main()
