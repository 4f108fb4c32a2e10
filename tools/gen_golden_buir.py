"""ORACLE tooling (test infrastructure): capture the BUIR golden vectors from the REAL reference.

Runs only where the reference tree exists (REFERENCE_ROOT, default: where oracle/gen_golden.py looks); the reference itself
never travels -- only the small .npz fixtures written to tests/golden/buir_*.npz do.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_buir.py

Builds the reference's own ``BUIREngine`` (beta_rec/models/buir.py) on seeded synthetic interactions, on the CPU, and calls
its ``train_single_batch`` three times.  Recorded per step: the weights before and after, the gradients, the optimizer
moments, the loss, and the fp64 gradients of a double copy of the same module.  ``buir_adam_ema`` also calls the
reference's own ``_update_target()`` after every step (the reference defines it and never calls it), which pins the
moving-target extension to the reference's code.

Asserted per step; a fixture that misses it is drawn again from another seed: the reference's fp32 gradients lie within
REL / 3 of the fp64 ones' scale (the GPU test allows REL of scale plus twice that distance).
"""
import copy
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from oracle.gen_golden import REF as _DEFAULT_REF  # noqa: E402  (where oracle/gen_golden.py finds the reference)

import buir_numpy as bx  # noqa: E402
from gen_golden_simgcl import interactions, norm_adj_of, quiet  # noqa: E402
from helpers import REL, float64_oracle, to64  # noqa: E402

REF = os.environ.get("REFERENCE_ROOT", _DEFAULT_REF)
KEYS, TRAINABLE = bx.KEYS, bx.TRAINABLE


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
    sys.path.insert(0, REF)
    from beta_rec.models.buir import BUIREngine

    return BUIREngine


def fixture(Engine, name, seed, **kw):
    for attempt in range(20):
        out = one_fixture(Engine, seed + 1000 * attempt, **kw)
        if isinstance(out, dict):
            break
        print(f"{name}: seed {seed + 1000 * attempt} rejected ({out})")
    else:
        raise SystemExit(f"{name}: no seed met the conditions")
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: losses {out['losses']}  reference's own rounding {float(out['own_rounding']):.2e} of scale  "
          f"{os.path.getsize(path) / 1024:.0f} KiB")


def double_copy(model):
    m64 = copy.deepcopy(model).double()
    for enc in (m64.online_encoder, m64.target_encoder):
        enc.norm_adj = enc.sparse_norm_adj = enc.sparse_norm_adj.double()
    return m64


def one_fixture(Engine, seed, optimizer, lr, D, U=40, I=60, B=48, hot=None, n_steps=3, momentum=0.9, ema=False):
    rng = np.random.default_rng(seed)
    eu, ei = interactions(rng, U, I, 6)
    coo = norm_adj_of(eu, ei, U, I).tocoo()
    N, L = U + I, 3                                    # buir.py:18: n_layers = 3 is hard-coded
    torch.manual_seed(seed)
    tadj = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]).astype(np.int64), coo.data.astype(np.float32), (N, N))
    model = dict(n_users=U, n_items=I, emb_dim=D, momentum=momentum, batch_size=B, norm_adj=tadj, optimizer=optimizer,
                 lr=lr, device_str="cpu")
    eng = quiet(Engine, {"model": model, "system": {"run_dir": "/tmp/hiprec_golden_runs"}})
    eng.model.train()
    if hot:          # every batch is drawn from a handful of users and items: every scatter row is contended
        hu, hi = rng.choice(U, size=hot[0], replace=False), rng.choice(I, size=hot[1], replace=False)
        users, pos = hu[rng.integers(0, hot[0], size=(n_steps, B))], hi[rng.integers(0, hot[1], size=(n_steps, B))]
    else:
        pick = rng.integers(0, eu.size, size=(n_steps, B))
        users, pos = eu[pick], ei[pick]
    neg = rng.integers(0, I, size=(n_steps, B))
    graph = (coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float32), N)

    def weights():
        return {k: v.detach().numpy().copy() for k, v in eng.model.state_dict().items()}

    out = {"meta": np.array([U, I, D, L, B, n_steps, seed], dtype=np.int64), "optimizer": np.array(optimizer),
           "lr": np.array(lr), "momentum": np.array(momentum), "ema": np.array(int(ema)), "adj_row": graph[0],
           "adj_col": graph[1], "adj_val": graph[2], "users": users, "pos": pos, "neg": neg, "torch_seed": np.array(seed),
           "state_dict_keys": np.array(list(eng.model.state_dict()))}
    assert tuple(out["state_dict_keys"]) == KEYS
    for k, v in weights().items():
        out[f"w0/{k}"] = v
    own, losses = 0.0, []
    for s in range(n_steps):
        batch = tuple(torch.from_numpy(a[s]) for a in (users, pos, neg))
        w_s = weights()
        m64 = double_copy(eng.model)
        loss = eng.train_single_batch(batch)
        named = dict(eng.model.named_parameters())
        assert all(named[k].grad is None for k in bx.TARGET), "nothing reaches the target"
        grads = {k: named[k].grad.detach().numpy().copy() for k in TRAINABLE}
        l64 = m64.get_loss(m64(batch[0], batch[1]))
        l64.backward()
        l64 = float(l64.detach())
        n64 = dict(m64.named_parameters())
        g64 = {k: n64[k].grad.detach().numpy().copy() for k in TRAINABLE}
        for k in TRAINABLE:
            own = max(own, float(np.abs(grads[k] - g64[k]).max() / np.abs(g64[k]).max()))
        if own > REL / 3:
            return f"reference's own rounding {own:.2e}"
        if abs(loss - l64) > 1e-5 * abs(loss):
            return f"loss {loss} vs fp64 {l64}"
        with float64_oracle(bx):
            l_np, g_np = bx.buir_grads(to64(w_s), graph, L, (users[s], pos[s], neg[s]))
        assert abs(l_np - l64) <= 1e-9 * abs(l_np), (l_np, l64)
        for k in TRAINABLE:
            assert np.abs(g_np[k] - g64[k]).max() <= 1e-9 * np.abs(g64[k]).max(), k
        if ema:
            eng.model._update_target()
        losses.append(loss)
        for k, v in weights().items():
            out[f"w{s + 1}/{k}"] = v
        for k in TRAINABLE:
            out[f"g{s + 1}/{k}"] = grads[k]
            out[f"g64_{s + 1}/{k}"] = g64[k]
        for pname, p in eng.model.named_parameters():
            pst = eng.optimizer.state.get(p, {})
            for sk, tag in (("exp_avg", "m"), ("exp_avg_sq", "v"), ("square_avg", "v")):
                if sk in pst:
                    out[f"{tag}{s + 1}/{pname}"] = pst[sk].detach().numpy().copy()
    out["losses"], out["own_rounding"] = np.array(losses, dtype=np.float64), np.array(own)
    out["predict_users"], out["predict_items"] = users[0], neg[0]
    out["predict_scores"] = eng.model.predict(users[0], neg[0]).numpy().copy()
    return out


def main():
    Engine = import_reference()
    fixture(Engine, "buir_adam", 61, optimizer="adam", lr=0.001, D=16)
    fixture(Engine, "buir_sgd_hot", 62, optimizer="sgd", lr=0.05, D=24, B=64, hot=(5, 7))
    fixture(Engine, "buir_rmsprop_d64", 63, optimizer="rmsprop", lr=1e-3, D=64, U=20, I=30, B=32)
    fixture(Engine, "buir_adam_ema", 64, optimizer="adam", lr=0.001, D=16, ema=True)


if __name__ == "__main__":
    main()
