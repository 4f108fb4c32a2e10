"""ORACLE tooling (test infrastructure): capture the SimGCL golden vectors from the REAL reference.

Runs only where the reference tree exists (REFERENCE_ROOT, default: where oracle/gen_golden.py looks); the reference itself
never travels -- only the small .npz fixtures written to tests/golden/simgcl_*.npz do.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_simgcl.py

Builds the reference's own ``SimGCLEngine`` (beta_rec/models/simgcl.py) on seeded synthetic interactions and calls its
``train_single_batch`` three times.  ``torch.rand_like`` is patched for the duration of a step: the reference calls it
with the PRE-noise tensor Y_k as its argument (simgcl.py:35), so the patch draws, sets the uniform to 0 wherever
0 < |y| < 1e-4 max|Y_k| (an element whose sign another summation order could flip; tests/simgcl_numpy.py: fragile_mask),
records and returns.  A step draws view 1's hops 1 .. L, then view 2's.  The loss parts of a step come from the numpy
restatement in fp64 on the recorded noise after its loss has been held to the reference's; the fp64 gradients from a
double copy of the same module replaying the recorded noise.

Asserted per step; a fixture that misses it is drawn again from another seed: the reference's fp32 gradients lie within
REL / 3 of the fp64 ones' scale (the GPU test allows REL of scale plus twice that distance), and at most 1 % of the
uniforms were zeroed.
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

import simgcl_numpy as sx  # noqa: E402
from helpers import REL, float64_oracle, to64  # noqa: E402

REF = os.environ.get("REFERENCE_ROOT", _DEFAULT_REF)
KEYS = sx.KEYS


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
    from beta_rec.models.simgcl import SimGCLEngine

    return SimGCLEngine


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def interactions(rng, U, I, per_user):
    """Unique (user, item) pairs with Zipf item degrees; every user and item keeps an edge."""
    pop = 1.0 / np.arange(1, I + 1) ** 0.8
    pop /= pop.sum()
    pairs = {(u % U, int(i)) for u, i in enumerate(rng.permutation(I))} | {(u, int(rng.integers(0, I))) for u in range(U)}
    for u in range(U):
        n = int(rng.integers(max(1, per_user // 2), per_user * 2))
        for i in rng.choice(I, size=min(n, I), replace=False, p=pop):
            pairs.add((u, int(i)))
    pairs = np.array(sorted(pairs), dtype=np.int64)[rng.permutation(len(pairs))]
    return pairs[:, 0].copy(), pairs[:, 1].copy()


def norm_adj_of(eu, ei, U, I):
    """D^-1/2 A D^-1/2 of the training graph as a scipy CSR matrix in fp32."""
    N = U + I
    A = sp.csr_matrix((np.ones(eu.size, dtype=np.float32), (eu, ei + U)), shape=(N, N))
    A = A + A.T
    d = np.power(np.asarray(A.sum(1)).flatten(), -0.5)
    d[np.isinf(d)] = 0.0
    return sp.diags(d).dot(A).dot(sp.diags(d)).tocsr().astype(np.float32)


class Noise:
    """The patch of ``torch.rand_like``: draw (or replay), zero the fragile elements, record."""

    def __init__(self, replay=None):
        self.drawn, self.zeroed, self.replay = [], 0, replay

    def __call__(self, y, *a, **k):
        if self.replay is not None:
            u = torch.from_numpy(self.replay[len(self.drawn)]).to(y.dtype)
            self.drawn.append(None)
            return u
        u = self.real(y, *a, **k)
        m = torch.from_numpy(sx.fragile_mask(y.detach().numpy()))
        self.zeroed += int(m.sum())
        u[m] = 0
        self.drawn.append(u.numpy().copy())
        return u

    def __enter__(self):
        self.real = torch.rand_like
        torch.rand_like = self
        return self

    def __exit__(self, *exc):
        torch.rand_like = self.real


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
    print(f"{name}: losses {out['losses']}  parts {out['parts'][0]}  reference's own rounding "
          f"{float(out['own_rounding']):.2e} of scale  zeroed {float(out['zeroed_share']):.2e}  "
          f"{os.path.getsize(path) / 1024:.0f} KiB")


def one_fixture(Engine, seed, optimizer, lr, L, D, U=40, I=60, B=48, hot=None, n_steps=3, eps=0.1, reg=1e-4, lam=0.5):
    rng = np.random.default_rng(seed)
    eu, ei = interactions(rng, U, I, 6)
    adj = norm_adj_of(eu, ei, U, I)
    coo = adj.tocoo()
    N = U + I
    torch.manual_seed(seed)
    tadj = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]).astype(np.int64), coo.data.astype(np.float32), (N, N))
    model = dict(n_users=U, n_items=I, emb_dim=D, n_layer=L, eps=eps, reg=reg, batch_size=B, norm_adj=tadj,
                 optimizer=optimizer, lr=lr, device_str="cpu")
    model["lambda"] = lam
    eng = quiet(Engine, {"model": model, "system": {"run_dir": "/tmp/hiprec_golden_runs"}})
    eng.model.train()
    if hot:          # every batch is drawn from a handful of users and items: n_uniq << B
        hu, hi = rng.choice(U, size=hot[0], replace=False), rng.choice(I, size=hot[1], replace=False)
        users, pos = hu[rng.integers(0, hot[0], size=(n_steps, B))], hi[rng.integers(0, hot[1], size=(n_steps, B))]
    else:
        pick = rng.integers(0, eu.size, size=(n_steps, B))
        users, pos = eu[pick], ei[pick]
    neg = rng.integers(0, I, size=(n_steps, B))
    graph = (coo.row.astype(np.int64), coo.col.astype(np.int64), coo.data.astype(np.float32), N)
    hp = dict(L=L, eps=eps, reg=reg, lam=lam, temp=0.2, user_view="reference")

    def weights():
        return {k: v.detach().numpy().copy() for k, v in eng.model.state_dict().items()}

    assert tuple(weights()) == KEYS
    out = {"meta": np.array([U, I, D, L, B, n_steps, seed], dtype=np.int64), "optimizer": np.array(optimizer),
           "lr": np.array(lr), "hp": np.array([eps, reg, lam, 0.2], dtype=np.float64), "inter_user": eu, "inter_item": ei,
           "adj_row": graph[0], "adj_col": graph[1], "adj_val": graph[2], "users": users, "pos": pos, "neg": neg,
           "torch_seed": np.array(seed)}
    for k, v in weights().items():
        out[f"w0/{k}"] = v
    own, zeroed, losses, parts_all, noises = 0.0, 0, [], [], []
    for s in range(n_steps):
        batch = tuple(torch.from_numpy(a[s]) for a in (users, pos, neg))
        w_s = weights()
        m64 = copy.deepcopy(eng.model).double()
        m64.norm_adj = m64.norm_adj.double()
        with Noise() as rec:
            loss = eng.train_single_batch(batch)
        assert len(rec.drawn) == 2 * L, "a step draws view 1's hops, then view 2's"
        noise = np.stack(rec.drawn).reshape(2, L, N, D)
        zeroed += rec.zeroed
        noises.append(noise)
        grads = {k: p.grad.detach().numpy().copy() for k, p in eng.model.named_parameters()}
        # the same step in fp64: a double copy of the module replaying the recorded noise
        ru, ri = m64.forward()
        ue, pe, ne = ru[batch[0]], ri[batch[1]], ri[batch[2]]
        with Noise(replay=rec.drawn):
            l64 = eng.bpr_loss(ue, pe, ne) + eng.l2_reg_loss(eng.reg, ue, pe, ne) + eng.cl_rate * m64.cal_cl_loss(
                batch[0], batch[1])
        l64.backward()
        g64 = {k: p.grad.detach().numpy().copy() for k, p in m64.named_parameters()}
        for k in KEYS:
            own = max(own, float(np.abs(grads[k] - g64[k]).max() / np.abs(g64[k]).max()))
        if own > REL / 3:
            return f"reference's own rounding {own:.2e}"
        if abs(loss - float(l64)) > 1e-5 * abs(loss):
            return f"loss {loss} vs fp64 {float(l64)}"
        with float64_oracle(sx):
            parts, l_np, g_np = sx.simgcl_grads(to64(w_s), graph, hp, tuple(a[s] for a in (users, pos, neg)), noise)
        assert abs(l_np - float(l64)) <= 1e-9 * abs(l_np), (l_np, float(l64))
        for k in KEYS:
            assert np.abs(g_np[k] - g64[k]).max() <= 1e-9 * np.abs(g64[k]).max(), k
        losses.append(loss)
        parts_all.append(parts)
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
    share = zeroed / (n_steps * 2 * L * N * D)
    if share > sx.ZEROED_CAP:
        return f"{share:.2%} of the uniforms zeroed"
    out["noise"] = np.stack(noises).astype(np.float32)
    out["losses"], out["parts"] = np.array(losses, dtype=np.float64), np.array(parts_all, dtype=np.float64)
    out["own_rounding"], out["zeroed_share"] = np.array(own), np.array(share)
    out["predict_users"], out["predict_items"] = users[0], neg[0]
    out["predict_scores"] = eng.model.predict(users[0], neg[0]).numpy().copy()
    return out


def main():
    Engine = import_reference()
    fixture(Engine, "simgcl_adam", 51, optimizer="adam", lr=0.001, L=2, D=16)
    fixture(Engine, "simgcl_sgd_hot_l3", 52, optimizer="sgd", lr=0.05, L=3, D=24, B=64, hot=(5, 7))
    fixture(Engine, "simgcl_rmsprop_d64_l1", 53, optimizer="rmsprop", lr=1e-3, L=1, D=64, reg=1e-2)


if __name__ == "__main__":
    main()
