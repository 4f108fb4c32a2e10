"""ORACLE tooling (test infrastructure): capture the MixGCF golden vectors from the REAL reference.

Runs only where the reference tree exists (REFERENCE_ROOT, default: where oracle/gen_golden.py looks); the reference itself
never travels -- only the small .npz fixtures written to tests/golden/mix_*.npz do.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_mixgcf.py

Builds the reference's own ``LightGCNEngine`` (beta_rec/models/mixgcf.py) on seeded synthetic graphs and calls its
``train_single_batch``, which returns the loss TENSOR and stops there (it never calls ``backward()`` or
``optimizer.step()``); this tool then calls ``loss.backward()`` and ``engine.optimizer.step()`` itself, so the recorded
gradients and updates are autograd's and torch.optim's on the reference's own graph.  The draws of a step (per hop the
edge ``rand(nnz)`` and the message ``bernoulli_``, then per k the seed ``rand(B, 1, L + 1, 1)``) are made ahead of the
reference from a saved generator state, in that order, and the generator is put back; after the reference's step the
generator must stand where the replay ended, which pins the order.

Two conditions, asserted per step; a fixture that misses one is generated again from another seed.  (a) Every (row, k,
hop) argmax wins by 1e-4 of the row's largest |score| in fp64 against every candidate that is another item, and the
reference, the fp32 and the fp64 restatement choose alike.  With a hundred-odd near-independent argmaxes per step no
whole batch ever meets this by chance, so it is met row by row: a row with a lead under 2e-4 draws its candidates
again (the seeds are known by then) before the reference sees the batch.  (b) The reference's gradients lie within
REL / 3 of the fp64 restatement's scale.
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
MARGIN = 1e-4


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
    from beta_rec.models.mixgcf import LightGCNEngine

    return LightGCNEngine


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def skewed_graph(rng, U, I, per_user):
    """D^-1 (A + I) of a bipartite graph with Zipf item degrees, as COO in a SHUFFLED order (the reference never
    coalesces; the order is the one its edge mask is drawn in)."""
    pop = 1.0 / np.arange(1, I + 1) ** 0.8
    pop /= pop.sum()
    pairs = set()
    for u in range(U):
        n = int(rng.integers(max(1, per_user // 2), per_user * 2))
        for i in rng.choice(I, size=min(n, I), replace=False, p=pop):
            pairs.add((u, int(i)))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    eu, ei = pairs[:, 0], pairs[:, 1]
    N = U + I
    rows = np.concatenate([eu, U + ei, np.arange(N)])
    cols = np.concatenate([U + ei, eu, np.arange(N)])
    deg = np.bincount(rows, minlength=N).astype(np.float64)
    vals = (1.0 / deg[rows]).astype(np.float32)
    perm = rng.permutation(rows.size)
    return eu, ei, rows[perm], cols[perm], vals[perm]


def rows_ok(mx, E64, U, users, pos, cand, seeds, pool):
    """Per batch row: condition (a) for the fp64 argmax itself."""
    sc = mx.sampler_scores(E64, U, users, pos, cand, seeds, pool)          # [B, K, n, H]
    first = sc.argmax(axis=2)
    best = np.take_along_axis(sc, first[:, :, None, :], axis=2)
    other = cand[..., None] != np.take_along_axis(cand[..., None], first[:, :, None, :], axis=2)
    gap = np.where(other, best - sc, np.inf).min(axis=2)
    scale = np.abs(sc).max(axis=(1, 2, 3))[:, None, None]
    return (gap >= 2 * MARGIN * scale).all(axis=(1, 2))                    # (twice the margin: the recorded vectors keep room)


def margins_ok(mx, E64, U, users, pos, cand, seeds, pool, choice):
    """Condition (a) in fp64: the winner beats every candidate that is ANOTHER item by MARGIN of the row's largest
    |score| (copies of one item tie exactly; the first of them wins everywhere)."""
    sc = mx.sampler_scores(E64, U, users, pos, cand, seeds, pool)          # [B, K, n, H]
    if sc.shape[2] == 1:
        return True
    best = np.take_along_axis(sc, choice[:, :, None, :], axis=2)           # [B, K, 1, H]
    win_item = np.take_along_axis(cand[..., None], choice[:, :, None, :], axis=2)
    other = cand[..., None] != win_item
    gap = np.where(other, best - sc, np.inf).min(axis=2)                   # [B, K, H]
    scale = np.abs(sc).max(axis=(1, 2, 3))[:, None, None]
    first = sc.argmax(axis=2)
    return bool((gap >= MARGIN * scale).all() and np.array_equal(first, choice))


def fixture(Engine, name, pool, D, L, n_negs, K, edge_rate, mess_rate, optimizer, lr, seed, ns="mixgcf", hot=False,
            U=30, I=24, B=33, n_steps=3, l2=1e-4, extra_cols=0):
    import mixgcf_numpy as mx
    from helpers import REL, float64_oracle, to64

    for attempt in range(20):
        out = one_fixture(Engine, mx, float64_oracle, to64, REL, pool, D, L, n_negs, K, edge_rate, mess_rate, optimizer,
                          lr, seed + 1000 * attempt, ns, hot, U, I, B, n_steps, l2, extra_cols)
        if isinstance(out, dict):
            break
        print(f"{name}: seed {seed + 1000 * attempt} rejected ({out})")
    else:
        raise SystemExit(f"{name}: no seed met the conditions")
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: losses {out['losses']}  max|x| {float(out['max_x']):.2f}  reference's own rounding "
          f"{float(out['own_rounding']):.2e} of scale  {os.path.getsize(path) / 1024:.0f} KiB")


def one_fixture(Engine, mx, float64_oracle, to64, REL, pool, D, L, n_negs, K, edge_rate, mess_rate, optimizer, lr, seed, ns,
                hot, U, I, B, n_steps, l2, extra_cols):
    rng = np.random.default_rng(seed)
    eu, ei, rows, cols, vals = skewed_graph(rng, U, I, 5)
    N, H, nnz = U + I, L + 1, rows.size
    graph = (rows, cols, vals, N)
    norm_t = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([rows, cols])), torch.from_numpy(vals), (N, N))
    torch.manual_seed(seed)
    model = dict(n_users=U, n_items=I, emb_dim=D, pool=pool, context_hops=L, mess_dropout=mess_rate is not None,
                 mess_dropout_rate=0.1 if mess_rate is None else mess_rate, edge_dropout=edge_rate is not None,
                 edge_dropout_rate=0.5 if edge_rate is None else edge_rate, norm_adj=norm_t, l2=l2, n_negs=n_negs, ns=ns,
                 K=K, optimizer=optimizer, lr=lr, device_str="cpu", batch_size=B)
    eng = quiet(Engine, {"model": model, "system": {"run_dir": "/tmp/hiprec_golden_runs"}})
    eng.model.train()
    hp = dict(pool=pool, L=L, n_negs=n_negs, K=K, ns=ns, l2=l2, edge_rate=edge_rate, mess_rate=mess_rate)
    M = (K if ns == "rns" else K * n_negs) + extra_cols
    if hot:   # 40 distinct (u, pos) pairs; Zipf candidates, so that rows repeat an item
        few = rng.choice(len(eu), size=40, replace=False)
        pick = few[rng.integers(0, 40, size=(n_steps, B))]
        pz = 1.0 / np.arange(1, I + 1) ** 1.1
        item_of_rank = rng.permutation(I)

        def draw_neg(*shape):
            return item_of_rank[rng.choice(I, size=shape, p=pz / pz.sum())]
    else:
        pick = rng.integers(0, len(eu), size=(n_steps, B))

        def draw_neg(*shape):
            return rng.integers(0, I, size=shape)
    neg = draw_neg(n_steps, B, M)
    users, pos = eu[pick], ei[pick]

    def weights():
        return {k: v.detach().numpy().copy() for k, v in eng.model.state_dict().items()}

    # scale the tables (as oracle/gen_golden.py scales NGCF's) until |x_k| spreads over several units, below 20
    for _ in range(3):
        sc = mx.mix_predict(weights(), graph, hp, np.repeat(users[0], 2), np.concatenate([pos[0], neg[0][:, 0]]))
        with torch.no_grad():
            f = float(np.sqrt(6.0 / max(float(np.abs(sc).max()), 1e-30)))
            eng.model.user_embedding.weight.mul_(f)
            eng.model.item_embedding.weight.mul_(f)
    out = {"meta": np.array([U, I, D, L, B, n_negs, K, n_steps, seed], dtype=np.int64), "pool": np.array(pool),
           "ns": np.array(ns), "optimizer": np.array(optimizer), "lr": np.array(lr), "l2": np.array(l2),
           "edge_rate": np.array(np.nan if edge_rate is None else edge_rate),
           "mess_rate": np.array(np.nan if mess_rate is None else mess_rate),
           "adj_row": rows, "adj_col": cols, "adj_val": vals, "users": users, "pos": pos, "neg": neg,
           "torch_seed": np.array(seed + 7)}
    for k, v in weights().items():
        out[f"w0/{k}"] = v
    torch.manual_seed(seed + 7)
    seeds_all, edge_all, mess_all, choice_all, losses = [], [], [], [], []
    own, max_x = 0.0, 0.0
    for s in range(n_steps):
        w_before = weights()
        state0 = torch.get_rng_state()
        # the draws the reference is about to make, in its order (the generator is put back before it runs)
        edge, mess = [], []
        for _l in range(L):
            if edge_rate is not None:
                edge.append(torch.floor(edge_rate + torch.rand(nnz)).type(torch.bool).numpy().astype(np.uint8))
            if mess_rate is not None and mess_rate > 0:
                mess.append(torch.empty(N, D).bernoulli_(1 - mess_rate).numpy().astype(np.uint8))
        sd = np.stack([torch.rand(B, 1, H, 1).view(B, H).numpy().copy() for _ in range(K)], axis=1) if ns != "rns" else \
            np.zeros((B, K, H), dtype=np.float32)
        state_replayed = torch.get_rng_state()
        torch.set_rng_state(state0)
        masks = (edge if edge else None, mess if mess else None)
        with float64_oracle(mx):
            w64 = to64(w_before)
            E64, _, _ = mx.propagate(w64, graph, hp, masks)
        if ns != "rns":
            # condition (a), met row by row: a row with a near tie draws its candidates again
            for _ in range(500):
                bad = ~rows_ok(mx, E64, U, users[s], pos[s], mx.candidates(neg[s], hp), sd.astype(np.float64), pool)
                if not bad.any():
                    break
                neg[s][bad] = draw_neg(int(bad.sum()), M)
            else:
                return "argmax margin"
        seen = []
        real_max = torch.max

        def recording_max(*a, **k):
            r = real_max(*a, **k)
            if k.get("dim") == 1:
                seen.append(r[1].detach().numpy().copy())
            return r

        torch.max = recording_max
        try:
            loss = eng.train_single_batch((torch.from_numpy(users[s]), torch.from_numpy(pos[s]), torch.from_numpy(neg[s])))
        finally:
            torch.max = real_max
        state1 = torch.get_rng_state()
        assert loss.requires_grad
        if s == 0:   # the deviation the mirror records: the reference's own step moves nothing
            for k, v in weights().items():
                out[f"ref_after_step/{k}"] = v
                assert np.array_equal(v, w_before[k])
        assert torch.equal(state1, state_replayed), "the reference's draws are not the replayed ones: the order differs"
        choice = np.stack(seen, axis=1).astype(np.int32) if ns != "rns" else np.zeros((B, K, H), dtype=np.int32)
        assert choice.shape == (B, K, H)
        eng.optimizer.zero_grad()
        loss.backward()
        grads = {n: p.grad.detach().numpy().copy() for n, p in eng.model.named_parameters()}
        eng.optimizer.step()
        # conditions (a) and (b)
        with float64_oracle(mx):
            cand = mx.candidates(neg[s], hp)
            if ns != "rns" and not margins_ok(mx, E64, U, users[s], pos[s], cand, sd.astype(np.float64), pool, choice):
                return "argmax margin"
            l64, g64, c64 = mx.mix_grads(w64, graph, hp, (users[s], pos[s], neg[s]), sd, masks)
        l32, g32, c32 = mx.mix_grads(w_before, graph, hp, (users[s], pos[s], neg[s]), sd, masks)
        if not (np.array_equal(c64, choice) and np.array_equal(c32, choice)):
            return "restatement chooses differently"
        for k in mx.KEYS:
            own = max(own, float(np.abs(grads[k] - g64[k]).max() / np.abs(g64[k]).max()))
        if own > REL / 3:
            return f"reference's own rounding {own:.2e}"
        if abs(float(loss.detach()) - l64) > 1e-5 * abs(l64):
            return f"loss {float(loss)} vs restatement {l64}"
        max_x = max(max_x, float(np.abs(mx.mix_predict(w64, graph, hp, users[s], pos[s])).max()))
        seeds_all.append(sd)
        edge_all.append(np.stack(edge) if edge else np.zeros((0, nnz), np.uint8))
        mess_all.append(np.stack(mess) if mess else np.zeros((0, N, D), np.uint8))
        choice_all.append(choice)
        losses.append(float(loss.detach()))
        for k, v in weights().items():
            out[f"w{s + 1}/{k}"] = v
        for k, v in grads.items():
            out[f"g{s + 1}/{k}"] = v
        for pname, p in eng.model.named_parameters():
            pst = eng.optimizer.state.get(p, {})
            for sk, tag in (("exp_avg", "m"), ("exp_avg_sq", "v"), ("square_avg", "v")):
                if sk in pst:
                    out[f"{tag}{s + 1}/{pname}"] = pst[sk].detach().numpy().copy()
    if max_x >= 20.0:
        return f"|score| reaches {max_x}"
    out["seeds"], out["edge_keep"], out["mess_keep"] = np.stack(seeds_all), np.stack(edge_all), np.stack(mess_all)
    out["choice"], out["losses"] = np.stack(choice_all), np.array(losses, dtype=np.float64)
    out["own_rounding"], out["max_x"] = np.array(own), np.array(max_x)
    with torch.no_grad():
        out["predict_users"], out["predict_items"] = users[0], neg[0][:, 0]
        out["predict_scores"] = eng.model.predict(users[0], neg[0][:, 0]).numpy().copy()   # with the FINAL weights
    return out


def main():
    Engine = import_reference()
    fixture(Engine, "mix_concat_adam", "concat", 64, 3, 5, 2, None, None, "adam", 0.01, 31)
    fixture(Engine, "mix_mean_sgd_drop", "mean", 20, 2, 3, 1, 0.5, 0.1, "sgd", 0.05, 32, extra_cols=2)
    fixture(Engine, "mix_sum_rmsprop", "sum", 100, 1, 8, 3, None, 0.1, "rmsprop", 1e-3, 33)
    fixture(Engine, "mix_final_adam_hot", "final", 16, 4, 6, 2, 0.5, None, "adam", 0.01, 34, hot=True)
    fixture(Engine, "mix_rns_sgd", "concat", 12, 3, 1, 2, None, None, "sgd", 0.05, 35, ns="rns")


if __name__ == "__main__":
    main()
