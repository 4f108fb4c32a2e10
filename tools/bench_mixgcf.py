"""Measure the MixGCF training step on the GPU: the HIP engine against the same step written with torch autograd.

    python tools/bench_mixgcf.py [--steps 1000] [--warmup 100] [--repeats 5] [--out profiles/mixgcf_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_mixgcf.py --hip-only --repeats 1 --steps 50 --shapes SHAPE   # kernel times

Two shapes on ML-100K-sized tables (943 x 1682, ~100k interactions, D 64, L 3, K 1, pool mean, no dropout): the
reference's default shape (B 400, n_negs 2) and the shape its example script defaults to (B 2048, n_negs 64).  A window
is ``--steps`` training steps on resident batches between two device synchronisations (0.15 s of HIP steps, 3 s of torch
steps at the default), after ``--warmup`` steps of each side at the same shape; HIP and torch windows alternate
``--repeats`` times in one process, so both see the same machine state; the median and the spread (max - min over the
median) of the windows are reported.  There is no parent number for a new model and the reference's own step never
trains, so the yardstick is that step (sparse.mm hops, gather, mix, argmax, K-pair softplus: models/mixgcf.py:46-67,
:176-286 restated here, nothing imported from the reference) with ``backward()`` and Adam added, on the same GPU, with
the mixing seeds drawn on the device on both sides.  Needs a GPU: there is no CPU timing path.

Byte model printed with the result: the sampler gathers B (2 + K n_negs) (L + 1) rows of 4 D bytes per step from hop
tables of (L + 1) N 4 D bytes in all (they fit L2), and adds B (2 + K) (L + 1) rows by float atomics.  The gather rate is
only derived when ``--kernel-us`` hands in the sampler kernel's time from a kernel trace taken in a run of its own.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U, I, D, L, K = 943, 1682, 64, 3, 1
SHAPES = {"default_b400_n2": (400, 2), "example_b2048_n64": (2048, 64)}
L2_DECAY, LR = 1e-4, 1e-3


def graph(seed=0, per_user=106):
    """D^-1 (A + I) of ~100k interactions with skewed item popularity, as a torch sparse COO tensor."""
    rng = np.random.default_rng(seed)
    pop = 1.0 / np.arange(1, I + 1) ** 0.8
    pop /= pop.sum()
    items = np.concatenate([rng.choice(I, per_user, replace=False, p=pop) for _ in range(U)])
    users = np.repeat(np.arange(U), per_user)
    N = U + I
    rows = np.concatenate([users, U + items, np.arange(N)])
    cols = np.concatenate([U + items, users, np.arange(N)])
    vals = (1.0 / np.bincount(rows, minlength=N)[rows]).astype(np.float32)
    adj = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([rows, cols])), torch.from_numpy(vals), (N, N)).coalesce()
    return users, items, adj


class TorchMixGCF(torch.nn.Module):
    """The step of models/mixgcf.py (pool mean, no dropout) in torch ops, on whatever device it is moved to."""

    def __init__(self, adj, n_negs):
        super().__init__()
        self.user_embedding = torch.nn.Embedding(U, D)
        self.item_embedding = torch.nn.Embedding(I, D)
        self.adj, self.n_negs = adj, n_negs

    def forward(self, users, pos, neg, seeds):
        e = torch.cat([self.user_embedding.weight, self.item_embedding.weight], dim=0)
        embs = [e]
        for _ in range(L):
            e = torch.sparse.mm(self.adj, e)
            embs.append(e)
        embs = torch.stack(embs, dim=1)
        ue, ie = embs[:U], embs[U:]
        B = users.shape[0]
        s_e, p_e = ue[users], ie[pos]
        negs = []
        for k in range(K):
            n_e = ie[neg[:, k * self.n_negs:(k + 1) * self.n_negs]]
            sd = seeds[:, k].view(B, 1, L + 1, 1)
            n_mix = sd * p_e.unsqueeze(1) + (1 - sd) * n_e
            scores = (s_e.mean(dim=1).view(B, 1, 1, D) * n_mix).sum(dim=-1)
            idx = torch.max(scores, dim=1)[1].detach()
            negs.append(n_mix.permute(0, 2, 1, 3)[torch.arange(B, device=idx.device)[:, None],
                                                  torch.arange(L + 1, device=idx.device)[None, :], idx])
        n_sel = torch.stack(negs, dim=1)                                   # [B, K, L + 1, D]
        u_p, p_p, n_p = s_e.mean(dim=1), p_e.mean(dim=1), n_sel.mean(dim=2)
        x = (u_p.unsqueeze(1) * n_p).sum(dim=-1) - (u_p * p_p).sum(dim=-1, keepdim=True)
        mf = torch.log(1 + torch.exp(x).sum(dim=1)).mean()
        reg = (s_e[:, 0].norm() ** 2 + p_e[:, 0].norm() ** 2 + n_sel[:, :, 0].norm() ** 2) / 2
        return mf + L2_DECAY * reg / B


def hip_engine(adj, n_negs, B, w0):
    import beta_recsys_amd as hp

    model = dict(n_users=U, n_items=I, emb_dim=D, pool="mean", context_hops=L, mess_dropout=False, mess_dropout_rate=0.1,
                 edge_dropout=False, edge_dropout_rate=0.5, norm_adj=adj, l2=L2_DECAY, n_negs=n_negs, ns="mixgcf", K=K,
                 optimizer="adam", lr=LR, device_str="cuda:0", batch_size=B, seed_rng="device", dropout_rng="device")
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.MixGCFEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_bench_runs"}})
    eng.model.load_state_dict(w0)
    eng.model.train()
    return eng


def run_shape(name, B, n_negs, args, users, items, adj, dev):
    rng = np.random.default_rng(B)
    n_batches = 8
    pick = rng.integers(0, len(users), (n_batches, B))
    batches = [(torch.from_numpy(users[p]).to(dev), torch.from_numpy(items[p]).to(dev),
                torch.from_numpy(rng.integers(0, I, (B, K * n_negs))).to(dev)) for p in pick]
    torch.manual_seed(0)
    ref = TorchMixGCF(adj.to(dev), n_negs)
    w0 = {"user_embedding.weight": ref.user_embedding.weight.detach().clone() * 0.3,
          "item_embedding.weight": ref.item_embedding.weight.detach().clone() * 0.3}
    ref.load_state_dict(w0)
    ref.to(dev)
    opt = torch.optim.Adam(ref.parameters(), lr=LR)
    eng = hip_engine(adj, n_negs, B, w0)

    def hip_steps(n=None):
        for s in range(n or args.steps):
            eng._enqueue_step(batches[s % n_batches])

    def torch_steps(n=None):
        for s in range(n or args.steps):
            u, p, n = batches[s % n_batches]
            opt.zero_grad()
            loss = ref(u, p, n, torch.rand(B, K, L + 1, device=dev))
            loss.backward()
            opt.step()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e6   # us per step

    sides = {"hip": hip_steps} if args.hip_only else {"hip": hip_steps, "torch": torch_steps}
    for fn in sides.values():
        fn(args.warmup)
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn))
    st = eng._sync_stats()
    H, N = L + 1, U + I
    out = {"shape": name, "n_users": U, "n_items": I, "nnz": int(adj._nnz()), "emb_dim": D, "context_hops": L, "batch": B,
           "n_negs": n_negs, "K": K, "pool": "mean", "optimizer": "adam", "steps_per_window": args.steps,
           "repeats": args.repeats, "hop_tables_bytes": H * N * D * 4,
           "sampler_gather_bytes_per_step": B * (2 + K * n_negs) * H * D * 4,
           "atomic_bytes_per_step": B * (2 + K) * H * D * 4, "last_loss_hip": st.loss}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 2) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 2)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
    if "torch" in times:
        out["speedup_vs_torch_autograd"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
        out["hip_beats_torch_beyond_spread"] = bool(max(times["hip"]) < min(times["torch"]))
    kernel_us = (args.kernel_us or {}).get(name)
    if kernel_us:
        out["sampler_kernel_us"] = kernel_us
        out["sampler_gather_GBps"] = round(out["sampler_gather_bytes_per_step"] / kernel_us / 1e3, 1)
    else:
        out["not_measured"] = ["sampler kernel time (kernel trace, a run of its own)", "sampler gather rate"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--kernel-us", type=json.loads, default=None,
                    help='{"shape": us} mean time of mixgcf_loss_kernel per launch, from a kernel trace of another run')
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mixgcf.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__

    dev = torch.device("cuda:0")
    users, items, adj = graph()
    result = {"tool": "tools/bench_mixgcf.py", "device": torch.cuda.get_device_name(0),
              "source_hash": __graft_entry__.source_hash(), "shapes": []}
    for name in args.shapes.split(","):
        B, n_negs = SHAPES[name]
        result["shapes"].append(run_shape(name, B, n_negs, args, users, items, adj, dev))
        print(json.dumps(result["shapes"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
