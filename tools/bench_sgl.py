"""Measure the SGL training step on the GPU: the HIP engine against the same step written with torch autograd.

    python tools/bench_sgl.py [--repeats 5] [--out profiles/sgl_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sgl.py --hip-only --repeats 1 --shapes SHAPE   # kernel times
    python tools/bench_sgl.py --kernel-stats SHAPE=DIR/.../*_kernel_stats.csv[,...] --out profiles/sgl_step.json  # fold them in

Two shapes, both ``both_side`` with edge dropout (``aug_type`` 1, ``ssl_ratio`` 0.4), D 64, L 3, Adam:
  * ``ml100k_b1024``: the reference's default -- 943 x 1682, ~100k interactions, B 1024;
  * ``wide_b2048``: 50 000 x 20 000, ~2 M interactions, B 2048 -- here the ``[B, n_users]`` and ``[B, n_items]`` score
    matrices (573 MB between them, and autograd keeps several copies) dominate what torch does.
The yardstick is the reference's step (sgl.py:82-145, :188-226, :277-394 restated here in torch ops, nothing imported
from the reference) with ``backward()`` and ``torch.optim.Adam``, on the same GPU, with the sub-matrices already
resident on the device on both sides (the refresh is once per epoch and not part of a step).

A window is ``steps`` training steps on resident batches, timed with device events around the whole window; windows
of the two sides alternate ``--repeats`` times in one process after a warm-up of each side at the same shape, and the
median and the spread (max - min over the median) are reported.  ``steps`` is chosen per side so that a window lasts
about ``--min-window`` seconds.  Peak memory is ``torch.cuda.max_memory_allocated`` over a side's set-up, warm-up and
first window (every step allocates alike) minus what was allocated before that side was built; both sides allocate
through torch.  Needs a GPU: there is no CPU timing path.

Not measured: hardware counters, anything multi-GPU.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

D, L = 64, 3
REGS, SSL_REG, SSL_TEMP, SSL_RATIO, LR = 1e-5, 0.02, 0.5, 0.4, 0.05     # configs/sgl_default.json
#                 U      I      per_user  B
SHAPES = {"ml100k_b1024": (943, 1682, 106, 1024), "wide_b2048": (50_000, 20_000, 40, 2048)}


def interactions(U, I, per_user, seed=0):
    """Unique (user, item) pairs with skewed item popularity."""
    rng = np.random.default_rng(seed)
    pop = 1.0 / np.arange(1, I + 1) ** 0.8
    cdf = np.cumsum(pop / pop.sum())
    items = np.minimum(np.searchsorted(cdf, rng.random((U, 2 * per_user))), I - 1)
    users = np.repeat(np.arange(U), 2 * per_user)
    key = np.unique(users * I + items.reshape(-1))
    keep = np.sort(rng.permutation(key.size)[: U * per_user])
    key = key[keep]
    return key // I, key % I


def norm_adj(users, items, U, I):
    import scipy.sparse as sp

    N = U + I
    A = sp.csr_matrix((np.ones(users.size, dtype=np.float32), (users, items + U)), shape=(N, N))
    A = A + A.T
    d = np.power(np.asarray(A.sum(1)).flatten(), -0.5)
    d[np.isinf(d)] = 0.0
    return sp.diags(d).dot(A).dot(sp.diags(d)).tocsr().astype(np.float32)


def l2_rows(x):
    return x / torch.norm(x, 2, 1, keepdim=True)


class TorchSGL(torch.nn.Module):
    """The step of models/sgl.py (both_side) in torch ops, on whatever device it is moved to."""

    def __init__(self, U, I, adj, subs):
        super().__init__()
        self.U, self.I = U, I
        self.user_embedding = torch.nn.Parameter(torch.nn.init.xavier_uniform_(torch.empty(U, D)))
        self.item_embedding = torch.nn.Parameter(torch.nn.init.xavier_uniform_(torch.empty(I, D)))
        self.adj, self.subs = adj, subs

    def pooled(self, mat):
        e = torch.cat([self.user_embedding, self.item_embedding], dim=0)
        embs = [e]
        for _ in range(L):
            e = torch.sparse.mm(mat, e)
            embs.append(e)
        return torch.split(torch.stack(embs, 1).mean(dim=1), [self.U, self.I], 0)

    def forward(self, users, pos, neg):
        ua, ia = self.pooled(self.adj)
        ua1, ia1 = self.pooled(self.subs[0])
        ua2, ia2 = self.pooled(self.subs[1])
        ssl = 0.0
        for e1, e2, idx in ((ua1, ua2, users), (ia1, ia2, pos)):
            q, k_all = l2_rows(e1[idx]), l2_rows(e2)
            pos_score = (q * l2_rows(e2[idx])).sum(dim=1)
            ttl = torch.exp(torch.matmul(q, k_all.T) / SSL_TEMP).sum(dim=1)
            ssl = ssl - torch.log(torch.exp(pos_score / SSL_TEMP) / ttl).sum()
        u, p, n = ua[users], ia[pos], ia[neg]
        u0, p0, n0 = self.user_embedding[users], self.item_embedding[pos], self.item_embedding[neg]
        reg = (u0.pow(2).sum() + p0.pow(2).sum() + n0.pow(2).sum()) / 2
        bpr = -torch.log(torch.sigmoid((u * p).sum(-1) - (u * n).sum(-1))).sum()
        return bpr + REGS * reg + SSL_REG * ssl


def hip_engine(U, I, adj, B):
    import beta_recsys_amd as hp

    model = dict(n_users=U, n_items=I, emb_dim=D, n_layers=L, regs=REGS, ssl_reg=SSL_REG, ssl_temp=SSL_TEMP,
                 ssl_mode="both_side", ssl_ratio=SSL_RATIO, aug_type=1, is_subgraph=True, pretrain=0, norm_adj=adj,
                 optimizer="adam", lr=LR, device_str="cuda:0", batch_size=B, sub_rng="device", sub_seed=1)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.SGLEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_bench_runs"}})
    eng.model.train()
    return eng


def sparse_of(sub, view, N):
    """One view of a SubMats handle as a coalesced torch sparse COO tensor on its device (what the reference builds),
    dropped edges removed."""
    val = sub.vals[view][0][: sub.nnz]
    rows = torch.repeat_interleave(torch.arange(N, device=val.device), sub.rowptr[1:] - sub.rowptr[:-1])
    on = val != 0
    return torch.sparse_coo_tensor(torch.stack([rows[on], sub.col[on].to(torch.int64)]), val[on], (N, N)).coalesce()


def timed_window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn(steps)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps          # us per step


def run_shape(name, args, dev):
    U, I, per_user, B = SHAPES[name]
    N = U + I
    users, items = interactions(U, I, per_user)
    adj = norm_adj(users, items, U, I)
    rng = np.random.default_rng(B)
    n_batches = 8
    pick = rng.integers(0, users.size, (n_batches, B))
    batches = [(torch.from_numpy(users[p]).to(dev), torch.from_numpy(items[p]).to(dev),
                torch.from_numpy(rng.integers(0, I, B)).to(dev)) for p in pick]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    eng = hip_engine(U, I, adj, B)
    loader = types.SimpleNamespace(dataset=types.SimpleNamespace(user_tensor=torch.from_numpy(users),
                                                                 pos_item_tensor=torch.from_numpy(items)))
    sub = eng.sub_mat_refresher(loader)
    eng._sub = sub

    def hip_steps(n):
        for s in range(n):
            eng._enqueue_step(batches[s % n_batches])

    sides = {"hip": hip_steps}
    peaks, times, steps = {}, {"hip": []}, {}
    hip_steps(args.warmup)
    steps["hip"] = max(args.warmup, int(args.min_window * 1e6 / timed_window(hip_steps, args.warmup)))
    torch.cuda.synchronize()
    peaks["hip"] = torch.cuda.max_memory_allocated() - base
    hip_resident = torch.cuda.memory_allocated() - base
    if not args.hip_only:
        base_t = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        torch.manual_seed(0)
        coo = adj.tocoo()
        adj_t = torch.sparse_coo_tensor(torch.from_numpy(np.vstack([coo.row, coo.col]).astype(np.int64)),
                                        torch.from_numpy(coo.data), (N, N)).coalesce().to(dev)
        ref = TorchSGL(U, I, adj_t, [sparse_of(sub, 0, N), sparse_of(sub, 1, N)]).to(dev)
        eng.model.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()})
        opt = torch.optim.Adam(ref.parameters(), lr=LR)

        def torch_steps(n):
            for s in range(n):
                opt.zero_grad()
                ref(*batches[s % n_batches]).backward()
                opt.step()

        sides["torch"] = torch_steps
        times["torch"] = []
        torch_steps(max(2, args.warmup // 4))
        steps["torch"] = max(2, int(args.min_window * 1e6 / timed_window(torch_steps, 2)))
        torch.cuda.synchronize()
        peaks["torch"] = torch.cuda.max_memory_allocated() - base_t
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(timed_window(fn, steps[k]))
    st = eng._sync_stats()
    out = {"n_users": U, "n_items": I, "interactions": int(users.size), "nnz_norm_adj": int(adj.nnz), "emb_dim": D,
           "n_layers": L, "batch": B, "ssl_mode": "both_side", "aug_type": 1, "ssl_ratio": SSL_RATIO, "ssl_temp": SSL_TEMP,
           "optimizer": "adam", "repeats": args.repeats, "steps_per_window": steps,
           "score_matrices_bytes": 4 * B * (U + I), "hip_resident_bytes": int(hip_resident), "last_loss_hip": st.loss,
           "last_parts_hip": list(eng.last_losses())}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 1) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
        out[f"{k}_peak_bytes"] = int(peaks[k])
    if "torch" in times:
        out["speedup_vs_torch_autograd"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
        out["hip_beats_torch_beyond_spread"] = bool(max(times["hip"]) < min(times["torch"]))
        out["peak_bytes_saved"] = int(peaks["torch"] - peaks["hip"])
        out["saves_at_least_the_score_matrices"] = bool(peaks["torch"] - peaks["hip"] >= out["score_matrices_bytes"])
    out["not_measured"] = ["hardware counters", "multi-GPU"]
    return out


def merge_kernel_stats(spec, path):
    """``name=csv[,name=csv]``: rocprofv3's kernel statistics of a ``--hip-only`` run of one shape, as
    ``kernel_share_percent`` (every kernel above 0.5 %) and ``kernel_us_per_call`` of that shape in the profile at
    ``path``."""
    import csv

    with open(path) as f:
        out = json.load(f)
    for item in spec.split(","):
        name, csv_path = item.split("=", 1)
        with open(csv_path, newline="") as f:
            rows = list(csv.DictReader(f))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        share, per_call = {}, {}
        for r in rows:
            short = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1]
            share[short] = share.get(short, 0.0) + 100.0 * float(r["TotalDurationNs"]) / total
            per_call[short] = round(float(r["AverageNs"]) / 1e3, 1)
        top = [k for k, v in sorted(share.items(), key=lambda kv: -kv[1]) if v >= 0.5]
        out["shapes"][name]["kernel_share_percent"] = {k: round(share[k], 1) for k in top}
        out["shapes"][name]["kernel_us_per_call"] = {k: per_call[k] for k in top}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--kernel-stats", default=None, help="shape=kernel_stats.csv[,...]: merge into --out and exit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.kernel_stats, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_sgl.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__

    dev = torch.device("cuda:0")
    result = {"tool": "tools/bench_sgl.py", "device": torch.cuda.get_device_name(0),
              "source_hash": __graft_entry__.source_hash(), "shapes": {}}
    for name in args.shapes.split(","):
        result["shapes"][name] = run_shape(name, args, dev)
        print(json.dumps({name: result["shapes"][name]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
