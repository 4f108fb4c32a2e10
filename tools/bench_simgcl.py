"""Measure the SimGCL training step on the GPU: the HIP engine against the reference's step written in torch autograd.

    python tools/bench_simgcl.py [--repeats 5] [--out profiles/simgcl_step.json]

Two shapes, Adam, the reference's default hyper-parameters (eps 0.1, reg 1e-4, lambda 0.5, temperature 0.2):
  * ``ml100k``: 943 x 1682, D 64, B 1000, L 2 (configs/simgcl_default.json on ml-100k), 100 000 interactions;
  * ``ml1m``: 6040 x 3706, D 64, B 4096, L 3, 1 000 000 interactions.
The interactions are random with Zipf item degrees; the graph is D^-1/2 A D^-1/2.  The yardstick is the reference's step
(simgcl.py:25-70, :101-163 restated here in torch ops: three forwards of ``torch.sparse.mm`` hops with ``rand_like``
noise, ``torch.unique``, the two InfoNCE terms, BPR and the norms; nothing imported from the reference) with
``backward()`` and ``torch.optim.Adam``, on the same GPU.

A window is ``steps`` training steps on resident batches, timed with device events around the whole window; windows of
the two sides alternate ``--repeats`` times in one process after a warm-up of each side at the same shape, and the
median and the spread (max - min over the median) are reported.  ``steps`` is chosen per side so that a window lasts
about ``--min-window`` seconds.  Peak memory is ``torch.cuda.max_memory_allocated`` over a side's set-up, warm-up and
first window minus what was allocated before that side was built; both sides allocate through torch.  ``kernel_shares``
is the share of the device time of a few HIP steps per kernel name, from ``torch.profiler`` (None where the profiler
gives no device events).  Needs a GPU.

Not measured: hardware counters, anything multi-GPU.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

EPS, REG, LAMBDA, TEMP, LR = 0.1, 1e-4, 0.5, 0.2, 0.001
#            U     I     D   L  B     interactions
SHAPES = {"ml100k": (943, 1682, 64, 2, 1000, 100_000), "ml1m": (6040, 3706, 64, 3, 4096, 1_000_000)}


def random_graph(U, I, n, rng):
    pop = 1.0 / np.arange(1, I + 1) ** 0.8
    key = np.unique(rng.integers(0, U, n).astype(np.int64) * I + rng.choice(I, size=n, p=pop / pop.sum()))
    users, items = key // I, key % I
    N = U + I
    a = sp.csr_matrix((np.ones(users.size, dtype=np.float32), (users, items + U)), shape=(N, N))
    a = a + a.T
    with np.errstate(divide="ignore"):
        d = np.power(np.asarray(a.sum(1)).flatten(), -0.5)
    d[np.isinf(d)] = 0.0
    return users, items, sp.diags(d).dot(a).dot(sp.diags(d)).tocsr().astype(np.float32)


class TorchSimGCL(torch.nn.Module):
    """The step of models/simgcl.py in torch ops, on whatever device it is moved to."""

    def __init__(self, U, I, D, L, adj):
        super().__init__()
        self.U, self.I, self.L, self.adj = U, I, L, adj
        self.user_embedding = torch.nn.Embedding(U, D)
        self.item_embedding = torch.nn.Embedding(I, D)

    def views(self, perturbed):
        e = torch.cat((self.user_embedding.weight, self.item_embedding.weight), dim=0)
        hops = []
        for _ in range(self.L):
            e = torch.sparse.mm(self.adj, e)
            if perturbed:
                e = e + torch.sign(e) * F.normalize(torch.rand_like(e), dim=-1) * EPS
            hops.append(e)
        return torch.split(torch.mean(torch.stack(hops, dim=1), dim=1), [self.U, self.I])

    @staticmethod
    def info_nce(a, b):
        pos = torch.exp((a * b).sum(dim=-1) / TEMP)
        ttl = torch.exp(torch.matmul(a, b.transpose(0, 1)) / TEMP).sum(dim=1)
        return -torch.log(pos / ttl).sum()

    def forward(self, users, pos, neg):
        ru, ri = self.views(False)
        u, p, n = ru[users], ri[pos], ri[neg]
        loss = -torch.log(1e-7 + torch.sigmoid((u * p).sum(1) - (u * n).sum(1))).sum()
        loss = loss + REG * (torch.norm(u, p=2) + torch.norm(p, p=2) + torch.norm(n, p=2))
        uu, ii = torch.unique(users), torch.unique(pos)
        u1, i1 = (F.normalize(x, dim=1) for x in self.views(True))
        _, i2 = self.views(True)
        u2, i2 = F.normalize(u1, dim=1), F.normalize(i2, dim=1)
        return loss + LAMBDA * (self.info_nce(u1[uu], u2[uu]) + self.info_nce(i1[ii], i2[ii]))


def timed_window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn(steps)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps          # us per step


def kernel_shares(fn, steps=20):
    """{kernel name: share of the device time} of ``steps`` steps, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(steps)
            torch.cuda.synchronize()
        rows = {}
        for e in prof.key_averages():
            t = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0) or 0.0)
            if t > 0 and ("kernel" in e.key or "Memcpy" in e.key or "Memset" in e.key or "hiprec" in e.key):
                rows[e.key.split("(")[0][:80]] = rows.get(e.key.split("(")[0][:80], 0.0) + t
        total = sum(rows.values())
        if total <= 0:
            return None
        return {k: round(v / total, 4) for k, v in sorted(rows.items(), key=lambda kv: -kv[1])}
    except Exception as exc:       # the profiler is an extra: the timing stands without it
        return {"unavailable": str(exc)[:200]}


def run_shape(name, args, dev):
    import beta_recsys_amd as hp

    U, I, D, L, B, n_inter = SHAPES[name]
    rng = np.random.default_rng(B)
    users, items, adj = random_graph(U, I, n_inter, rng)
    n_batches = 8
    picks = [rng.integers(0, users.size, B) for _ in range(n_batches)]
    batches = [(torch.from_numpy(users[p]).to(dev), torch.from_numpy(items[p]).to(dev),
                torch.from_numpy(rng.integers(0, I, B)).to(dev)) for p in picks]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    torch.manual_seed(0)
    model = dict(n_users=U, n_items=I, emb_dim=D, n_layer=L, eps=EPS, reg=REG, norm_adj=adj, optimizer="adam", lr=LR,
                 device_str="cuda:0", batch_size=B, cl_temp=TEMP)
    model["lambda"] = LAMBDA
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.SimGCLEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_bench_runs"}})
    eng.model.train()
    eng._setup()

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
        coo = adj.tocoo()
        tadj = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]).astype(np.int64), coo.data, (U + I, U + I)).coalesce().to(dev)
        ref = TorchSimGCL(U, I, D, L, tadj).to(dev)
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
    n_uniq = [int(np.mean([np.unique(users[p]).size for p in picks])), int(np.mean([np.unique(items[p]).size for p in picks]))]
    out = {"n_users": U, "n_items": I, "nnz": int(adj.nnz), "emb_dim": D, "n_layer": L, "batch": B, "optimizer": "adam",
           "mean_unique_users_items": n_uniq, "repeats": args.repeats, "steps_per_window": steps,
           "spmm_per_step": {"forward": 1 + 3 * (L - 1), "backward": L, "reference": 6 * L},
           "workspace_bytes": int(eng.model._ws["ws"].numel() * 4), "hip_resident_bytes": int(hip_resident),
           "last_loss_hip": st.loss, "last_parts_hip": list(eng.last_losses())}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 1) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
        out[f"{k}_peak_bytes"] = int(peaks[k])
    if "torch" in times:
        out["speedup_vs_torch"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
        out["hip_beats_torch_beyond_spread"] = bool(max(times["hip"]) < min(times["torch"]))
        out["peak_bytes_saved"] = int(peaks["torch"] - peaks["hip"])
    out["kernel_shares"] = None if args.no_shares else kernel_shares(hip_steps)
    out["not_measured"] = ["hardware counters", "multi-GPU"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side")
    ap.add_argument("--no-shares", action="store_true", help="skip the per-kernel shares")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_simgcl.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__

    dev = torch.device("cuda:0")
    result = {"tool": "tools/bench_simgcl.py", "device": torch.cuda.get_device_name(0),
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
