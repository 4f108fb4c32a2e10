"""Measure the SR-GNN training step on the GPU: the HIP engine against the same step written as torch ops.

    python tools/bench_srgnn.py [--steps 8] [--windows 4] [--warmup 2] [--repeats 3] [--out profiles/srgnn_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_srgnn.py --hip-only --repeats 1 --shapes diginetica
    python tools/bench_srgnn.py --merge profiles/srgnn_step.json --kernel-stats diginetica=DIR/..._results.db

Shapes (Adam lr 1e-3, l2 1e-5, hybrid):
  diginetica   B 100, H 100, step 1, 43 097 items, ragged lengths (geometric, mean about 5, one session of 69)
  b512         B 512, H 128, step 2, 43 097 items, the same length law capped at 40
``--steps`` batches of synthetic sessions (ids drawn from a pool of 2 x length per session, so sessions revisit items)
are built on the host once.  A window is ``--windows`` passes over them between two device synchronisations; the sides
alternate ``--repeats`` times in one process, so both see the same machine state.  Both sides are handed HOST arrays at
every step and upload them, as a loader's batches arrive.  Sides:
  hip     SRGNNEngine's launches (hiprec_srgnn_grad, which builds the session graphs on the device, + the dense optimizer
          sweep), python-looped, no host sync
  torch   the step as the published code writes it: the dense adjacency ``A [B, n, 2n]``, node ids and alias are built in
          numpy OUTSIDE the timed window (the published loader does that work per batch on the host; it is left out here,
          which favours this side), then ``torch.matmul`` with autograd and ``torch.optim.Adam(weight_decay=l2)``, no host
          sync either
Peak memory is each side's own: ``torch.cuda.max_memory_allocated`` over the side's construction and its first steps,
less what was allocated before (the engine's workspace comes from the same allocator).  Before anything is timed both
sides compute the first batch's loss from the same weights; the two values are recorded and the tool stops if they differ
by more than 1e-4 relative.  ``--kernel-stats`` folds the kernel shares of a rocprofv3 ``--hip-only`` run of one shape
into an existing result file.  There is no earlier number for this model.  Needs a GPU.
"""
import argparse
import contextlib
import csv
import io
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_NODE, LR, L2 = 43098, 1e-3, 1e-5
SHAPES = {"diginetica": dict(B=100, H=100, step=1, max_len=69), "b512": dict(B=512, H=128, step=2, max_len=40)}


def host_batches(steps, B, max_len, seed=1):
    """``[(seq [T, B], target [B], lens [B])]`` as numpy int64; the first session of the first batch has ``max_len``."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(steps):
        lens = np.minimum(rng.geometric(1.0 / 5.0, B), max_len)
        if t == 0:
            lens[0] = max_len
        lens = np.sort(lens)[::-1].copy()
        seq = np.zeros((int(lens[0]), B), dtype=np.int64)
        for b, n in enumerate(lens):
            pool = rng.integers(1, N_NODE, 2 * int(n))
            seq[:n, b] = pool[rng.integers(0, pool.size, int(n))]
        out.append((seq, rng.integers(1, N_NODE, B), lens.astype(np.int64)))
    return out


def dense_inputs(seq, lens):
    """The published loader's per-batch arrays: ``items [B, n]``, ``A [B, n, 2n]`` float32, ``alias [B, T]``,
    ``mask [B, T]``."""
    T, B = seq.shape
    nodes = [np.unique(seq[:lens[b], b]) for b in range(B)]
    n = max(len(x) for x in nodes)
    items = np.zeros((B, n), dtype=np.int64)
    A = np.zeros((B, n, 2 * n), dtype=np.float32)
    alias = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        k = len(nodes[b])
        items[b, :k] = nodes[b]
        al = np.searchsorted(nodes[b], seq[:lens[b], b])
        alias[b, :lens[b]] = al
        u_A = np.zeros((n, n), dtype=np.float32)
        u_A[al[:-1], al[1:]] = 1
        s_in = u_A.sum(0)
        s_in[s_in == 0] = 1
        s_out = u_A.sum(1)
        s_out[s_out == 0] = 1
        A[b] = np.concatenate([(u_A / s_in).T, (u_A.T / s_out).T], axis=1)
    mask = (np.arange(T)[None, :] < lens[:, None]).astype(np.float32)
    return items, A, alias, mask


class TorchSRGNN(torch.nn.Module):
    """The step of include/hiprec.h's SR-GNN block as torch ops; parameters keyed like the engine's state_dict."""

    def __init__(self, w, step):
        super().__init__()
        self.names = list(w)
        self.params = torch.nn.ParameterList(torch.nn.Parameter(v.clone()) for v in w.values())
        self.step = step

    def forward(self, items, A, alias, mask, lens, target):
        w = dict(zip(self.names, self.params))
        n = items.shape[1]
        h = w["embedding.weight"][items]
        for _ in range(self.step):
            a_in = torch.matmul(A[:, :, :n], F.linear(h, w["gnn.linear_edge_in.weight"], w["gnn.linear_edge_in.bias"]))
            a_out = torch.matmul(A[:, :, n:], F.linear(h, w["gnn.linear_edge_out.weight"], w["gnn.linear_edge_out.bias"]))
            inputs = torch.cat([a_in + w["gnn.b_iah"], a_out + w["gnn.b_oah"]], 2)
            i_r, i_z, i_n = F.linear(inputs, w["gnn.w_ih"], w["gnn.b_ih"]).chunk(3, 2)
            h_r, h_z, h_n = F.linear(h, w["gnn.w_hh"], w["gnn.b_hh"]).chunk(3, 2)
            r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
            ng = torch.tanh(i_n + r * h_n)
            h = ng + z * (h - ng)
        B = items.shape[0]
        x = h[torch.arange(B, device=h.device)[:, None], alias]
        ht = x[torch.arange(B, device=h.device), lens - 1]
        q1 = F.linear(ht, w["linear_one.weight"], w["linear_one.bias"])[:, None, :]
        q2 = F.linear(x, w["linear_two.weight"], w["linear_two.bias"])
        alpha = F.linear(torch.sigmoid(q1 + q2), w["linear_three.weight"])
        s_g = (alpha * x * mask[:, :, None]).sum(1)
        a = F.linear(torch.cat([s_g, ht], 1), w["linear_transform.weight"], w["linear_transform.bias"])
        return F.cross_entropy(a @ w["embedding.weight"][1:].T, target - 1)


def measure(name, B, H, step, max_len, args, hp, dev):
    torch.manual_seed(0)
    cfg = {"model": {"hidden_size": H, "step": step, "nonhybrid": False, "batch_size": B, "lr": LR, "l2": L2,
                     "optimizer": "adam", "device_str": "cuda:0"},
           "dataset": {"n_node": N_NODE}, "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    batches = host_batches(args.steps, B, max_len)
    torch.cuda.synchronize()
    peaks = {}

    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.SRGNNEngine(cfg)
    w0 = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
    first_loss = {"hip": float(eng.backward_only(batches[0])[0])}      # the loss excludes the l2 term
    eng.load_optimizer_state(0)

    def hip():
        for b in batches:
            eng._enqueue_step(b)

    hip()
    torch.cuda.synchronize()
    peaks["hip"] = torch.cuda.max_memory_allocated() - base
    sides = {"hip": hip}
    if not args.hip_only:
        dense = [dense_inputs(seq, lens) + (lens, target) for seq, target, lens in batches]      # not timed
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ref = TorchSRGNN({k: v.to(dev) for k, v in w0.items()}, step).to(dev)
        opt = torch.optim.Adam(ref.parameters(), lr=LR, weight_decay=L2)
        with torch.no_grad():
            first_loss["torch"] = float(ref(*(torch.from_numpy(a).to(dev) for a in dense[0])))
        if abs(first_loss["torch"] - first_loss["hip"]) > 1e-4 * abs(first_loss["torch"]):
            raise SystemExit(f"{name}: the two sides do not compute the same loss from the same weights: {first_loss}")

        def torch_steps():
            for d in dense:
                opt.zero_grad()
                ref(*(torch.from_numpy(a).to(dev) for a in d)).backward()
                opt.step()

        torch_steps()
        torch.cuda.synchronize()
        peaks["torch"] = torch.cuda.max_memory_allocated() - base
        sides["torch"] = torch_steps

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.windows):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (args.windows * len(batches)) * 1e6   # us per step

    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn))
    st = eng._sync_stats()
    lens_all = np.concatenate([b[2] for b in batches])
    out = {"batch": B, "hidden_size": H, "step": step, "mean_length": round(float(lens_all.mean()), 2),
           "max_length": int(lens_all.max()), "rows_per_step": round(float(lens_all.sum()) / len(batches), 1),
           "last_loss_hip": st.loss,
           "first_step_loss": first_loss,      # both sides from the same initial weights; they must agree to 1e-4
           # hiprec_srgnn_grad's kernels (DESIGN 3.32 lists them; two memsets beside them), then the optimizer sweep
           "launches_per_step_derived": 20 + 8 * step + 1,
           "workspace_mb": round(eng.model._ws.numel() / 1e6, 1)}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 1) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
        out[f"{k}_peak_memory_mb"] = round(peaks[k] / 1e6, 1)
    if "torch" in times:
        out["hip_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
    del eng
    torch.cuda.empty_cache()
    return out


def kernel_shares(path, top=12):
    """``[{kernel, calls, share}]`` of a rocprofv3 ``--kernel-trace --stats`` run, the largest first: its
    ``*_kernel_stats.csv``, or the ``top_kernels`` view of its ``*_results.db``."""
    if path.endswith(".db"):
        import sqlite3

        with contextlib.closing(sqlite3.connect(path)) as db:
            rows = [(n, int(c), float(d)) for n, c, d in db.execute("select name, total_calls, total_duration from top_kernels")]
    else:
        with open(path, newline="") as f:
            rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(f)]
    total = sum(r[2] for r in rows) or 1.0
    rows.sort(key=lambda r: -r[2])
    short = lambda n: n.replace("(anonymous namespace)::", "").split("(")[0].split("::")[-1][-60:]      # noqa: E731
    return [{"kernel": short(n), "calls": c, "share": round(d / total, 4)} for n, c, d in rows[:top]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", default=None, help="an existing result file to fold --kernel-stats into")
    ap.add_argument("--kernel-stats", action="append", default=[], metavar="SHAPE=CSV_OR_DB")
    args = ap.parse_args()
    if args.merge:
        with open(args.merge) as f:
            out = json.load(f)
        for item in args.kernel_stats:
            shape, path = item.split("=", 1)
            out["shapes"][shape]["hip_kernel_shares"] = kernel_shares(path)
        with open(args.merge, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        return
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_srgnn.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_srgnn.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "n_node": N_NODE, "optimizer": "adam", "l2": L2,
           "steps_per_window": args.windows * args.steps, "repeats": args.repeats, "shapes": {}}
    for name in args.shapes.split(","):
        out["shapes"][name] = measure(name, args=args, hp=hp, dev=dev, **SHAPES[name])
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
