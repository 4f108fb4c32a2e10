"""Measure SLIM's ``prepare_model`` on the GPU at a MovieLens-1M-like shape, next to the same schedule written as torch
ops on the same card.

    python tools/bench_slim.py [--repeats 5] [--warmup 1] [--out profiles/slim.json]

Shape: 6040 users x 3706 items, about 1 M pairs (tools/bench_knn.py's synthetic log), l1 = l2 = 1, tol 1e-5, at most 100
sweeps (the model's defaults).

Device side, HIP events around each stage, the median over ``--repeats`` after ``--warmup`` runs:
  * ``gram``     hiprec_ease_gram: A = X^T X + l2 I by integer counting;
  * ``solve``    hiprec_slim_fit: every column by cyclic coordinate descent, one workgroup per column;
  * ``prepare_model``  the whole call, wall clock between two synchronisations: the two CSRs (torch), both stages, the
                 read-back of the status word, the sweep counts and nnz;
  * ``recommend``  4096 query users, top 10 under the training frame's seen mask;
with the sweep histogram, nnz, the number of unconverged columns and the peak device memory of ``prepare_model``
(torch.cuda.max_memory_allocated, reset before it).

Yardstick: the only one there is -- the same schedule as torch ops, all columns advancing together one coordinate at a
time (the rank-1 form of tests/slim_numpy.py), for ``--torch-sweeps`` sweeps with ``tol = 0``; the kernel is timed again
under the same stopping rule (``max_sweeps = --torch-sweeps``, ``tol = 0``) and both results are compared.

Needs a GPU: there is no CPU timing path.
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_knn import N_ITEMS, N_USERS, synthetic_log  # noqa: E402


def summary(ms):
    return {"ms": [round(x, 4) for x in ms], "ms_median": round(float(np.median(ms)), 4),
            "ms_spread": round(max(ms) - min(ms), 4)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def torch_sweeps(A, l1, sweeps):
    """``sweeps`` sweeps of the positive-mode schedule on every column at once: row ``j`` of ``WT`` / ``QT`` is column
    ``j`` of ``W`` / ``A W``; coordinate ``k`` of all columns is one elementwise step and one rank-1 update."""
    n = A.shape[0]
    WT = torch.zeros_like(A)
    QT = torch.zeros_like(A)
    diag = A.diagonal().clone()
    for _ in range(sweeps):
        for k in range(n):
            wk = WT[:, k]
            t = wk - ((QT[:, k] - A[k]) + l1) / diag[k]
            d = torch.clamp_min(t, 0.0) - wk
            d[k] = 0.0
            QT.addr_(d, A[k])
            wk.add_(d)
    return WT.t().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--l1", type=float, default=1.0)
    ap.add_argument("--l2", type=float, default=1.0)
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--max-sweeps", type=int, default=100)
    ap.add_argument("--torch-sweeps", type=int, default=2)
    ap.add_argument("--hip-only", action="store_true", help="skip the torch yardstick")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_slim.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp
    from beta_recsys_amd._stats import clear_status

    warnings.simplefilter("ignore", RuntimeWarning)          # unconverged columns are counted below
    dev = torch.device("cuda:0")
    users, items = synthetic_log()
    users_d, items_d = torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev)
    n = N_ITEMS
    cfg = dict(n_users=N_USERS, n_items=n, l1_reg=args.l1, l2_reg=args.l2, tol=args.tol, max_sweeps=args.max_sweeps,
               device_str="cuda:0")
    result = {"tool": "tools/bench_slim.py", "device": torch.cuda.get_device_name(0),
              "source_hash": __graft_entry__.source_hash(), "n_users": N_USERS, "n_items": n,
              "n_interactions": int(users.size), "l1": args.l1, "l2": args.l2, "tol": args.tol,
              "max_sweeps": args.max_sweeps, "repeats": args.repeats, "warmup": args.warmup,
              "lds_bytes_per_block": 2 * 4 * n, "blocks": n, "threads_per_block": 256}
    model = hp.SLIM(cfg)

    whole = []
    for it in range(args.warmup + args.repeats):
        torch.cuda.reset_peak_memory_stats(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.prepare_model((users_d, items_d))
        torch.cuda.synchronize()
        if it >= args.warmup:
            whole.append((time.perf_counter() - t0) * 1e3)
    result["prepare_model"] = dict(summary(whole), peak_device_bytes=int(torch.cuda.max_memory_allocated(dev)))
    result["distinct_pairs"] = int(model._b[1].numel())
    sweeps = model.sweeps.cpu().numpy()
    edges = [1, 2, 3, 5, 9, 17, 33, 65, args.max_sweeps + 1]
    edges = sorted({e for e in edges if e <= args.max_sweeps + 1})
    hist, _ = np.histogram(sweeps, bins=edges)
    result["sweeps"] = {"min": int(sweeps.min()), "median": float(np.median(sweeps)), "mean": round(float(sweeps.mean()), 2),
                        "max": int(sweeps.max()), "total": int(sweeps.sum()),
                        "histogram": {f"{a}..{b - 1}": int(c) for a, b, c in zip(edges[:-1], edges[1:], hist)}}
    result["n_unconverged"] = model.n_unconverged
    result["nnz"] = model.nnz
    result["density"] = round(model.nnz / (n * (n - 1)), 5)

    stages = {"gram": [], "solve": []}
    for it in range(args.warmup + args.repeats):
        clear_status(model._stats)
        t_gram, A = event_ms(model.gram)
        t_solve, out = event_ms(lambda: model._solve(A))
        if it >= args.warmup:
            stages["gram"].append(t_gram)
            stages["solve"].append(t_solve)
    for key, ms in stages.items():
        result[key] = summary(ms)
    assert torch.equal(out[0], model.item_weights), "the staged run and prepare_model disagree"
    result["solve"]["us_per_column_sweep"] = round(result["solve"]["ms_median"] * 1e3 / result["sweeps"]["total"], 3)

    seen = model.seen_csr()
    gen = torch.Generator(device="cpu").manual_seed(0)
    query = torch.randint(0, N_USERS, (4096,), generator=gen).to(dev)
    ms = []
    for it in range(args.warmup + args.repeats):
        t, _ = event_ms(lambda: model.recommend(query, 10, seen=seen))
        if it >= args.warmup:
            ms.append(t)
    result["recommend"] = {"q4096": summary(ms)}

    if not args.hip_only:
        fixed = hp.SLIM(dict(cfg, tol=0.0, max_sweeps=args.torch_sweeps))
        fixed._stats = model._stats
        hip_ms, torch_ms = [], []
        for it in range(args.warmup + args.repeats):
            t, got = event_ms(lambda: fixed._solve(A))
            if it >= args.warmup:
                hip_ms.append(t)
        for it in range(1 + min(args.repeats, 2)):          # (slow: one warm-up and at most two timed runs)
            t, W_t = event_ms(lambda: torch_sweeps(A, args.l1, args.torch_sweeps))
            if it >= 1:
                torch_ms.append(t)
        scale = float(W_t.abs().max())
        result["fixed_sweeps"] = {
            "sweeps": args.torch_sweeps, "hip_solve": summary(hip_ms), "torch_rank1_form": summary(torch_ms),
            "max_abs_diff_over_scale": float((got[0] - W_t).abs().max() / scale),
            "ratio_torch_over_hip": round(float(np.median(torch_ms)) / float(np.median(hip_ms)), 2)}
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
