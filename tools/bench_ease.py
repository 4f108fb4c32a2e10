"""Measure EASE's ``prepare_model`` on the GPU at a MovieLens-1M-like shape, next to torch's Cholesky inverse of the same
matrix on the same card.

    python tools/bench_ease.py [--repeats 5] [--warmup 1] [--out profiles/ease.json]

Shape: 6040 users x 3706 items, about 1 M pairs (tools/bench_knn.py's synthetic log), reg 500.

Device side, HIP events around each stage, the median over ``--repeats`` after ``--warmup`` runs:
  * ``gram``     hiprec_ease_gram: G = X^T X + reg I by integer counting;
  * ``invert``   hiprec_ease_invert: the blocked Cholesky, L^-1 carried along, P = L^-T L^-1 (4 launches per panel);
  * ``finish``   hiprec_ease_finish: B = -P / diag(P), zero diagonal, both triangles;
  * ``prepare_model``  the whole call, wall clock between two synchronisations: the two CSRs (torch), the three stages
                 and the read-back of the status word;
  * ``recommend``  256, 1024 and 4096 query users, top 10 under the training frame's seen mask;
and the peak device memory of ``prepare_model`` (torch.cuda.max_memory_allocated, reset before it).

Yardstick: ``torch.linalg.cholesky`` + ``torch.cholesky_inverse`` of the same ``G``.  Both results' ``max |G P - I|``
(evaluated in fp64 on the card) are recorded next to the times: a time is only worth comparing when its answer is right.

Cost model: ``n^3 / 3`` multiply-adds each for the factorisation, for L^-1 and for L^-T L^-1, so ``2 n^3`` flops,
against the 157 TF fp32-MFMA peak.  Needs a GPU: there is no CPU timing path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_knn import N_ITEMS, N_USERS, synthetic_log  # noqa: E402

REG, PEAK_TF = 500.0, 157.0


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


def residual(G, P):
    n = G.shape[0]
    return float((G.double() @ P.double() - torch.eye(n, dtype=torch.float64, device=G.device)).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reg", type=float, default=REG)
    ap.add_argument("--hip-only", action="store_true", help="skip the torch yardstick")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_ease.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp
    from beta_recsys_amd import _lib
    from beta_recsys_amd._stats import clear_status

    dev = torch.device("cuda:0")
    users, items = synthetic_log()
    users_d, items_d = torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev)
    n = N_ITEMS
    flops = 2.0 * n ** 3
    result = {"tool": "tools/bench_ease.py", "device": torch.cuda.get_device_name(0),
              "source_hash": __graft_entry__.source_hash(), "n_users": N_USERS, "n_items": n,
              "n_interactions": int(users.size), "reg": args.reg, "repeats": args.repeats, "warmup": args.warmup,
              "panels": -(-n // hp.ease.PANEL), "launches_of_invert": 4 * (-(-n // hp.ease.PANEL)) - 2 + 3,
              "model_flops_of_invert": flops, "peak_tf_fp32_mfma": PEAK_TF}
    model = hp.EASE(dict(n_users=N_USERS, n_items=n, reg=args.reg, device_str="cuda:0", keep_inverse=True))

    # the whole call
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

    # the three stages on their own
    lib = _lib.load()
    stages = {"gram": [], "invert": [], "finish": []}
    for it in range(args.warmup + args.repeats):
        ws, ws_bytes = model._ease_workspace(lib, dev)
        clear_status(model._stats)
        t_gram, G = event_ms(lambda: model.gram((ws, ws_bytes)))
        G0 = G.clone()
        t_inv, _ = event_ms(lambda: model._invert(G, ws, ws_bytes))
        B = ws[:n * n].view(n, n)
        t_fin, _ = event_ms(lambda: model._finish(G, B))
        model._raise_not_spd()
        if it >= args.warmup:
            for key, t in (("gram", t_gram), ("invert", t_inv), ("finish", t_fin)):
                stages[key].append(t)
    for key, ms in stages.items():
        result[key] = summary(ms)
    result["invert"]["achieved_tf"] = round(flops / (result["invert"]["ms_median"] * 1e-3) / 1e12, 3)
    result["invert"]["fraction_of_fp32_mfma_peak"] = round(result["invert"]["achieved_tf"] / PEAK_TF, 4)
    result["invert"]["max_abs_GP_minus_I"] = residual(G0, G)
    assert torch.equal(B, model.item_weights), "the staged run and prepare_model disagree"

    # queries
    seen = model.seen_csr()
    gen = torch.Generator(device="cpu").manual_seed(0)
    result["recommend"] = {}
    for q in (256, 1024, 4096):
        query = torch.randint(0, N_USERS, (q,), generator=gen).to(dev)
        ms = []
        for it in range(args.warmup + args.repeats):
            t, _ = event_ms(lambda: model.recommend(query, 10, seen=seen))
            if it >= args.warmup:
                ms.append(t)
        result["recommend"][f"q{q}"] = summary(ms)

    if not args.hip_only:
        ms = []
        for it in range(args.warmup + args.repeats):
            t, P_t = event_ms(lambda: torch.cholesky_inverse(torch.linalg.cholesky(G0)))
            if it >= args.warmup:
                ms.append(t)
        result["torch_cholesky_inverse"] = dict(summary(ms), max_abs_GP_minus_I=residual(G0, P_t),
                                                finite=bool(torch.isfinite(P_t).all()))
        result["max_abs_diff_of_P_vs_torch_over_scale"] = float((G - P_t).abs().max() / P_t.abs().max())
        result["ratio_torch_over_hip_invert"] = round(
            result["torch_cholesky_inverse"]["ms_median"] / result["invert"]["ms_median"], 3)
    print(json.dumps(result), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
