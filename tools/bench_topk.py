"""Measure full-catalogue top-K recommendation on the GPU: the fused HIP path against the torch op sequence.

    python tools/bench_topk.py [--iters 5] [--warmup 2] [--repeats 3] [--out profiles/topk.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_topk.py --hip-only --repeats 1      # kernel times

k = 20 at two shapes:
  * headline   the headline tables (6040 x 3706 x 64), all 6040 users queried, seen lists of mean length ~166 (ML-1M:
               1 000 209 interactions / 6040 users);
  * catalogue  4096 query users against 1 000 000 x 128 item factors (the item side of BASELINE configs[3]), seen lists
               of mean length ~100 (that config names no data set; 100 is this tool's choice).
Seen lists are drawn per user from a Zipf(1.0) item popularity (with replacement, duplicates dropped; the measured mean
length is in the output).  The yardstick is what a user of torch would write on the same GPU: ``U[q] @ I.T``, ``+ bias``,
``index_put_`` of -inf at the seen pairs, ``torch.topk`` -- at the catalogue shape chunked over users, CHUNK = 512 users
(a 2 GB score matrix per chunk; all 4096 at once would be 16 GB).  A window is ``--iters`` calls between two device
synchronisations; fused and torch windows alternate ``--repeats`` times in one process.  The fused call includes its
host sync (the status word is read back after every call); the torch side syncs once per window.
Needs a GPU: there is no CPU timing path.

Printed with the result: the FLOPs of the scores (2 n_query n_items D) over the fused time as a fraction of the fp32-MFMA
peak, and the HBM floor of one pass over the item factors per 64-user tile (which is what the kernel would read if no
tile's pass hit in a cache).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MFMA_F32_PEAK = 157.3e12   # FLOP/s, fp32-input MFMA
HBM_RATE = 6.29e12         # B/s measured float4 copy
K = 20
CHUNK = 512                # users per score matrix of the torch side at the catalogue shape
USER_TILE = 64             # query users per block of topk_score_kernel
SHAPES = {"headline": dict(n_query=6040, n_items=3706, dim=64, seen_mean=166, chunk=None),
          "catalogue": dict(n_query=4096, n_items=1_000_000, dim=128, seen_mean=100, chunk=CHUNK)}


def zipf_seen(n_users, n_items, mean_len, dev, seed):
    """(users, items) id columns: per user draws from a Zipf(1.0) popularity over a random item permutation, enough of
    them that the mean number of DISTINCT items per user reaches ``mean_len``."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    p = 1.0 / torch.arange(1, n_items + 1, device=dev, dtype=torch.float64)
    perm = torch.randperm(n_items, device=dev, generator=gen)
    draws = mean_len
    while True:
        ranks = torch.multinomial((p / p.sum()).float(), n_users * draws, replacement=True, generator=gen)
        users = torch.arange(n_users, device=dev).repeat_interleave(draws)
        key = torch.unique(users * n_items + perm[ranks])
        if key.numel() >= n_users * mean_len or draws > 64 * mean_len:
            return torch.div(key, n_items, rounding_mode="floor"), key % n_items
        draws = int(draws * 1.3) + 1


def run_shape(name, spec, args, dev):
    from beta_recsys_amd.data import build_positive_csr
    from beta_recsys_amd.recommend import normalise_seen, topk_factors

    n, n_items, dim = spec["n_query"], spec["n_items"], spec["dim"]
    gen = torch.Generator(device=dev).manual_seed(17)
    U = torch.randn(n, dim, device=dev, generator=gen) * 0.1
    I = torch.randn(n_items, dim, device=dev, generator=gen) * 0.1
    bias = torch.randn(n_items, device=dev, generator=gen) * 0.1
    su, si = zipf_seen(n, n_items, spec["seen_mean"], dev, seed=3)
    csr = normalise_seen(build_positive_csr(su, si, n, n_items), n, n_items, dev)   # checked once, like the factors
    query = torch.arange(n, device=dev)
    chunk = spec["chunk"] or n
    neg_inf = torch.tensor(float("-inf"), device=dev)
    bounds = [(lo, min(lo + chunk, n)) for lo in range(0, n, chunk)]
    pair_slices = [(int(csr[0][lo]), int(csr[0][hi])) for lo, hi in bounds]   # su is sorted by user (unique keys)

    def fused():
        return topk_factors(U, I, 1.0, bias, query, K, csr, 0)

    def torch_ops():
        items, scores = [], []
        for (lo, hi), (a, b) in zip(bounds, pair_slices):
            s = U[query[lo:hi]] @ I.T
            s += bias
            s.index_put_((su[a:b] - lo, si[a:b]), neg_inf)
            top = torch.topk(s, K)
            items.append(top.indices)
            scores.append(top.values)
        return torch.cat(items), torch.cat(scores)

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.iters * 1e3   # ms per call

    sides = {"fused": fused} if args.hip_only else {"fused": fused, "torch": torch_ops}
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn))
    flops = 2.0 * n * n_items * dim
    item_bytes = 4.0 * n_items * dim
    tiles = (n + USER_TILE - 1) // USER_TILE
    out = {"shape": name, "n_query": n, "n_items": n_items, "emb_dim": dim, "k": K,
           "seen_mean_len": round(si.numel() / n, 2), "torch_chunk_users": chunk, "iters_per_window": args.iters,
           "repeats": args.repeats, "score_flops": flops, "item_factor_bytes": item_bytes, "user_tiles": tiles,
           "hbm_floor_ms_one_pass_per_user_tile": round(tiles * item_bytes / HBM_RATE * 1e3, 4)}
    for k, v in times.items():
        out[f"{k}_ms"] = [round(x, 4) for x in v]
        out[f"{k}_ms_median"] = round(float(np.median(v)), 4)
        out[f"{k}_ms_spread"] = round(max(v) - min(v), 4)
    out["fused_fraction_of_f32_mfma_peak"] = round(flops / (out["fused_ms_median"] * 1e-3) / MFMA_F32_PEAK, 4)
    if "torch" in times:
        out["speedup_vs_torch_ops"] = round(out["torch_ms_median"] / out["fused_ms_median"], 3)
        # the requirement: the fused median is not above the torch median by more than torch's own max - min
        out["fused_within_torch_spread_or_faster"] = bool(
            out["fused_ms_median"] <= out["torch_ms_median"] + out["torch_ms_spread"])
        fi, fs = fused()
        ti, ts = torch_ops()
        out["scores_max_abs_diff_vs_torch"] = float((fs - ts).abs().max())
        out["lists_identical_to_torch"] = float((fi == ti).all(dim=1).float().mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_topk.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__

    dev = torch.device("cuda:0")
    result = {"tool": "tools/bench_topk.py", "device": torch.cuda.get_device_name(0),
              "source_hash": __graft_entry__.source_hash(), "f32_mfma_peak_flops": MFMA_F32_PEAK,
              "hbm_rate_bytes_per_s": HBM_RATE, "shapes": []}
    for name in args.shapes.split(","):
        result["shapes"].append(run_shape(name, SHAPES[name], args, dev))
        print(json.dumps(result["shapes"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
