"""Measure one full ALS sweep on the GPU at a MovieLens-1M-like shape, next to the same normal equations on torch.

    python tools/bench_als.py [--dims 64 128] [--iters 3] [--warmup 1] [--repeats 3] [--out profiles/als_sweep.json]

Shape: 6040 users x 3706 items, about 1 M pairs (tools/bench_knn.py's synthetic log: per-user counts log-normal around
ML-1M's mean of 166, items from a Zipf(1.0) popularity, 1 % of the pairs twice), alpha 40, reg 0.1, D = 64 and 128.

Device side (a window is ``--iters`` sweeps between two device synchronisations, ``--repeats`` windows):
  * ``sweep``   ``update_users`` + ``update_items``: per half a Gram launch and a solve launch (csrc/als.hip) and the
                read-back of the failed-pivot counter and the status word;
  * ``loss``    ``hiprec_als_loss`` and its Gram launch;
and the peak device memory (torch.cuda.max_memory_allocated, reset before the window).

Yardstick, on the same card: the same normal equations on torch -- per chunk of ``--torch-chunk`` rows
``A = (alpha R_chunk) @ [y y^T as rows] + G + reg I`` (one dense GEMM: torch has no batched sparse rank-k update),
``b = C_chunk @ Y``, ``torch.linalg.cholesky_ex`` and ``torch.cholesky_solve`` -- for both halves.  Its result is
compared with the library's, and the chunks whose factorisation torch flags are counted: a flagged chunk or a large
difference means the yardstick's time is not that of a right answer.

Cost model: ``2 nnz D^2`` flops of assembly per half-sweep plus ``n D^3 / 3`` of factorisation, against the 157 TF
fp32-MFMA peak; the tool prints the achieved fraction.  Needs a GPU: there is no CPU timing path.
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
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_knn import N_ITEMS, N_USERS, synthetic_log  # noqa: E402

ALPHA, REG, PEAK_TF = 40.0, 0.1, 157.0


def torch_half_sweep(R, other, alpha, reg, chunk, flagged):
    """``R [rows, cols]`` dense counts on the device, ``other [cols, D]``: the rows' exact solves, chunk by chunk.
    ``flagged``: a list that collects ``(first row, matrices with info != 0)`` of the chunks ``cholesky_ex`` flags; the
    solve goes on regardless and the caller compares the result with the library's."""
    D = other.shape[1]
    G_reg = other.T @ other + reg * torch.eye(D, device=other.device)
    outer = (other[:, :, None] * other[:, None, :]).reshape(other.shape[0], D * D)
    out = torch.zeros((R.shape[0], D), device=other.device)
    infos = []
    for r0 in range(0, R.shape[0], chunk):
        Rc = R[r0:r0 + chunk]
        A = ((alpha * Rc) @ outer).view(-1, D, D) + G_reg
        b = (torch.where(Rc > 0, 1.0 + alpha * Rc, torch.zeros_like(Rc)) @ other).unsqueeze(2)
        L, info = torch.linalg.cholesky_ex(A)
        out[r0:r0 + chunk] = torch.cholesky_solve(b, L).squeeze(2)
        infos.append((r0, info))
    flagged.extend((r0, int((info != 0).sum())) for r0, info in infos if bool((info != 0).any()))
    return out * (R.sum(dim=1, keepdim=True) > 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--torch-chunk", type=int, default=512)
    ap.add_argument("--hip-only", action="store_true", help="skip the torch yardstick")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_als.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    users, items = synthetic_log()
    users_d, items_d = torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev)
    result = {"tool": "tools/bench_als.py", "device": torch.cuda.get_device_name(0),
              "source_hash": __graft_entry__.source_hash(), "n_users": N_USERS, "n_items": N_ITEMS,
              "n_interactions": int(users.size), "alpha": ALPHA, "reg": REG, "iters_per_window": args.iters,
              "repeats": args.repeats, "peak_tf_fp32_mfma": PEAK_TF}

    def windows(fn):
        for _ in range(args.warmup):
            fn()
        out = []
        torch.cuda.reset_peak_memory_stats(dev)
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / args.iters * 1e3)
        return {"ms": [round(x, 4) for x in out], "ms_median": round(float(np.median(out)), 4),
                "ms_spread": round(max(out) - min(out), 4),
                "peak_device_bytes": int(torch.cuda.max_memory_allocated(dev))}

    for D in args.dims:
        torch.manual_seed(D)
        cfg = {"model": dict(n_users=N_USERS, n_items=N_ITEMS, emb_dim=D, alpha=ALPHA, reg=REG, stddev=0.1,
                             device_str="cuda:0")}
        with contextlib.redirect_stdout(io.StringIO()):
            eng = hp.ALSEngine(cfg)
        eng.prepare((users_d, items_d))
        start = eng.model.flat.clone()
        nnz = int(eng._b[1].numel())
        flops = 2 * (2.0 * nnz * D * D) + (N_USERS + N_ITEMS) * D ** 3 / 3.0

        def sweep():
            eng.update_users()
            eng.update_items()

        row = {"nnz": nnz, "model_flops_per_sweep": flops, "sweep": windows(sweep), "loss": windows(eng.loss)}
        row["achieved_tf"] = round(flops / (row["sweep"]["ms_median"] * 1e-3) / 1e12, 3)
        row["fraction_of_fp32_mfma_peak"] = round(row["achieved_tf"] / PEAK_TF, 4)
        if not args.hip_only:
            R = torch.zeros((N_USERS, N_ITEMS), device=dev)
            R.index_put_((users_d, items_d), torch.ones(users_d.numel(), device=dev), accumulate=True)
            Rt = R.T.contiguous()
            eng.model.flat.copy_(start)
            X0, Y0 = (t.clone() for t in eng.model.ranking_factors()[:2])
            state = {}

            def torch_sweep():
                state["flagged"] = []
                state["X"] = torch_half_sweep(R, Y0, ALPHA, REG, args.torch_chunk, state["flagged"])
                state["Y"] = torch_half_sweep(Rt, state["X"], ALPHA, REG, args.torch_chunk, state["flagged"])

            row["torch_sweep"] = windows(torch_sweep)
            # chunks whose factorisation torch flagged as not positive definite in the last sweep (every A is finite and
            # positive definite by construction); the comparison below says whether the result was right regardless
            row["torch_sweep"]["chunks_flagged_by_cholesky_ex"] = len(state["flagged"])
            row["torch_sweep"]["chunks_per_sweep"] = -(-N_USERS // args.torch_chunk) + -(-N_ITEMS // args.torch_chunk)
            row["torch_sweep"]["users_finite"] = bool(torch.isfinite(state["X"]).all())
            row["torch_sweep"]["finite"] = bool(torch.isfinite(state["X"]).all() and torch.isfinite(state["Y"]).all())
            sweep()
            X, Y = eng.model.ranking_factors()[:2]
            row["max_abs_diff_vs_torch_over_scale"] = {
                "users": float((X - state["X"]).abs().max() / state["X"].abs().max()),
                "items": float((Y - state["Y"]).abs().max() / state["Y"].abs().max())}
            row["ratio_torch_over_hip"] = round(row["torch_sweep"]["ms_median"] / row["sweep"]["ms_median"], 2)
            del R, Rt
        result[f"d{D}"] = row
        print(json.dumps({f"d{D}": row}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
