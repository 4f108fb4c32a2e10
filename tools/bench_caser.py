"""Measure the Caser training step on the GPU: the HIP engine against the same step written as torch ops.

    python tools/bench_caser.py [--steps 4] [--windows 4] [--warmup 2] [--repeats 3] [--out profiles/caser_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_caser.py --hip-only --repeats 1   # kernel times

Shapes (T 3, N 3, relu / relu, dropout 0.5 drawn on the device, l2 1e-6, Adam lr 1e-3):
  ml1m   6040 users x 3416 items, B 512, L 5, d 50, n_v 4, n_h 16 (the paper's MovieLens-1M setting)
  wide   the same tables, B 4096, L 9, d 128, n_v 16, n_h 64
``--steps`` batches of synthetic sequences are staged on the device once.  A window is ``--windows`` passes over those
batches between two device synchronisations; the sides alternate ``--repeats`` times in one process, so both see the
same machine state.  Sides:
  hip     CaserEngine's launches (hiprec_caser_grad + the dense optimizer sweep), python-looped, no host sync
  torch   the same model as torch ops with autograd (one F.conv2d and one max per height, a concat, F.dropout, a
          baddbmm against the gathered W2 rows, torch.optim.Adam(weight_decay=l2)), no host sync either
Peak memory is each side's own: ``torch.cuda.max_memory_allocated`` over the side's construction and its first steps,
less what was allocated before (the engine's workspace comes from the same allocator).  Before anything is timed both
sides compute the first batch's loss from the same initial weights in eval mode; the two values are recorded and the tool
stops if they differ by more than 1e-4 relative.  There is no earlier number for this model.  Needs a GPU.
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

U, I, T, N, P, L2, LR = 6040, 3416, 3, 3, 0.5, 1e-6, 1e-3
SHAPES = {"ml1m": dict(B=512, L=5, d=50, n_v=4, n_h=16), "wide": dict(B=4096, L=9, d=128, n_v=16, n_h=64)}


class TorchCaser(torch.nn.Module):
    """The model of include/hiprec.h's Caser block as torch ops; parameters keyed like the engine's state_dict."""

    def __init__(self, w, L, p):
        super().__init__()
        self.names = list(w)
        self.params = torch.nn.ParameterList(torch.nn.Parameter(v.clone()) for v in w.values())
        self.L, self.p = L, p

    def forward(self, users, seq, pos, neg):
        w = dict(zip(self.names, self.params))
        E = w["item_embeddings.weight"][seq].unsqueeze(1)                          # [B, 1, L, d]
        out_v = F.conv2d(E, w["conv_v.weight"], w["conv_v.bias"]).flatten(1)
        out_h = [F.relu(F.conv2d(E, w[f"conv_h.{i}.weight"], w[f"conv_h.{i}.bias"]).squeeze(3)).max(2).values
                 for i in range(self.L)]
        o = F.dropout(torch.cat([out_v] + out_h, 1), self.p, self.training)
        z = F.relu(F.linear(o, w["fc1.weight"], w["fc1.bias"]))
        x = torch.cat([z, w["user_embeddings.weight"][users]], 1).unsqueeze(2)
        items = torch.cat([pos, neg], 1)
        s = torch.baddbmm(w["b2.weight"][items], w["W2.weight"][items], x).squeeze(2)
        sp, sn = s[:, :pos.shape[1]], s[:, pos.shape[1]:]
        return F.softplus(-sp).mean() + F.softplus(sn).mean()


def batches_on(dev, steps, B, L, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        arrays = (rng.integers(0, U, B), rng.integers(1, I + 1, (B, L)), rng.integers(1, I + 1, (B, T)),
                  rng.integers(1, I + 1, (B, N)))
        out.append(tuple(torch.from_numpy(a).to(dev) for a in arrays))
    return out


def measure(name, B, L, d, n_v, n_h, args, hp, dev):
    torch.manual_seed(0)
    cfg = {"model": {"n_users": U, "n_items": I, "emb_dim": d, "L": L, "T": T, "neg_samples": N, "n_v": n_v, "n_h": n_h,
                     "ac_conv": "relu", "ac_fc": "relu", "dropout_rate": P, "l2": L2, "lr": LR, "optimizer": "adam",
                     "batch_size": B, "device_str": "cuda:0", "dropout_rng": "device", "dropout_seed": 1},
           "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    batches = batches_on(dev, args.steps, B, L)
    torch.cuda.synchronize()
    peaks = {}

    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.CaserEngine(cfg)
    w0 = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
    # the same step on both sides: the first batch's loss from the same weights, in eval mode (no dropout draws)
    eng.model.eval()
    first_loss = {"hip": float(eng.backward_only(batches[0])[0])}
    eng.model.train()
    eng.load_optimizer_state(0)

    def hip():
        for b in batches:
            eng._enqueue_step(b)

    hip()
    torch.cuda.synchronize()
    peaks["hip"] = torch.cuda.max_memory_allocated() - base
    sides = {"hip": hip}
    if not args.hip_only:
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ref = TorchCaser({k: v.to(dev) for k, v in w0.items()}, L, P).to(dev)
        opt = torch.optim.Adam(ref.parameters(), lr=LR, weight_decay=L2)
        ref.eval()
        with torch.no_grad():
            first_loss["torch"] = float(ref(*batches[0]))
        ref.train()
        if abs(first_loss["torch"] - first_loss["hip"]) > 1e-4 * abs(first_loss["torch"]):
            raise SystemExit(f"{name}: the two sides do not compute the same loss from the same weights: {first_loss}")

        def torch_steps():
            for b in batches:
                opt.zero_grad()
                ref(*b).backward()
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
    width = n_v * d + n_h * L
    conv_flop = 2 * B * n_h * d * sum(h * (L - h + 1) for h in range(1, L + 1))
    out = {"batch": B, "L": L, "emb_dim": d, "n_v": n_v, "n_h": n_h, "fc1_inputs": width, "last_loss_hip": st.loss,
           "first_batch_eval_loss": first_loss,      # both sides from the same initial weights; they must agree to 1e-4
           # derived, not measured: the horizontal filters' forward products; their backward is twice that
           "conv_h_forward_gflop_derived": round(conv_flop / 1e9, 3),
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_caser.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_caser.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "n_users": U, "n_items": I, "T": T, "neg_samples": N,
           "dropout": P, "l2": L2, "optimizer": "adam", "steps_per_window": args.windows * args.steps,
           "repeats": args.repeats, "shapes": {}}
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
