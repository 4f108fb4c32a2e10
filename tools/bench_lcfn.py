"""Measure the LCFN training step on the GPU: the HIP engine against the reference's op sequence written in torch.

    python tools/bench_lcfn.py [--repeats 5] [--out profiles/lcfn_step.json]

Three shapes, Adam, ``lamda`` 0.02:
  * ``ml100k``: 943 x 1682, F 4 / 8, D 64, layer 1, B 400 (configs/lcfn_default.json on ml-100k);
  * ``ml1m``: 6040 x 3706, F 30 / 18, D 64, layer 1, B 400;
  * ``wide``: 200 000 x 100 000, F 256 / 256, D 64, layer 2, B 4096 -- here the two [n, F] bases (307 MB) are read four
    times per layer and bandwidth decides.
The bases are random with columns of unit norm (an eigendecomposition of a 200 000-node Laplacian is no part of a step).
The yardstick is the reference's step (lcfn.py:55-87, :171-205 restated here in torch ops -- ``matmul(P, diag(f))``,
``matmul(P^T, X)``, the transform, the sigmoid, per side and layer; nothing imported from the reference; for layer 2 the
obvious reading of its loop) with ``backward()`` and ``torch.optim.Adam``, on the same GPU.

A window is ``steps`` training steps on resident batches, timed with device events around the whole window; windows of
the two sides alternate ``--repeats`` times in one process after a warm-up of each side at the same shape, and the
median and the spread (max - min over the median) are reported.  ``steps`` is chosen per side so that a window lasts
about ``--min-window`` seconds.  Peak memory is ``torch.cuda.max_memory_allocated`` over a side's set-up, warm-up and
first window minus what was allocated before that side was built; both sides allocate through torch.
``min_bytes_per_step`` is what the HIP step must move at least (bases four times per layer, the table-sized reads and
writes of every launch, the optimizer sweep); over the measured time it gives ``achieved_gb_per_s``.  Needs a GPU.

Not measured: hardware counters, per-kernel times, anything multi-GPU.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LAMDA, LR = 0.02, 0.005
#            U        I        F_u  F_i  D   L  B
SHAPES = {"ml100k": (943, 1682, 4, 8, 64, 1, 400), "ml1m": (6040, 3706, 30, 18, 64, 1, 400),
          "wide": (200_000, 100_000, 256, 256, 64, 2, 4096)}


def random_basis(n, f, rng):
    b = rng.standard_normal((n, f), dtype=np.float32)
    return b / np.linalg.norm(b, axis=0, keepdims=True)


class TorchLCFN(torch.nn.Module):
    """The step of models/lcfn.py in torch ops, on whatever device it is moved to."""

    def __init__(self, U, I, D, L, P, Q, filters_u, filters_i, transformers):
        super().__init__()
        self.L = L
        self.user_embeddings = torch.nn.Embedding(U, D)
        self.item_embeddings = torch.nn.Embedding(I, D)
        torch.nn.init.normal_(self.user_embeddings.weight, mean=0.01, std=0.02)
        torch.nn.init.normal_(self.item_embeddings.weight, mean=0.01, std=0.02)
        self.P, self.Q = P, Q
        self.user_filters, self.item_filters, self.transformers = filters_u, filters_i, transformers

    def side(self, emb, B, filters):
        x = emb
        out = [x]
        for k in range(self.L):
            x = torch.matmul(torch.matmul(B, torch.diag(filters[k])), torch.matmul(torch.transpose(B, 0, 1), x))
            x = torch.sigmoid(torch.matmul(x, self.transformers[k]))
            out.append(x)
        return torch.cat(out, 1)

    def forward(self, users, pos, neg):
        ua = self.side(self.user_embeddings.weight, self.P, self.user_filters)
        ia = self.side(self.item_embeddings.weight, self.Q, self.item_filters)
        u, p, n = ua[users], ia[pos], ia[neg]
        bpr = -torch.mean(torch.nn.functional.logsigmoid((u * p).sum(1) - (u * n).sum(1)))
        reg = (torch.norm(self.user_embeddings(users)) + torch.norm(self.item_embeddings(pos))
               + torch.norm(self.item_embeddings(neg)))
        for k in range(self.L):
            reg = reg + torch.norm(self.user_filters[k]) + torch.norm(self.item_filters[k]) + torch.norm(self.transformers[k])
        return bpr + LAMDA * reg


def min_bytes_per_step(U, I, Fu, Fi, D, L):
    """What one HIP step reads and writes at least, launch by launch (fp32)."""
    bases, rows = U * Fu + I * Fi, U + I
    fwd = rows * D * 2 + L * (2 * bases + rows * D * 2)          # hop 0 copy; per layer: project + expand
    bwd = rows * (L + 1) * D + L * (2 * bases + rows * D * 4)    # clear G; per layer: project reads G, X; expand r/m/w
    sweep = rows * D * 8                                         # Adam: w, g, m, v read and written
    return 4 * (fwd + bwd + sweep)


def timed_window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn(steps)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / steps          # us per step


def run_shape(name, args, dev):
    import beta_recsys_amd as hp

    U, I, Fu, Fi, D, L, B = SHAPES[name]
    rng = np.random.default_rng(B)
    P, Q = random_basis(U, Fu, rng), random_basis(I, Fi, rng)
    n_batches = 8
    batches = [tuple(torch.from_numpy(rng.integers(0, n, B)).to(dev) for n in (U, I, I)) for _ in range(n_batches)]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    torch.manual_seed(0)
    np.random.seed(0)
    model = dict(n_users=U, n_items=I, emb_dim=D, layer=L, lamda=LAMDA, graph_embeddings=[P, Q], optimizer="adam", lr=LR,
                 device_str="cuda:0", batch_size=B)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.LCFNEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_bench_runs"}})
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
        m = eng.model
        ref = TorchLCFN(U, I, D, L, torch.from_numpy(P).to(dev), torch.from_numpy(Q).to(dev),
                        [t.detach().clone() for t in m.user_filters], [t.detach().clone() for t in m.item_filters],
                        [t.detach().clone() for t in m.transformers]).to(dev)
        m.load_state_dict({k: v.detach().clone() for k, v in ref.state_dict().items()})
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
    out = {"n_users": U, "n_items": I, "frequencies": [Fu, Fi], "emb_dim": D, "layer": L, "batch": B, "optimizer": "adam",
           "repeats": args.repeats, "steps_per_window": steps, "bases_bytes": 4 * (U * Fu + I * Fi),
           "min_bytes_per_step": min_bytes_per_step(U, I, Fu, Fi, D, L), "launches_per_step": 6 + 6 * L,
           "hip_resident_bytes": int(hip_resident), "last_loss_hip": st.loss, "last_parts_hip": list(eng.last_losses())}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 1) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
        out[f"{k}_peak_bytes"] = int(peaks[k])
    out["achieved_gb_per_s"] = round(out["min_bytes_per_step"] / out["hip_us_per_step_median"] / 1e3, 1)
    out["us_per_launch"] = round(out["hip_us_per_step_median"] / out["launches_per_step"], 2)
    if "torch" in times:
        out["speedup_vs_torch"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
        out["hip_beats_torch_beyond_spread"] = bool(max(times["hip"]) < min(times["torch"]))
        out["peak_bytes_saved"] = int(peaks["torch"] - peaks["hip"])
    out["not_measured"] = ["hardware counters", "per-kernel times", "multi-GPU"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_lcfn.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__

    dev = torch.device("cuda:0")
    result = {"tool": "tools/bench_lcfn.py", "device": torch.cuda.get_device_name(0),
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
