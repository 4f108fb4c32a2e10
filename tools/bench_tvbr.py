"""Measure the TVBR training step on the GPU: the HIP engine against the reference's own op sequence on torch.

    python tools/bench_tvbr.py [--steps 8] [--warmup 2] [--repeats 5] [--out profiles/tvbr_step.json]
    rocprofv3 --kernel-trace --stats -f csv -d DIR -- python tools/bench_tvbr.py --hip-only --repeats 1 --shapes default
    python tools/bench_tvbr.py --kernel-stats default=DIR/.../*_kernel_stats.csv --out profiles/tvbr_step.json

The second form is a run of its own under the profiler (one shape per run, so that the shares are that shape's); the
third needs no GPU: it adds each kernel's share of the traced GPU time to the profile the first form wrote.

Shapes: ``default`` is configs/tvbr_default.json (batch 256, n_neg 5, 512-wide random features, emb_dim 64, time_step
10) on tafeng-like table sizes (U 30 000, I 20 000); ``batch4096`` the same widths at batch 4096; ``limits`` the
kernels' limits (emb_dim 128, time_step 255) with 2048-wide features at batch 1024.  All train with RMSprop, alpha 0.001
and tanh, the reference's defaults.  ``--steps`` batches of uniformly drawn triples and negatives are staged on the
device once; as in the epoch loop every row of a batch shares one ``t``, and the batches walk through the time steps.  A
window is as many passes over those batches as last a quarter of a second (calibrated per side on the warm-up) between
two device events, read after a device synchronisation; the sides alternate ``--repeats`` times in one process, so both
see the same machine state.  Sides:
  hip     TVBREngine's launches (hiprec_tvbr_grad + the dense optimizer sweep) with ``noise_rng = "device"`` (one
          torch.randn per step on the GPU), python-looped, no host sync
  torch   the reference's op sequence (models/tvbr.py:121-369, 449-465 restated here, nothing imported from the
          reference: embedding lookups / torch.cat with the time row and the features / every nn.Linear twice /
          torch.randn_like on the GPU / bmm / logsigmoid / kl_div + autograd + torch.optim.RMSprop) WITHOUT
          ``loss.item()``
Recorded per side: the median time per step and the peak device memory above what was allocated before the side's first
step.  There is no earlier number for this model: the yardstick is the torch side of the same run.  Needs a GPU.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LR, ALPHA, ACT = 5e-4, 0.001, "tanh"
SHAPES = {"default": dict(U=30000, I=20000, B=256, n_neg=5, D=64, T=10, Fu=512, Fi=512),
          "batch4096": dict(U=30000, I=20000, B=4096, n_neg=5, D=64, T=10, Fu=512, Fi=512),
          "limits": dict(U=30000, I=20000, B=1024, n_neg=5, D=128, T=255, Fu=2048, Fi=2048)}
MIN_WINDOW_S = 0.25


class TorchTVBR(torch.nn.Module):
    """The op sequence of models/tvbr.py:65-369 (tanh) on whatever device it is moved to."""

    def __init__(self, U, I, D, T, Fu, Fi, n_neg, batch_size, user_fea, item_fea):
        super().__init__()
        nn = torch.nn
        self.emb_dim, self.n_neg, self.batch_size, self.esp = D, n_neg, batch_size, 1e-10
        self.fea = {"u": user_fea, "i": item_fea}
        r = 0.1 * D ** -0.5
        self.user_emb, self.item_emb = nn.Embedding(U, D), nn.Embedding(I, D)
        self.user_emb.weight.data.uniform_(-r, r)
        self.item_emb.weight.data.uniform_(-r, r)
        self.time_embdding = nn.Embedding(T + 1, T + 1, _weight=torch.eye(T + 1))
        self.user_mean = nn.Embedding(U, D, _weight=torch.ones(U, D))
        self.user_std = nn.Embedding(U, D, _weight=torch.zeros(U, D))
        self.item_mean, self.item_std = nn.Embedding(I, D), nn.Embedding(I, D)
        self.item_mean.weight.data.uniform_(-r, r)
        self.item_std.weight.data.uniform_(-r, r)
        for side, Fw in (("u", Fu), ("i", Fi)):
            for kind in ("mean", "std"):
                setattr(self, f"time2{kind}_{side}", nn.Sequential(nn.Linear(D + T + 1 + Fw, D), nn.Tanh()))

    def to(self, dev):
        self.fea = {k: v.to(dev) for k, v in self.fea.items()}
        return super().to(dev)

    def encode(self, side, index, post_rows, pri_rows):
        """((mean, std) of the prior, (mean, std) of the posterior): every Linear runs twice on a concatenated input."""
        fea = self.fea[side][index]
        tables = (self.user_mean, self.user_std) if side == "u" else (self.item_mean, self.item_std)
        mean_row, std_row = tables[0](index), tables[1](index)
        to_mean, to_std = getattr(self, "time2mean_" + side), getattr(self, "time2std_" + side)
        out = []
        for rows in (pri_rows, post_rows):
            mean = to_mean(torch.cat([mean_row, rows, fea], 1))
            std = to_std(torch.cat([std_row, rows, fea], 1)).mul(0.5).exp()
            out.append((mean, std))
        return out

    def kl_div(self, pri, post):
        var1, var2 = pri[1].pow(2) + self.esp, post[1].pow(2) + self.esp
        diff = post[0] - pri[0]
        return (torch.log(var2 / var1) - 1 + (1.0 / var2) * var1 + diff * (1.0 / var2) * diff).mul(0.5).sum(dim=1).mean()

    def forward(self, batch):
        pos_u, pos_i_1, pos_i_2, neg_u, neg_i_1, neg_i_2, pos_t, neg_t = batch
        D2, n = 2 * self.emb_dim, self.n_neg
        rows = {"pos": (self.time_embdding(pos_t + 1), self.time_embdding(pos_t)),
                "neg": (self.time_embdding(neg_t + 1), self.time_embdding(neg_t))}
        kl, embs = 0.0, []
        for side, index, group, table in (("u", pos_u, "pos", self.user_emb), ("i", pos_i_1, "pos", self.item_emb),
                                          ("i", pos_i_2, "pos", self.item_emb), ("u", neg_u.view(-1), "neg", self.user_emb),
                                          ("i", neg_i_1.view(-1), "neg", self.item_emb),
                                          ("i", neg_i_2.view(-1), "neg", self.item_emb)):
            pri, post = self.encode(side, index, *rows[group])
            std = torch.exp(0.5 * post[1])
            z = post[0] + torch.randn_like(std) * std
            kl = kl + self.kl_div(pri, post)
            embs.append(torch.cat((z, table(index)), dim=1))
        emb_u, emb_1, emb_2 = embs[:3]
        neg_eu, neg_e1, neg_e2 = (e.view(-1, n, D2) for e in embs[3:])
        total = 0.0
        for e, other, neg in ((emb_u, emb_1 + emb_2, neg_eu), (emb_1, emb_u + emb_2, neg_e1), (emb_2, emb_u + emb_1, neg_e2)):
            pos = F.logsigmoid(torch.sum(torch.mul(e, other).squeeze(), dim=1))
            ng = F.logsigmoid(-1 * torch.bmm(neg, e.unsqueeze(2)).squeeze())
            total = total + -1 * (torch.sum(pos) + torch.sum(ng))
        return (1 - ALPHA) * total / (3 * self.batch_size) + ALPHA * (-0.5 * kl)


def batches_on(dev, steps, U, I, T, B, n_neg, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for s in range(steps):
        ids = tuple(torch.from_numpy(rng.integers(0, n, shape)).to(dev)
                    for n, shape in ((U, B), (I, B), (I, B), (U, (B, n_neg)), (I, (B, n_neg)), (I, (B, n_neg))))
        t = s % T
        out.append(ids + (torch.full((B,), t, dtype=torch.int64, device=dev),
                          torch.full((B * n_neg,), t, dtype=torch.int64, device=dev)))
    return out


def measure(name, U, I, B, n_neg, D, T, Fu, Fi, args, hp, dev):
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    fea = (torch.from_numpy(rng.standard_normal((U, Fu)).astype(np.float32)),
           torch.from_numpy(rng.standard_normal((I, Fi)).astype(np.float32)))
    ref = TorchTVBR(U, I, D, T, Fu, Fi, n_neg, B, *fea)
    w0 = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    cfg = {"model": {"n_users": U, "n_items": I, "late_dim": 512, "emb_dim": D, "n_neg": n_neg, "batch_size": B,
                     "alpha": ALPHA, "time_step": T, "activator": ACT, "optimizer": "rmsprop", "lr": LR,
                     "device_str": "cuda:0", "noise_rng": "device"},
           "user_fea": fea[0], "item_fea": fea[1], "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.TVBREngine(cfg)
    eng.model.load_state_dict(w0)
    eng.model.train()
    batches = batches_on(dev, args.steps, U, I, T, B, n_neg)
    state = {}

    def hip():
        for b in batches:
            eng._enqueue_step(b)

    def torch_steps():
        if "opt" not in state:                  # built on first use, so that a side's peak memory is its own
            ref.to(dev)
            state["opt"] = torch.optim.RMSprop(ref.parameters(), lr=LR)
        for b in batches:
            state["opt"].zero_grad()
            ref(b).backward()
            state["opt"].step()

    def window(fn, passes):
        """Seconds between two device events around `passes` calls of fn."""
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(passes):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / 1e3

    sides = {"hip": hip}
    if not args.hip_only:
        sides["torch"] = torch_steps
    peak, passes = {}, {}
    for k, fn in sides.items():
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - before) / 1e6
        passes[k] = max(1, int(np.ceil(args.min_window / max(window(fn, 1), 1e-6))))
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn, passes[k]) / (passes[k] * len(batches)) * 1e6)   # us per step
    st = eng._sync_stats()
    Ru, Ri = B * (1 + n_neg), 2 * B * (1 + n_neg)
    Ku, Ki = D + T + 1 + Fu, D + T + 1 + Fi
    out = {"n_users": U, "n_items": I, "batch": B, "n_neg": n_neg, "emb_dim": D, "time_step": T, "fea": [Fu, Fi],
           "user_rows": Ru, "item_rows": Ri, "last_rec_loss_hip": st.loss, "last_kl_loss_hip": st.reg,
           # 2 flops per multiply-add, two encoders per side: base forward + wgrad over K, the table-column dgrad over D
           "gemm_gflop_per_step": round(2 * 2 * (2 * D * (Ru * Ku + Ri * Ki) + (Ru + Ri) * D * D) / 1e9, 3),
           "workspace_mb": round(eng.model._ws.numel() / 1e6, 1),
           "steps_per_window": {k: passes[k] * len(batches) for k in sides}}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 1) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
        out[f"{k}_peak_memory_mb"] = round(peak[k], 1)
    if "torch" in times:
        out["hip_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
        out["hip_not_slower_than_torch"] = bool(out["hip_us_per_step_median"] <= 1.05 * out["torch_us_per_step_median"])
    return out


def merge_kernel_stats(spec, path):
    """``name=csv[,name=csv]``: rocprofv3's kernel statistics of a ``--hip-only`` run of one shape, as
    ``kernel_share_percent`` (every kernel above 0.5 %) of that shape in the profile at ``path``."""
    import csv

    with open(path) as f:
        out = json.load(f)
    for item in spec.split(","):
        name, csv_path = item.split("=", 1)
        with open(csv_path, newline="") as f:
            rows = list(csv.DictReader(f))
        total = sum(float(r["TotalDurationNs"]) for r in rows)
        share = {}
        for r in rows:          # "hiprec::(anonymous namespace)::tv_loss_kernel(hiprec::...)" -> "tv_loss_kernel"
            short = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1]
            share[short] = round(share.get(short, 0.0) + 100.0 * float(r["TotalDurationNs"]) / total, 1)
        out["shapes"][name]["kernel_share_percent"] = {k: v for k, v in sorted(share.items(), key=lambda kv: -kv[1])
                                                       if v >= 0.5}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--min-window", type=float, default=MIN_WINDOW_S, help="seconds per timed window")
    ap.add_argument("--kernel-stats", default=None, help="shape=kernel_stats.csv[,...]: merge into --out and exit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.kernel_stats, args.out)
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_tvbr.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_tvbr.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "optimizer": "rmsprop", "alpha": ALPHA, "activator": ACT,
           "min_window_s": args.min_window, "repeats": args.repeats, "shapes": {}}
    for name in args.shapes.split(","):
        out["shapes"][name] = measure(name, args=args, hp=hp, dev=dev, **SHAPES[name])
        print(name, json.dumps(out["shapes"][name]), flush=True)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
