"""Measure the GRU4Rec training step on the GPU: the HIP engine against the same step written as torch ops.

    python tools/bench_gru4rec.py [--steps 8] [--windows 4] [--warmup 2] [--repeats 3] [--out profiles/gru4rec_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_gru4rec.py --hip-only --repeats 1   # kernel times

Shapes (40 000 items, constrained embedding, S 2048 extra samples, no dropout, Adam lr 1e-3):
  xe128     B 128, layers [100], cross-entropy with logq 1
  bpr512    B 512, layers [128, 128], bpr-max with bpreg 1 and elu_param 0.5
``--steps`` steps of synthetic ids are staged on the device once; the first resets every slot, the others every
sixteenth.  A window is ``--windows`` passes over those steps between two device synchronisations; the sides alternate
``--repeats`` times in one process, so both see the same machine state.  Sides:
  hip     GRU4RecEngine's launches (hiprec_gru4rec_grad + the dense optimizer sweep), python-looped, no host sync
  torch   the same step as torch ops with autograd (index, F.linear per gate block, the [B, N] score block, softmax /
          ELU / sigmoid on it, torch.optim.Adam), state carried in detached tensors, no host sync either
Peak memory is each side's own: ``torch.cuda.max_memory_allocated`` over the side's construction and its first steps,
less what was allocated before (the engine's workspace comes from the same allocator).  Before anything is timed both
sides compute the first step's loss from the same weights and a zero state; the two values are recorded and the tool
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

I, S, LR, ALPHA = 40000, 2048, 1e-3, 0.5
SHAPES = {"xe128": dict(B=128, layers=[100], loss="cross-entropy", logq=1.0, bpreg=0.0, elu=0.0),
          "bpr512": dict(B=512, layers=[128, 128], loss="bpr-max", logq=0.0, bpreg=1.0, elu=0.5)}


class TorchGRU4Rec(torch.nn.Module):
    """The step of include/hiprec.h's GRU4Rec block as torch ops; parameters keyed like the engine's state_dict."""

    def __init__(self, w, layers, loss, logq, bpreg, elu, log_p):
        super().__init__()
        self.names = list(w)
        self.params = torch.nn.ParameterList(torch.nn.Parameter(v.clone()) for v in w.values())
        self.layers, self.loss, self.logq, self.bpreg, self.elu, self.log_p = layers, loss, logq, bpreg, elu, log_p
        self.state = None

    def forward(self, in_items, targets, reset, samples):
        w = dict(zip(self.names, self.params))
        B = in_items.numel()
        if self.state is None:
            self.state = [torch.zeros(B, H, device=in_items.device) for H in self.layers]
        x = w["Wy.weight"][in_items]
        live = (reset == 0).float()[:, None]
        for i, H in enumerate(self.layers):
            hp = self.state[i] * live
            gi = F.linear(x, w[f"G.{i}.weight_ih"], w[f"G.{i}.bias_ih"])
            gh = F.linear(hp, w[f"G.{i}.weight_hh"], w[f"G.{i}.bias_hh"])
            ir, iz, i_n = gi.split(H, 1)
            hr, hz, hn = gh.split(H, 1)
            r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
            n = torch.tanh(i_n + r * hn)
            x = (1 - z) * n + z * hp
            self.state[i] = x.detach()
        cand = torch.cat([targets, samples])
        R = torch.addmm(w["By.weight"][cand].T, x, w["Wy.weight"][cand].T)
        if self.loss == "cross-entropy":
            if self.logq:
                R = R - self.logq * torch.cat([self.log_p[targets], ALPHA * self.log_p[samples]])[None, :]
            return -torch.log(torch.softmax(R, 1).diagonal() + 1e-24).sum()
        eye = torch.eye(B, R.shape[1], dtype=torch.bool, device=R.device)
        Rp = F.elu(R, self.elu) if self.elu > 0 else R
        s = torch.softmax(Rp.masked_fill(eye, -float("inf")), 1)
        A = (torch.sigmoid(Rp.diagonal()[:, None] - Rp) * s).sum(1)      # s is 0 on the diagonal
        return (-torch.log(A + 1e-24) + self.bpreg * (Rp * Rp * s).sum(1)).sum()


def steps_on(dev, steps, B, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for t in range(steps):
        reset = (rng.random(B) < 1.0 / 16).astype(np.uint8) if t else np.ones(B, dtype=np.uint8)
        arrays = (rng.integers(0, I, B), rng.integers(0, I, B), reset, rng.integers(0, I, S))
        out.append(tuple(torch.from_numpy(a).to(dev) for a in arrays))
    return out


def measure(name, B, layers, loss, logq, bpreg, elu, args, hp, dev):
    torch.manual_seed(0)
    cfg = {"model": {"layers": layers, "constrained_embedding": True, "loss": loss, "bpreg": bpreg, "elu_param": elu,
                     "logq": logq, "n_sample": S, "sample_alpha": ALPHA, "dropout_p_embed": 0.0, "dropout_p_hidden": 0.0,
                     "batch_size": B, "lr": LR, "optimizer": "adam", "device_str": "cuda:0"},
           "dataset": {"n_items": I}, "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    steps = steps_on(dev, args.steps, B)
    probs = np.random.default_rng(2).integers(1, 100, I).astype(np.float64)
    probs /= probs.sum()
    torch.cuda.synchronize()
    peaks = {}

    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.GRU4RecEngine(cfg)
    eng.set_item_probs(probs)
    w0 = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
    # the same step on both sides: the first step's loss from the same weights and a zero state
    eng.model.reset_state(B)
    first_loss = {"hip": float(eng.backward_only(steps[0])[0])}
    eng.load_optimizer_state(0)

    def hip():
        for b in steps:
            eng._enqueue_step(b)

    hip()
    torch.cuda.synchronize()
    peaks["hip"] = torch.cuda.max_memory_allocated() - base
    sides = {"hip": hip}
    if not args.hip_only:
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        ref = TorchGRU4Rec({k: v.to(dev) for k, v in w0.items()}, layers, loss, logq, bpreg, elu, eng._log_p).to(dev)
        opt = torch.optim.Adam(ref.parameters(), lr=LR)
        with torch.no_grad():
            first_loss["torch"] = float(ref(*steps[0]))
        if abs(first_loss["torch"] - first_loss["hip"]) > 1e-4 * abs(first_loss["torch"]):
            raise SystemExit(f"{name}: the two sides do not compute the same loss from the same weights: {first_loss}")

        def torch_steps():
            for b in steps:
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
        return (time.perf_counter() - t0) / (args.windows * len(steps)) * 1e6   # us per step

    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn))
    st = eng._sync_stats()
    out = {"batch": B, "layers": layers, "loss": loss, "logq": logq, "bpreg": bpreg, "elu_param": elu,
           "candidates": B + S, "last_loss_hip": st.loss,
           "first_step_loss": first_loss,      # both sides from the same initial weights; they must agree to 1e-4
           "launches_per_step_derived": 6 + 5 * len(layers) + 1,      # hiprec_gru4rec_grad's and the optimizer sweep
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
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_gru4rec.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_gru4rec.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "n_items": I, "n_sample": S, "sample_alpha": ALPHA,
           "optimizer": "adam", "steps_per_window": args.windows * args.steps, "repeats": args.repeats, "shapes": {}}
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
