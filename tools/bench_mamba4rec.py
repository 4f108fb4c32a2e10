"""Measure Mamba4Rec on the GPU: the selective scan alone against the same scan as torch ops (a Python loop over the
positions with autograd: the only form there is without a CUDA extension), forward and backward, and the whole training
step of the HIP engine against the same model written as torch ops.

    python tools/bench_mamba4rec.py [--steps 3] [--warmup 2] [--repeats 5] [--out profiles/mamba4rec_step.json]

Scan stage (B 128; T in 50, 200, 256; d_inner in 128, 256; N in 16, 32), ``--stage-iters`` HIP calls per sample:
  hip_fwd    hiprec_mamba4rec_scan, out only: one launch
  torch_fwd  the loop of tests/mamba4rec_torch.py under no_grad (one call per sample)
  hip_bwd    hiprec_mamba4rec_scan from dout: all seven gradients, kernel + the folds of its partials
  torch_bwd  the loop with autograd and torch.autograd.grad of it: forward AND backward, the tape cannot be kept
             (one call per sample; the HIP backward recomputes the states, so hip_bwd alone is the fair counterpart of
             torch_bwd minus torch_fwd; both are reported)
Whole step (43 097 items, B 128, T 50, D 64, two layers, d_state 32, d_conv 4, expand 2, ffn 4 D, Adam lr 1e-3, no dropout):
  hip        Mamba4RecEngine's launches (hiprec_mamba4rec_grad + the dense optimizer sweep), no host sync
  torch      the same model as torch ops with autograd, fp32, TF32 off
One sample is the HIP-event time of a pass divided by its number of calls; the sides alternate ``--repeats`` times in one
process after ``--warmup`` passes each, and the medians are reported with their spread.  Peak memory is
``torch.cuda.max_memory_allocated`` of one pass above what was resident before it (the HIP side's scratch and workspace are
torch tensors).  Before anything is timed the stage's two forms must agree to 1e-5 of each output's scale and the two steps'
first losses to 1e-4.  Needs a GPU.
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
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

I, B, NB, LR = 43097, 128, 2, 1e-3
STAGE_SHAPES = [(T, Di, N) for T in (50, 200, 256) for Di in (128, 256) for N in (16, 32)]
STEP = dict(T=50, D=64, N=32, Kc=4, expand=2)


def event_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)


def alternate(sides, calls, args):
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(event_us(fn, calls[k]))
    out = {}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us"] = [round(x, 1) for x in v]
        out[f"{k}_us_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
    return out


def measure_stage(T, Di, N, args, dev):
    import mamba4rec_torch as mt
    from beta_recsys_amd import _lib, selective_scan

    n = args.stage_iters
    gen = torch.Generator(device=dev).manual_seed(T * 1000 + Di + N)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)      # noqa: E731
    u, dt_pre, z, Bm, Cm, dout = rnd(B, T, Di), rnd(B, T, Di) * 2 - 2, rnd(B, T, Di), rnd(B, T, N), rnd(B, T, N), rnd(B, T, Di)
    A, Dp = -torch.exp(torch.rand(Di, N, device=dev, generator=gen) * 3 - 1), rnd(Di)
    start = torch.randint(0, T // 2, (B,), device=dev, generator=gen)
    m = (torch.arange(T, device=dev)[None] >= start[:, None]).float()
    ins = (u, dt_pre, z, A, Bm, Cm, Dp)

    # the timed HIP side calls the library on buffers made once: no allocation inside the window
    lib, st, start32 = _lib.load(), _lib.stream_ptr(dev), start.to(torch.int32)
    need = lib.hiprec_mamba4rec_scan_scratch_floats(B, T, Di, N)
    bufs = [torch.empty_like(t) for t in (u,) + ins] + [torch.empty(need, device=dev)]
    head = [_lib.ptr(t) for t in ins + (start32,)]

    def hip_fwd():
        for _ in range(n):
            _lib.check(lib.hiprec_mamba4rec_scan(*head, None, B, T, Di, N, _lib.ptr(bufs[0]), *([None] * 8), 0, st))

    def hip_bwd():
        for _ in range(n):
            _lib.check(lib.hiprec_mamba4rec_scan(*head, _lib.ptr(dout), B, T, Di, N, None, *(_lib.ptr(t) for t in bufs[1:]),
                                                 need, st))

    def torch_fwd():
        with torch.no_grad():
            return mt.selective_scan(*ins, m)

    def torch_bwd():
        leaves = [t.detach().requires_grad_() for t in ins]
        return torch.autograd.grad(mt.selective_scan(*leaves, m), leaves, dout)

    got, ref = selective_scan(*ins, start, dout=dout), (torch_fwd(),) + tuple(torch_bwd())
    names = ("out", "du", "ddt", "dz", "dA", "dBm", "dCm", "dD")
    diff = {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip(names, got, ref)}
    if max(diff.values()) > 1e-5:
        raise SystemExit(f"T {T} d_inner {Di} N {N}: the HIP scan and the torch loop differ: {diff}")
    del got, ref
    out = {"T": T, "d_inner": Di, "d_state": N, "batch": B, "max_rel_diff_vs_torch_loop": diff}
    out.update(alternate({"hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_bwd": hip_bwd, "torch_bwd": torch_bwd},
                         {"hip_fwd": n, "torch_fwd": 1, "hip_bwd": n, "torch_bwd": 1}, args))
    out["hip_fwd_speedup_vs_torch_loop"] = round(out["torch_fwd_us_median"] / out["hip_fwd_us_median"], 1)
    out["hip_fwd_bwd_speedup_vs_torch_loop"] = round(out["torch_bwd_us_median"] / out["hip_bwd_us_median"], 1)
    out["peak_mb_above_resident"] = {"hip_bwd": peak_mb(lambda: selective_scan(*ins, start, dout=dout)),
                                     "torch_bwd": peak_mb(torch_bwd)}
    return out


class TorchMamba4Rec(torch.nn.Module):
    """include/hiprec.h's Mamba4Rec as torch ops (tests/mamba4rec_torch.py's forward); parameters keyed like the engine's."""

    def __init__(self, w, cfg):
        super().__init__()
        self.names = list(w)
        self.params = torch.nn.ParameterList(torch.nn.Parameter(v.clone()) for v in w.values())
        self.cfg = cfg

    def forward(self, seq, pos, neg):
        import mamba4rec_torch as mt

        w = dict(zip(self.names, self.params))
        f, E = mt.forward(w, self.cfg, seq)[:, -1], w["item_emb.weight"]
        return (F.softplus(-(f * E[pos]).sum(-1)) + F.softplus((f * E[neg]).sum(-1))).mean()


def measure_step(args, hp, dev):
    torch.manual_seed(0)
    T, D = STEP["T"], STEP["D"]
    model = {"n_users": B, "n_items": I, "emb_dim": D, "maxlen": T, "num_blocks": NB, "dropout_rate": 0.0, "batch_size": B,
             "lr": LR, "optimizer": "adam", "device_str": "cuda:0", "d_state": STEP["N"], "d_conv": STEP["Kc"],
             "expand": STEP["expand"]}
    rng = np.random.default_rng(1)
    batches = []
    for _ in range(args.steps):
        seq = rng.integers(1, I + 1, (B, T))
        seq[np.arange(T)[None, :] < rng.integers(0, T // 2, B)[:, None]] = 0      # left padding of mixed lengths
        pos, neg = rng.integers(1, I + 1, B), rng.integers(1, I + 1, B)
        batches.append(tuple(torch.from_numpy(a).to(dev) for a in (seq, pos, neg)))
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.Mamba4RecEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_bench_runs"}})
    w0 = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
    step_batches = [(None,) + b for b in batches]
    first = {"hip": float(eng.backward_only(step_batches[0])[0])}
    ref = TorchMamba4Rec(w0, model).to(dev)
    opt = torch.optim.Adam(ref.parameters(), lr=LR)
    with torch.no_grad():
        first["torch"] = float(ref(*batches[0]))
    if abs(first["torch"] - first["hip"]) > 1e-4 * abs(first["torch"]):
        raise SystemExit(f"the two sides do not compute the same loss from the same weights: {first}")

    def hip():
        for b in step_batches:
            eng._enqueue_grad(b)
            eng._enqueue_opt()

    def torch_steps():
        for b in batches:
            opt.zero_grad()
            ref(*b).backward()
            opt.step()

    out = {"maxlen": T, "emb_dim": D, **{k: v for k, v in STEP.items() if k not in "TD"}, "first_batch_loss": first}
    n = len(batches)
    step = alternate({"hip": hip, "torch": torch_steps}, {"hip": n, "torch": n}, args)
    out.update({k.replace("_us", "_us_per_step"): v for k, v in step.items()})
    out["hip_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
    out["workspace_mb"] = round(eng.model._ws.numel() / 1e6, 1)
    out["peak_mb_above_resident"] = {"hip": peak_mb(hip), "torch": peak_mb(torch_steps)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--stage-iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mamba4rec.py measures on the GPU; no GPU found and there is no CPU timing path")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_mamba4rec.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "n_items": I, "batch": B, "num_blocks": NB, "optimizer": "adam",
           "steps_per_sample": args.steps, "stage_calls_per_sample": args.stage_iters, "repeats": args.repeats,
           "scan_stage": [measure_stage(T, Di, N, args, dev) for T, Di, N in STAGE_SHAPES], "step": measure_step(args, hp, dev)}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
