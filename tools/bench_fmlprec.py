"""Measure FMLP-Rec on the GPU: the filter stage alone against the same stage as ``torch.fft`` ops, forward and backward,
and the whole training step of the HIP engine against the same model written as torch ops.

    python tools/bench_fmlprec.py [--steps 4] [--warmup 3] [--repeats 7] [--out profiles/fmlprec_step.json]

Filter stage (B 256; T in 50, 200, 256; D in 64, 128), ``--stage-iters`` calls per sample:
  hip_fwd    hiprec_fmlprec_filter, y only: one launch, the spectrum stays in LDS
  torch_fwd  torch.fft.rfft(norm="ortho") -> * view_as_complex(W) -> torch.fft.irfft(norm="ortho"), no autograd
  hip_bwd    hiprec_fmlprec_filter from dy: dx and dW (the spectrum of x recomputed), kernel + the fold of its partials
  torch_bwd  torch.autograd.grad of the retained torch_fwd graph: dx and dW
Whole step (43 097 items, B 256, two blocks, ffn 4 D, Adam lr 1e-3, no dropout) at T 50 / D 64 and T 200 / D 128:
  hip        FMLPRecEngine's launches (hiprec_fmlprec_grad + the dense optimizer sweep), no host sync
  torch      the same model as torch ops with autograd (torch.fft, F.layer_norm eps 1e-12, F.gelu, softplus loss on the
             last position, torch.optim.Adam), fp32, TF32 off
One sample is the HIP-event time of a pass divided by its number of calls; the sides alternate ``--repeats`` times in one
process after ``--warmup`` passes each, and the medians are reported with their spread.  Before anything is timed the
stage's two forms must agree to 1e-5 of each output's scale and the two steps' first losses to 1e-4.  Needs a GPU.
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

I, B, NB, LR = 43097, 256, 2, 1e-3
STAGE_SHAPES = [(T, D) for T in (50, 200, 256) for D in (64, 128)]
STEP_SHAPES = {"t50_d64": dict(T=50, D=64), "t200_d128": dict(T=200, D=128)}


def torch_filter(x, weight):
    spectrum = torch.fft.rfft(x, dim=1, norm="ortho") * torch.view_as_complex(weight)[None]
    return torch.fft.irfft(spectrum, n=x.shape[1], dim=1, norm="ortho")


class TorchFMLPRec(torch.nn.Module):
    """include/hiprec.h's FMLP-Rec as torch ops; parameters keyed like the engine's state_dict."""

    def __init__(self, w, D):
        super().__init__()
        self.names = list(w)
        self.params = torch.nn.ParameterList(torch.nn.Parameter(v.clone()) for v in w.values())
        self.D = D

    def forward(self, seq, pos, neg):
        w, D = dict(zip(self.names, self.params)), self.D
        ln = lambda v, p: F.layer_norm(v, (D,), w[p + ".weight"], w[p + ".bias"], 1e-12)      # noqa: E731
        E = w["item_emb.weight"]
        x = ln(F.embedding(seq, E, padding_idx=0) + w["pos_emb.weight"][None], "emb_norm")
        for b in range(NB):
            p = f"blocks.{b}."
            h = ln(x + torch_filter(x, w[p + "filter.complex_weight"]), p + "norm1")
            z = F.linear(F.gelu(F.linear(h, w[p + "fc1.weight"], w[p + "fc1.bias"])), w[p + "fc2.weight"], w[p + "fc2.bias"])
            x = ln(h + z, p + "norm2")
        f = x[:, -1]
        return (F.softplus(-(f * E[pos]).sum(-1)) + F.softplus((f * E[neg]).sum(-1))).mean()


def event_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def alternate(sides, n, args):
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(event_us(fn, n))
    out = {}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us"] = [round(x, 1) for x in v]
        out[f"{k}_us_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
    return out


def measure_stage(T, D, args, dev):
    from beta_recsys_amd import _lib
    from beta_recsys_amd.fmlprec import twiddle_table

    lib, st, n = _lib.load(), _lib.stream_ptr(dev), args.stage_iters
    gen = torch.Generator(device=dev).manual_seed(T * 1000 + D)
    x = torch.randn(B, T, D, device=dev, generator=gen)
    wt = 0.3 * torch.randn(T // 2 + 1, D, 2, device=dev, generator=gen)
    dy = torch.randn(B, T, D, device=dev, generator=gen)
    tw = twiddle_table(T, dev)
    y, dx, dw = torch.empty_like(x), torch.empty_like(x), torch.empty_like(wt)
    scratch = torch.empty(lib.hiprec_fmlprec_filter_scratch_floats(B, T, D), device=dev)

    def hip_fwd():
        for _ in range(n):
            _lib.check(lib.hiprec_fmlprec_filter(_lib.ptr(x), _lib.ptr(wt), _lib.ptr(tw), None, 1.0, None, B, T, D,
                                                 _lib.ptr(y), None, None, None, 0, st))

    def hip_bwd():
        for _ in range(n):
            _lib.check(lib.hiprec_fmlprec_filter(_lib.ptr(x), _lib.ptr(wt), _lib.ptr(tw), None, 1.0, _lib.ptr(dy), B, T, D,
                                                 None, _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(scratch), scratch.numel(), st))

    def torch_fwd():
        with torch.no_grad():
            for _ in range(n):
                torch_filter(x, wt)

    xg, wg = x.clone().requires_grad_(), wt.clone().requires_grad_()
    graph = torch_filter(xg, wg)

    def torch_bwd():
        for _ in range(n):
            torch.autograd.grad(graph, (xg, wg), dy, retain_graph=True)

    hip_fwd()
    hip_bwd()
    ref = (graph.detach(),) + torch.autograd.grad(graph, (xg, wg), dy, retain_graph=True)
    diff = {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip(("y", "dx", "dw"), (y, dx, dw), ref)}
    if max(diff.values()) > 1e-5:
        raise SystemExit(f"T {T} D {D}: the HIP filter and torch.fft differ: {diff}")
    out = {"T": T, "D": D, "batch": B, "max_rel_diff_vs_torch_fft": diff}
    out.update(alternate({"hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_bwd": hip_bwd, "torch_bwd": torch_bwd}, n, args))
    out["hip_fwd_speedup_vs_torch_fft"] = round(out["torch_fwd_us_median"] / out["hip_fwd_us_median"], 2)
    out["hip_bwd_speedup_vs_torch_fft"] = round(out["torch_bwd_us_median"] / out["hip_bwd_us_median"], 2)
    return out


def measure_step(name, T, D, args, hp, dev):
    torch.manual_seed(0)
    cfg = {"model": {"n_users": B, "n_items": I, "emb_dim": D, "maxlen": T, "num_blocks": NB, "dropout_rate": 0.0,
                     "batch_size": B, "lr": LR, "optimizer": "adam", "device_str": "cuda:0"},
           "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    rng = np.random.default_rng(1)
    batches = []
    for _ in range(args.steps):
        seq = rng.integers(1, I + 1, (B, T))
        seq[np.arange(T)[None, :] < rng.integers(0, T // 2, B)[:, None]] = 0      # left padding of mixed lengths
        pos, neg = rng.integers(1, I + 1, B), rng.integers(1, I + 1, B)
        batches.append(tuple(torch.from_numpy(a).to(dev) for a in (seq, pos, neg)))
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.FMLPRecEngine(cfg)
    w0 = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
    step_batches = [(None,) + b for b in batches]
    first = {"hip": float(eng.backward_only(step_batches[0])[0])}
    ref = TorchFMLPRec(w0, D).to(dev)
    opt = torch.optim.Adam(ref.parameters(), lr=LR)
    with torch.no_grad():
        first["torch"] = float(ref(*batches[0]))
    if abs(first["torch"] - first["hip"]) > 1e-4 * abs(first["torch"]):
        raise SystemExit(f"{name}: the two sides do not compute the same loss from the same weights: {first}")

    def hip():
        for b in step_batches:
            eng._enqueue_grad(b)
            eng._enqueue_opt()

    def torch_steps():
        for b in batches:
            opt.zero_grad()
            ref(*b).backward()
            opt.step()

    out = {"maxlen": T, "emb_dim": D, "first_batch_loss": first}
    step = alternate({"hip": hip, "torch": torch_steps}, len(batches), args)
    out.update({k.replace("_us", "_us_per_step"): v for k, v in step.items()})
    out["hip_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
    out["workspace_mb"] = round(eng.model._ws.numel() / 1e6, 1)
    del eng
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--stage-iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fmlprec.py measures on the GPU; no GPU found and there is no CPU timing path")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_fmlprec.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "n_items": I, "batch": B, "num_blocks": NB, "optimizer": "adam",
           "steps_per_sample": args.steps, "stage_calls_per_sample": args.stage_iters, "repeats": args.repeats,
           "filter_stage": [measure_stage(T, D, args, dev) for T, D in STAGE_SHAPES], "step": {}}
    for name, shape in STEP_SHAPES.items():
        out["step"][name] = measure_step(name, args=args, hp=hp, dev=dev, **shape)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
