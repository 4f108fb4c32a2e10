"""Measure HSTU on the GPU: the attention stage alone against the same stage as torch ops with autograd, forward and
backward, and the whole training step of the HIP engine against the same model written as torch ops.

    python tools/bench_hstu.py [--steps 4] [--warmup 3] [--repeats 7] [--out profiles/hstu_step.json]

Attention stage (B 128; T in 50, 200, 256; (H, dqk, dv) in (2, 32, 32), (8, 16, 16); maxlen = T, 128 buckets),
``--stage-iters`` calls per sample:
  hip_fwd    hiprec_hstu_attention, AV only: one launch, no [B, H, T, T] tensor
  torch_fwd  einsum -> + pos_w gather + ts_w gather -> silu / N -> mask -> einsum, no autograd
  hip_bwd    hiprec_hstu_attention from dAV: dq, dk, dv, d pos_w, d ts_w (two kernels + the fold of the bias slabs)
  torch_bwd  torch.autograd.grad of the retained torch_fwd graph: d act, d pos_w, d ts_w
  sas_fwd    sanity line: SASRec's softmax attention forward (hiprec_sasrec_attention) at the same (B, T, H, head width)
  sas_bwd    its two backward kernels
Whole step (43 097 items, B 128, two blocks, Adam lr 1e-3, no dropout) at T 50 / D 64 and T 200 / D 128:
  hip        HSTUEngine's launches (hiprec_hstu_grad + the dense optimizer sweep), no host sync
  torch      the same model as torch ops with autograd and torch.optim.Adam, fp32, TF32 off
with the peak device memory of each side.  One sample is the HIP-event time of a pass divided by its number of calls; the
sides alternate ``--repeats`` times in one process after ``--warmup`` passes each, and the medians are reported with their
spread.  Before anything is timed the stage's two forms must agree to 1e-4 of each output's scale and the two steps' first
losses to 1e-4.  Needs a GPU.
"""
import argparse
import contextlib
import io
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

I, B, NB, NBK, LR = 43097, 128, 2, 128, 1e-3
STAGE_SHAPES = [(T, H, d, d) for T in (50, 200, 256) for H, d in ((2, 32), (8, 16))]
STEP_SHAPES = {"t50_d64": dict(T=50, D=64, H=2, dq=32, dv=32), "t200_d128": dict(T=200, D=128, H=2, dq=32, dv=32)}


def torch_buckets(ts):
    te = torch.cat([ts[:, 1:], ts[:, -1:]], 1)
    d = (te[:, :, None] - ts[:, None, :]).abs().clamp(min=1).double()
    return torch.clamp(torch.floor(torch.log(d) / 0.301), max=NBK).long()


def torch_attention(act, pos_w, ts_w, seq, bkt, H, dq, dv, N):
    Bn, T, _ = act.shape
    _, v, q, k = act.split([H * dv, H * dv, H * dq, H * dq], -1)
    S = torch.einsum("bihd,bjhd->bhij", q.reshape(Bn, T, H, dq), k.reshape(Bn, T, H, dq))
    t = torch.arange(T, device=act.device)
    S = S + pos_w[N - 1 + t[None, :] - t[:, None]] + ts_w[bkt][:, None]
    valid = seq != 0
    mask = (t[None, :] <= t[:, None])[None] & valid[:, :, None] & valid[:, None, :]
    A = F.silu(S) / N * mask[:, None].to(S.dtype)
    return torch.einsum("bhij,bjhd->bihd", A, v.reshape(Bn, T, H, dv)).reshape(Bn, T, H * dv)


class TorchHSTU(torch.nn.Module):
    """include/hiprec.h's HSTU as torch ops; parameters keyed like the engine's state_dict."""

    def __init__(self, w, D, H, dq, dv, N):
        super().__init__()
        self.names = list(w)
        self.params = torch.nn.ParameterList(torch.nn.Parameter(v.clone()) for v in w.values())
        self.dims = (D, H, dq, dv, N)

    def forward(self, seq, ts, pos, neg):
        w = dict(zip(self.names, self.params))
        D, H, dq, dv, N = self.dims
        E = w["item_emb.weight"]
        valid = (seq != 0).float()[..., None]
        bkt = torch_buckets(ts)
        x = (E[seq] * math.sqrt(D) + w["pos_emb.weight"][None]) * valid
        for b in range(NB):
            p = f"blocks.{b}."
            act = F.silu(F.layer_norm(x, (D,), w[p + "norm.weight"], w[p + "norm.bias"], 1e-6) @ w[p + "uvqk"])
            av = torch_attention(act, w[p + "pos_w"], w[p + "ts_w"], seq, bkt, H, dq, dv, N)
            y = F.layer_norm(av, (H * dv,), None, None, 1e-6) * act[..., :H * dv]
            x = (x + F.linear(y, w[p + "o.weight"], w[p + "o.bias"])) * valid
        f = F.layer_norm(x, (D,), w["last_norm.weight"], w["last_norm.bias"], 1e-6)
        lab = pos != 0
        terms = F.softplus(-(f * E[pos]).sum(-1)) + F.softplus((f * E[neg]).sum(-1))
        return terms[lab].sum() / lab.sum()


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


def random_batch(rng, T, dev):
    seq = rng.integers(1, I + 1, (B, T))
    seq[np.arange(T)[None, :] < rng.integers(0, T // 2, B)[:, None]] = 0      # left padding of mixed lengths
    ts = np.where(seq != 0, 1_600_000_000 + np.cumsum(rng.integers(1, 100000, (B, T)), 1), 0)
    pos, neg = (np.where(seq != 0, rng.integers(1, I + 1, (B, T)), 0) for _ in range(2))
    return tuple(torch.from_numpy(a).to(dev) for a in (seq, ts, pos, neg))


def measure_stage(T, H, dq, dv, args, dev):
    from beta_recsys_amd import _lib
    from beta_recsys_amd.hstu import attention_stage, bucket_bytes

    lib, st, n, N = _lib.load(), _lib.stream_ptr(dev), args.stage_iters, T
    gen = torch.Generator(device=dev).manual_seed(T * 1000 + H)
    seq, ts, _, _ = random_batch(np.random.default_rng(T + H), T, dev)
    act = F.silu(torch.randn(B, T, 2 * H * (dq + dv), device=dev, generator=gen))
    pos_w = 0.5 * torch.randn(2 * N - 1, device=dev, generator=gen)
    ts_w = 0.5 * torch.randn(NBK + 1, device=dev, generator=gen)
    dav = torch.randn(B, T, H * dv, device=dev, generator=gen)
    bytes_, bkt = bucket_bytes(ts, seq, NBK), torch_buckets(ts)
    av, dact, dpos, dts = torch.empty_like(dav), torch.zeros_like(act), torch.zeros_like(pos_w), torch.zeros_like(ts_w)
    scratch = torch.empty(lib.hiprec_hstu_attention_scratch_floats(B, T, H, NBK), device=dev)

    def call(with_av, with_dav):
        p = _lib.ptr
        _lib.check(lib.hiprec_hstu_attention(p(act), p(pos_w), p(ts_w), p(seq), p(bytes_), p(dav) if with_dav else None, B,
                                             T, H, dq, dv, N, NBK, p(av) if with_av else None, p(dact), p(dpos), p(dts),
                                             p(scratch), scratch.numel(), st))

    def hip_fwd():
        for _ in range(n):
            call(True, False)

    def hip_bwd():
        for _ in range(n):
            call(False, True)

    def torch_fwd():
        with torch.no_grad():
            for _ in range(n):
                torch_attention(act, pos_w, ts_w, seq, bkt, H, dq, dv, N)

    # the sanity line: SASRec's attention kernels on q | k | v of the same head width (dqk == dv in every shape here)
    Dm = H * dq
    qkv = torch.randn(B * T, 3 * Dm, device=dev, generator=gen)
    s_out, s_do, s_dqkv = (torch.empty(B * T, n_, device=dev) for n_ in (Dm, Dm, 3 * Dm))
    s_do.normal_(generator=gen)
    s_lse, s_delta = torch.empty(B * H * T, device=dev), torch.empty(B * H * T, device=dev)

    def sas(with_do):
        p = _lib.ptr
        _lib.check(lib.hiprec_sasrec_attention(p(qkv), p(s_do) if with_do else None, B, T, H, Dm, p(s_out), p(s_lse),
                                               p(s_delta), p(s_dqkv), st))

    def sas_fwd():
        for _ in range(n):
            sas(False)

    def sas_bwd():
        for _ in range(n):
            sas(True)

    leaves = [t.clone().requires_grad_() for t in (act, pos_w, ts_w)]
    graph = torch_attention(*leaves, seq, bkt, H, dq, dv, N)

    def torch_bwd():
        for _ in range(n):
            torch.autograd.grad(graph, leaves, dav, retain_graph=True)

    got = attention_stage(act, pos_w, ts_w, seq, bytes_, H, dq, dv, N, dav=dav)
    gact, gpos, gts = torch.autograd.grad(graph, leaves, dav, retain_graph=True)
    _, gv, gq, gk = gact.split([H * dv, H * dv, H * dq, H * dq], -1)
    ref = (graph.detach(), gq, gk, gv, gpos, gts)
    diff = {k: float((a - b).abs().max() / b.abs().max()) for k, a, b in zip(("av", "dq", "dk", "dv", "dpos_w", "dts_w"), got, ref)}
    if max(diff.values()) > 1e-4:
        raise SystemExit(f"T {T} H {H}: the HIP attention and the torch ops differ: {diff}")
    out = {"T": T, "H": H, "dqk": dq, "dv": dv, "batch": B, "max_rel_diff_vs_torch_ops": diff}
    sas_fwd()
    out.update(alternate({"hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "hip_bwd": hip_bwd, "torch_bwd": torch_bwd,
                          "sas_fwd": sas_fwd, "sas_bwd": sas_bwd}, n, args))
    out["hip_fwd_vs_sasrec_attention"] = round(out["sas_fwd_us_median"] / out["hip_fwd_us_median"], 2)
    out["hip_bwd_vs_sasrec_attention"] = round(out["sas_bwd_us_median"] / out["hip_bwd_us_median"], 2)
    out["hip_fwd_speedup_vs_torch_ops"] = round(out["torch_fwd_us_median"] / out["hip_fwd_us_median"], 2)
    out["hip_bwd_speedup_vs_torch_ops"] = round(out["torch_bwd_us_median"] / out["hip_bwd_us_median"], 2)
    return out


def measure_step(name, T, D, H, dq, dv, args, hp, dev):
    torch.manual_seed(0)
    cfg = {"model": {"n_users": B, "n_items": I, "emb_dim": D, "maxlen": T, "num_blocks": NB, "num_heads": H,
                     "attention_dim": dq, "linear_dim": dv, "num_buckets": NBK, "dropout_rate": 0.0, "batch_size": B,
                     "lr": LR, "optimizer": "adam", "device_str": "cuda:0"},
           "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    rng = np.random.default_rng(1)
    batches = [random_batch(rng, T, dev) for _ in range(args.steps)]
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.HSTUEngine(cfg)
    w0 = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
    step_batches = [(None,) + b for b in batches]
    first = {"hip": float(eng.backward_only(step_batches[0])[0])}
    ref = TorchHSTU(w0, D, H, dq, dv, T).to(dev)
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

    peak = {}
    for side, fn in (("hip", hip), ("torch", torch_steps)):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        peak[side] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
    out = {"maxlen": T, "emb_dim": D, "heads": H, "dqk": dq, "dv": dv, "first_batch_loss": first,
           "peak_mb_above_resident": peak, "workspace_mb": round(eng.model._ws.numel() / 1e6, 1)}
    step = alternate({"hip": hip, "torch": torch_steps}, len(batches), args)
    out.update({k.replace("_us", "_us_per_step"): v for k, v in step.items()})
    out["hip_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
    del eng
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--stage-iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_hstu.py measures on the GPU; no GPU found and there is no CPU timing path")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_hstu.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "n_items": I, "batch": B, "num_blocks": NB, "num_buckets": NBK,
           "optimizer": "adam", "steps_per_sample": args.steps, "stage_calls_per_sample": args.stage_iters,
           "repeats": args.repeats, "attention_stage": [measure_stage(*s, args, dev) for s in STAGE_SHAPES], "step": {}}
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
