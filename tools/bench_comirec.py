"""Measure ComiRec-DR on the GPU: each stage of csrc/comirec.hip against the same stage as torch ops on the same card, and the
whole training step of the HIP engine against the same step written as torch ops with autograd.

    python tools/bench_comirec.py [--steps 3] [--warmup 2] [--repeats 5] [--out profiles/comirec_step.json]

Shapes: (T 20, K 4, D 64) and (T 50, K 4, D 64), each at B 128 and B 1024; 43 097 items, 3 routing iterations, 1280 samples.
Stages, ``--stage-iters`` HIP calls per sample (one torch call per sample):
  project   hiprec_comirec_project (gather + T position GEMMs on the MFMA) vs ``E[seq]`` + ``torch.einsum``
  route     hiprec_comirec_route (one launch) vs the restatement's op sequence on the same ``uh`` under no_grad
  backward  hiprec_comirec_backward (row lists, d routing.weight, d e with its scatter) from ``d s``, ``k*`` and ``c`` vs
            autograd of the last weighted sum ``s[k*] = sum_t c[k*, t] (routing.weight[t, k*] E[seq[t]])``: torch's forward
            AND backward, the tape cannot be kept; both sides produce d routing.weight and d item_emb
Whole step (Adam lr 1e-3):
  hip       ComiRecEngine's launches (hiprec_comirec_grad + the dense optimizer sweep), no host sync
  torch     tests/comirec_torch.py's ops with autograd and torch.optim.Adam, fp32, TF32 off
One sample is the HIP-event time of a pass divided by its number of calls; the sides alternate ``--repeats`` times in one
process after ``--warmup`` passes each, and the medians are reported with their spread.  Peak memory is
``torch.cuda.max_memory_allocated`` of one pass above what was resident before it (the HIP side's workspace is a torch
tensor that stays resident, reported beside it).  Before anything is timed the two forms of a stage must agree to 1e-4 of each
output's scale and the two steps' first losses to 1e-4.  Not built for comparison: a routing form with ``uh`` held in LDS at
short ``T``, and a projection through hipBLASLt's grouped GEMM.  Needs a GPU.
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

I, R, S, LR = 43097, 3, 1280, 1e-3
SHAPES = [(B, T, 4, 64) for T in (20, 50) for B in (128, 1024)]


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


def torch_route(uh, mask, iters):
    """tests/comirec_torch.py's routing loop on a given ``uh [B, K, T, D]``."""
    b = uh.new_zeros(uh.shape[:3])
    for r in range(iters):
        c = torch.softmax(b, 1) * mask[:, None, :]
        s = (c[..., None] * uh).sum(2)
        n = (s * s).sum(-1, keepdim=True)
        v = s * n / (1 + n) / torch.sqrt(n + 1e-9)
        if r < iters - 1:
            b = b + (uh * v[:, :, None, :]).sum(-1)
    return v, c


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def measure(B, T, K, D, args, hp, dev):
    from beta_recsys_amd import _lib

    torch.manual_seed(B + T)
    model = {"n_items": I, "emb_dim": D, "maxlen": T, "num_interest": K, "routing_iters": R, "batch_size": B, "lr": LR,
             "optimizer": "adam", "device_str": "cuda:0"}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.ComiRecEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_bench_runs"}})
    m = eng.model
    with torch.no_grad():      # the fixtures' scale: the routing logits stay of order 1
        m.item_emb.weight.data.mul_(0.5)
        m.routing.weight.data.mul_(D ** -0.5)
    w0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(B * 1000 + T)
    batches = []
    for _ in range(args.steps):
        seq = rng.integers(1, I + 1, (B, T))
        seq[np.arange(T)[None, :] < rng.integers(0, T // 2, B)[:, None]] = 0      # left padding of mixed lengths
        batches.append(tuple(torch.from_numpy(a).to(dev) for a in (seq, rng.integers(1, I + 1, B), rng.integers(1, I + 1, S))))
    seq = batches[0][0]
    lib, st, n = _lib.load(), _lib.stream_ptr(dev), args.stage_iters
    E, W = m.item_emb.weight.data, m.routing.weight.data
    seq_flat, mask = seq.reshape(-1).contiguous(), (seq != 0).float()
    uh = torch.empty((B, T, K, D), device=dev)
    live = torch.empty((B, T), dtype=torch.uint8, device=dev)
    v, c, nsq = torch.empty((B, K, D), device=dev), torch.empty((B, K, T), device=dev), torch.empty((B, K), device=dev)
    stats = m._device_stats()

    def hip_project():
        for _ in range(n):
            _lib.check(lib.hiprec_comirec_project(_lib.ptr(W), _lib.ptr(E), I + 1, _lib.ptr(seq_flat), None, B, T, K, D,
                                                  _lib.ptr(uh), _lib.ptr(live), _lib.ptr(stats), st))

    def torch_project():
        return torch.einsum("tkij,btj->btki", W, E[seq])

    def hip_route():
        for _ in range(n):
            _lib.check(lib.hiprec_comirec_route(_lib.ptr(uh), _lib.ptr(live), B, T, K, D, R, _lib.ptr(v), _lib.ptr(c),
                                                _lib.ptr(nsq), st))

    def torch_route_call():
        with torch.no_grad():
            return torch_route(uh_t, mask, R)

    hip_project()
    uh_t = torch_project().permute(0, 2, 1, 3).contiguous()      # [B, K, T, D], the restatement's layout
    hip_route()
    v_t, c_t = torch_route_call()
    diff = {"uh": rel(uh.permute(0, 2, 1, 3), uh_t), "interests": rel(v, v_t), "c": rel(c, c_t)}

    gen = torch.Generator(device=dev).manual_seed(7)
    ds = torch.randn(B, D, device=dev, generator=gen)
    kstar = torch.randint(0, K, (B,), device=dev, generator=gen).to(torch.int32)
    lists = torch.empty(8 + K * B, dtype=torch.int32, device=dev)
    g_flat = torch.zeros_like(m.flat)
    pick = kstar.long()

    def hip_backward():
        for _ in range(n):
            _lib.check(lib.hiprec_comirec_backward(ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(g_flat),
                                                   _lib.ptr(seq_flat), _lib.ptr(c), _lib.ptr(ds), _lib.ptr(kstar), B,
                                                   _lib.ptr(lists), st))

    def torch_backward():
        El, Wl = E.detach().requires_grad_(), W.detach().requires_grad_()
        uh_l = torch.einsum("tkij,btj->bkti", Wl, El[seq])
        s = (c[..., None] * uh_l).sum(2)[torch.arange(B, device=dev), pick]
        return torch.autograd.grad(s, [El, Wl], ds)

    g_flat.zero_()
    _lib.check(lib.hiprec_comirec_backward(ctypes.byref(m.shape), _lib.ptr(m.flat), _lib.ptr(g_flat), _lib.ptr(seq_flat),
                                           _lib.ptr(c), _lib.ptr(ds), _lib.ptr(kstar), B, _lib.ptr(lists), st))
    gE, gW = torch_backward()
    got = m.views(g_flat)
    diff["d_item_emb"], diff["d_routing_weight"] = rel(got["item_emb.weight"], gE), rel(got["routing.weight"], gW)
    if max(diff.values()) > 1e-4:
        raise SystemExit(f"B {B} T {T}: the HIP stages and the torch ops differ: {diff}")
    del gE, gW

    out = {"batch": B, "T": T, "K": K, "D": D, "max_rel_diff_vs_torch_ops": diff}
    sides = {"hip_project": hip_project, "torch_project": torch_project, "hip_route": hip_route,
             "torch_route": torch_route_call, "hip_backward": hip_backward, "torch_backward": torch_backward}
    out.update(alternate(sides, {k: n if k.startswith("hip") else 1 for k in sides}, args))
    for stage in ("project", "route", "backward"):
        out[f"{stage}_speedup_vs_torch_ops"] = round(out[f"torch_{stage}_us_median"] / out[f"hip_{stage}_us_median"], 2)

    # the whole step
    import comirec_torch as ct

    params = {k: torch.nn.Parameter(t.clone()) for k, t in w0.items()}
    opt = torch.optim.Adam(params.values(), lr=LR)

    def torch_loss(b):
        sq, target, samples = b
        Et = params["item_emb.weight"]
        vv, _ = ct.route(Et[sq], params["routing.weight"], sq != 0, R)
        tg = Et[target]
        ks = (vv * tg[:, None, :]).sum(-1).detach().argmax(1)
        ro = vv[torch.arange(B, device=dev), ks]
        z0 = (ro * tg).sum(-1)
        zj = (ro @ Et[samples].T).masked_fill(samples[None, :] == target[:, None], -float("inf"))
        return (torch.logsumexp(torch.cat([z0[:, None], zj], 1), 1) - z0).mean()

    m.load_state_dict(w0)
    first = {"hip": float(eng.backward_only(batches[0])[0])}
    with torch.no_grad():
        first["torch"] = float(torch_loss(batches[0]))
    if abs(first["torch"] - first["hip"]) > 1e-4 * abs(first["torch"]):
        raise SystemExit(f"the two sides do not compute the same loss from the same weights: {first}")

    def hip():
        for b in batches:
            eng._enqueue_grad(b)
            eng._enqueue_opt()

    def torch_steps():
        for b in batches:
            opt.zero_grad()
            torch_loss(b).backward()
            opt.step()

    step = alternate({"hip": hip, "torch": torch_steps}, {"hip": len(batches), "torch": len(batches)}, args)
    out["step"] = {k.replace("_us", "_us_per_step"): x for k, x in step.items()}
    out["step"]["first_batch_loss"] = first
    out["step"]["hip_speedup_vs_torch_ops"] = round(step["torch_us_median"] / step["hip_us_median"], 2)
    out["step"]["workspace_mb"] = round(m._ws.numel() / 1e6, 1)
    out["step"]["peak_mb_above_resident"] = {"hip": peak_mb(hip), "torch": peak_mb(torch_steps)}
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
        raise SystemExit("tools/bench_comirec.py measures on the GPU; no GPU found and there is no CPU timing path")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_comirec.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "n_items": I, "routing_iters": R, "n_sample": S, "optimizer": "adam",
           "steps_per_sample": args.steps, "stage_calls_per_sample": args.stage_iters, "repeats": args.repeats,
           "shapes": [measure(B, T, K, D, args, hp, dev) for B, T, K, D in SHAPES]}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
