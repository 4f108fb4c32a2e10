"""Measure DIN on the GPU: the activation-unit stage of csrc/din.hip (forward + backward) against the naive concatenated
torch form with autograd and against the same algebra (the ``U + V + Wp`` split) in torch ops, a scoring call, and the whole
Adam step of the HIP engine against the same step in torch ops, all on the same card.

    python tools/bench_din.py [--steps 3] [--warmup 2] [--repeats 5] [--out profiles/din_step.json]

43 097 items, D 64, att_hidden [80, 40], dnn_hidden [200, 80], sigmoid unit, Dice tower.
  stage     ``DIN.attention_stage`` with ``dpooled`` (prep, U and V through the grouped GEMM, the fused forward, the fused
            backward, its GEMM group, fold and unfold) vs ``tests/din_torch.attention`` + ``torch.autograd.grad`` (``naive``) and
            vs the split form in torch ops (``split``), at B 128 / 1024, T 50 / 200, C 4; every side produces ``pooled``, the
            unit's parameter gradients, ``d e`` and ``d q``
  scoring   ``DINEngine.predict`` vs the restatement in eval mode under ``no_grad`` at B 128, T 50, C 100, forward only
  step      ``hiprec_din_grad`` + the dense optimizer sweep vs the restatement's ops + BCE + ``torch.optim.Adam``
One sample is the HIP-event time of a pass divided by its number of calls; the sides alternate ``--repeats`` times in one
process after ``--warmup`` passes each; medians with their spread.  Peak memory is ``torch.cuda.max_memory_allocated`` of one
pass above what was resident before it.  Before anything is timed the sides must agree to 1e-4 of each output's scale.  Needs
a GPU.
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
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_comirec import alternate, peak_mb, rel      # noqa: E402

I, D, LR = 43097, 64, 1e-3
SHAPES = [(B, T, 4) for T in (50, 200) for B in (128, 1024)]


def split_attention(e, q, mask, w):
    """The kernel's algebra in torch ops: the first layer as U + V + (q * e) Wp^T."""
    Wq, We, Wd, Wp = w["att.0.weight"].split(D, dim=1)
    U = e @ (We - Wd).T + w["att.0.bias"]
    V = q @ (Wq + Wd).T
    h = torch.sigmoid(U[:, None] + V[:, :, None] + (q[:, :, None, :] * e[:, None]) @ Wp.T)
    h = torch.sigmoid(h @ w["att.1.weight"].T + w["att.1.bias"])
    a = (h @ w["att.2.weight"].T + w["att.2.bias"])[..., 0] / D ** 0.5 * mask[:, None, :]
    return torch.einsum("bct,btd->bcd", a, e)


def make_engine(hp, B, T):
    model = {"n_items": I, "emb_dim": D, "maxlen": T, "batch_size": B, "lr": LR, "optimizer": "adam", "device_str": "cuda:0"}
    with contextlib.redirect_stdout(io.StringIO()):
        return hp.DINEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_bench_runs"}})


def measure(B, T, C, args, hp, dev):
    import din_torch as dt

    torch.manual_seed(B + T)
    eng = make_engine(hp, B, T)
    m = eng.model
    with torch.no_grad():
        m.item_emb.weight.data.mul_(5.0)      # rows of order 0.5, the fixtures' scale
    cfg = {"dnn_hidden": m.dnn_hidden}
    w0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(B * 1000 + T)
    batches = []
    for _ in range(args.steps):
        seq = rng.integers(1, I + 1, (B, T))
        seq[np.arange(T)[None, :] < rng.integers(0, T // 2, B)[:, None]] = 0      # left padding of mixed lengths
        cand, label = rng.integers(1, I + 1, (B, C)), (rng.random((B, C)) < 0.25).astype(np.float32)
        batches.append(tuple(torch.from_numpy(a).to(dev) for a in (seq, cand, label)))
    seq, cand, _ = batches[0]
    n = args.stage_iters
    E = m.item_emb.weight.data
    e, q, mask = E[seq].contiguous(), E[cand].contiguous(), seq != 0
    dpooled = torch.randn(B, C, D, device=dev, generator=torch.Generator(device=dev).manual_seed(7))
    names = [k for k in w0 if k.startswith("att.") and not k.endswith("alpha")]

    def hip_stage():
        for _ in range(n):
            out = m.attention_stage(e, q, mask, dpooled)
        return out

    def torch_stage(fn):
        el, ql = e.detach().requires_grad_(), q.detach().requires_grad_()
        wl = {k: w0[k].detach().requires_grad_() for k in names}
        pooled = fn(el, ql, wl)
        return pooled, torch.autograd.grad(pooled, [el, ql] + [wl[k] for k in names], dpooled)

    def naive():
        return torch_stage(lambda el, ql, wl: dt.attention(el, ql, mask, {**w0, **wl}, "sigmoid")[0])

    def split():
        return torch_stage(lambda el, ql, wl: split_attention(el, ql, mask.float(), wl))

    pooled, _, g, de, dq = hip_stage()
    diff = {}
    for side, fn in (("naive", naive), ("split", split)):
        p_t, grads_t = fn()
        diff[side] = max([rel(pooled, p_t), rel(de, grads_t[0]), rel(dq, grads_t[1])] +
                         [rel(g[k], gt) for k, gt in zip(names, grads_t[2:])])
    if max(diff.values()) > 1e-4:
        raise SystemExit(f"B {B} T {T}: the HIP stage and the torch ops differ: {diff}")
    out = {"batch": B, "T": T, "C": C, "tiles": m.tiles(), "stage_max_rel_diff_vs_torch_ops": diff}
    sides = {"hip_stage": hip_stage, "torch_naive_stage": naive, "torch_split_stage": split}
    out.update(alternate(sides, {k: n if k.startswith("hip") else 1 for k in sides}, args))
    out["stage_speedup_vs_naive"] = round(out["torch_naive_stage_us_median"] / out["hip_stage_us_median"], 2)
    out["stage_speedup_vs_split"] = round(out["torch_split_stage_us_median"] / out["hip_stage_us_median"], 2)
    out["stage_peak_mb_above_resident"] = {"hip": peak_mb(lambda: m.attention_stage(e, q, mask, dpooled)),
                                           "torch_naive": peak_mb(naive), "torch_split": peak_mb(split)}

    # the whole step
    params = {k: torch.nn.Parameter(t.clone()) for k, t in w0.items() if "running" not in k}
    run = {k: t.clone() for k, t in w0.items() if "running" in k}
    opt = torch.optim.Adam(params.values(), lr=LR)

    def torch_loss(b):
        z, live = dt.logits(params, cfg, b[0], b[1], run, True)
        return F.binary_cross_entropy_with_logits(z.reshape(-1)[live], b[2].reshape(-1)[live])

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


def scoring(args, hp, dev, B=128, T=50, C=100):
    import din_torch as dt

    torch.manual_seed(1)
    eng = make_engine(hp, B, T)
    m = eng.model
    with torch.no_grad():
        m.item_emb.weight.data.mul_(5.0)
    w = dict(m.state_dict())
    rng = np.random.default_rng(3)
    seq, cand = (torch.from_numpy(rng.integers(1, I + 1, s)).to(dev) for s in ((B, T), (B, C)))
    n = args.stage_iters

    def hip():
        for _ in range(n):
            z = eng.predict(seq, cand)
        return z

    def torch_ops():
        with torch.no_grad():
            return dt.logits(w, {"dnn_hidden": m.dnn_hidden}, seq, cand, w, False)[0]

    diff = rel(hip(), torch_ops())
    if diff > 1e-4:
        raise SystemExit(f"scoring: HIP and torch ops differ by {diff}")
    out = {"batch": B, "T": T, "C": C, "max_rel_diff_vs_torch_ops": diff}
    out.update(alternate({"hip": hip, "torch": torch_ops}, {"hip": n, "torch": 1}, args))
    out["speedup_vs_torch_ops"] = round(out["torch_us_median"] / out["hip_us_median"], 2)
    out["peak_mb_above_resident"] = {"hip": peak_mb(lambda: eng.predict(seq, cand)), "torch": peak_mb(torch_ops)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--stage-iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_din.py measures on the GPU; no GPU found and there is no CPU timing path")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_din.py", "device": torch.cuda.get_device_name(0), "source_hash": __graft_entry__.source_hash(),
           "n_items": I, "emb_dim": D, "att_hidden": [80, 40], "dnn_hidden": [200, 80], "optimizer": "adam",
           "steps_per_sample": args.steps, "stage_calls_per_sample": args.stage_iters, "repeats": args.repeats,
           "shapes": [measure(B, T, C, args, hp, dev) for B, T, C in SHAPES], "scoring": scoring(args, hp, dev)}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
