"""Measure ETA on the GPU: the retrieval stage of csrc/eta.hip, the attention stage (forward and forward + backward), a
scoring call and the whole Adam step of the HIP engine, each against the same computation in torch ops with autograd on the
same card, and DIN's step at T 256 beside it as a time yardstick only (a different model).

    python tools/bench_eta.py [--steps 3] [--stage-iters 20] [--warmup 2] [--repeats 5] [--out profiles/eta_step.json]

43 097 items, D 64, 64 hash bits, top_k 48, 4 heads, dnn_hidden [200, 80], Dice tower, B 128 / 1024, T 1024 / 4096, C 4.
  retrieve  ``ETA.retrieve_stage`` vs a sign matmul, the distance as ``(m - <+-1 codes>) / 2``, ``topk`` of ``ham T + (T - 1 -
            t)`` (the same tie rule, so both sides must return the same ``sel``) and a sort of the positions
  stage     ``ETA.attention_stage`` without / with ``dv`` on that ``sel`` vs a gather of the selected rows, the projections,
            the masked softmax and ``torch.autograd.grad``; both sides produce ``v``, ``d e``, ``d q`` and the gradients of
            ``att.*``.  The stage entry returns ``d e [B, T, D]`` and clears it first, the whole step scatters compact rows
  scoring   ``ETAEngine.predict`` vs the torch form in eval mode under ``no_grad`` at B 128, T 1024, C 100
  step      ``hiprec_eta_grad`` + the dense optimizer sweep vs the torch form + ``torch.optim.Adam``
One sample is the HIP-event time of a pass divided by its number of calls; the sides alternate ``--repeats`` times in one
process after ``--warmup`` passes each; medians with their spread.  Peak memory is ``torch.cuda.max_memory_allocated`` of one
pass above what was resident before it.  Before anything is timed the sides must agree (``sel`` exactly, floats to 1e-4 of
each output's scale).  Needs a GPU.
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

I, D, M, K, H, LR = 43097, 64, 64, 48, 4, 1e-3
SHAPES = [(B, T, 4) for T in (1024, 4096) for B in (128, 1024)]
ATT = [f"att.{p}.{n}" for p in "qkvo" for n in ("weight", "bias")]


def make_engine(hp, B, T, cls="ETAEngine"):
    model = {"n_items": I, "emb_dim": D, "maxlen": T, "batch_size": B, "lr": LR, "optimizer": "adam", "device_str": "cuda:0",
             "hash_bits": M, "top_k": K, "num_heads": H}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = getattr(hp, cls)({"model": model, "system": {"run_dir": "/tmp/hiprec_bench_runs"}})
    with torch.no_grad():
        eng.model.item_emb.weight.data.mul_(5.0)      # rows of order 0.5, the fixtures' scale
    return eng


def torch_retrieve(e, q, live, hash_w):
    """``sel [B, C, K]`` int32 in torch ops: sign matmul, +-1 inner product, one ``topk`` with the kernel's tie rule."""
    T = e.shape[1]
    se, sq = (torch.where(x @ hash_w.T >= 0, 1.0, -1.0) for x in (e, q))
    key = (M - sq @ se.transpose(1, 2)) / 2 * T + (T - 1 - torch.arange(T, device=e.device))
    key = key.masked_fill(~live[:, None, :], float("inf"))
    val, at = key.topk(min(K, T), -1, largest=False)
    at = torch.where(torch.isinf(val), T, at).sort(-1)[0]
    return torch.where(at < T, at, -1).to(torch.int32)


def torch_attention(e, q, sel, w):
    B, C, k = sel.shape
    on = (sel >= 0)[..., None]
    rows = e[torch.arange(B, device=e.device)[:, None, None], sel.clamp(min=0).long()]      # [B, C, k, D]
    Qp, Kp, Vp = (F.linear(x, w[f"att.{p}.weight"], w[f"att.{p}.bias"]) for p, x in (("q", q), ("k", rows), ("v", rows)))
    s = (Qp.view(B, C, 1, H, D // H) * Kp.view(B, C, k, H, D // H)).sum(-1) / (D // H) ** 0.5
    p = torch.softmax(s.masked_fill(~on, -1e30), 2) * on
    o = (p[..., None] * Vp.view(B, C, k, H, D // H)).sum(2).reshape(B, C, D)
    return F.linear(o, w["att.o.weight"], w["att.o.bias"])


def torch_logits(w, run, seq, cand, train):
    E = w["item_emb.weight"]
    e, q = E[seq], E[cand]
    with torch.no_grad():
        sel = torch_retrieve(e, q, seq != 0, w["hash.weight"])
    v = torch_attention(e, q, sel, w)
    y = torch.cat([v, q, v * q], -1).reshape(-1, 3 * D)
    for l in range(2):
        y = F.linear(y, w[f"dnn.{l}.weight"], w[f"dnn.{l}.bias"])
        p = torch.sigmoid(F.batch_norm(y, run[f"dnn.{l}.running_mean"], run[f"dnn.{l}.running_var"], None, None, train, 0.1,
                                       1e-8))
        y = p * y + (1 - p) * w[f"dnn.{l}.alpha"] * y
    return F.linear(y, w["out.weight"], w["out.bias"]).view(cand.shape)


def measure(B, T, C, args, hp, dev):
    torch.manual_seed(B + T)
    eng = make_engine(hp, B, T)
    m = eng.model
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
    gen = torch.Generator(device=dev).manual_seed(7)
    E = m.item_emb.weight.data
    e, q, mask = E[seq].contiguous(), E[cand].contiguous(), seq != 0
    dv = torch.randn(B, C, D, device=dev, generator=gen)

    def loop(fn):
        def run():
            for _ in range(n):
                out = fn()
            return out
        return run

    sel = m.retrieve_stage(e, q, mask)[2]
    if not torch.equal(sel, torch_retrieve(e, q, mask, w0["hash.weight"])):
        raise SystemExit(f"B {B} T {T}: the HIP retrieval and the torch ops select different positions")

    def torch_stage():
        el, ql = e.detach().requires_grad_(), q.detach().requires_grad_()
        wl = {k: w0[k].detach().requires_grad_() for k in ATT}
        v = torch_attention(el, ql, sel, wl)
        return v, torch.autograd.grad(v, [el, ql] + [wl[k] for k in ATT], dv)

    v, de, dq, g = m.attention_stage(e, q, sel, dv)
    v_t, grads_t = torch_stage()
    diff = max([rel(v, v_t), rel(de, grads_t[0]), rel(dq, grads_t[1])] +
               [rel(g[k], gt) for k, gt in zip(ATT, grads_t[2:]) if k != "att.k.bias"])      # d att.k.bias is exactly zero
    if diff > 1e-4:
        raise SystemExit(f"B {B} T {T}: the HIP attention stage and the torch ops differ by {diff}")
    out = {"batch": B, "T": T, "C": C, "tiles": m.tiles(C), "stage_max_rel_diff_vs_torch_ops": diff}
    with torch.no_grad():
        sides = {"hip_retrieve": loop(lambda: m.retrieve_stage(e, q, mask)),
                 "torch_retrieve": lambda: torch_retrieve(e, q, mask, w0["hash.weight"]),
                 "hip_stage_fwd": loop(lambda: m.attention_stage(e, q, sel)),
                 "torch_stage_fwd": lambda: torch_attention(e, q, sel, w0)}
        out.update(alternate(sides, {k: n if k.startswith("hip") else 1 for k in sides}, args))
    sides = {"hip_stage": loop(lambda: m.attention_stage(e, q, sel, dv)), "torch_stage": torch_stage}
    out.update(alternate(sides, {"hip_stage": n, "torch_stage": 1}, args))
    for k in ("retrieve", "stage_fwd", "stage"):
        out[f"{k}_speedup"] = round(out[f"torch_{k}_us_median"] / out[f"hip_{k}_us_median"], 2)
    out["retrieve_peak_mb_above_resident"] = {"hip": peak_mb(lambda: m.retrieve_stage(e, q, mask)),
                                              "torch": peak_mb(lambda: torch_retrieve(e, q, mask, w0["hash.weight"]))}
    out["stage_peak_mb_above_resident"] = {"hip": peak_mb(lambda: m.attention_stage(e, q, sel, dv)), "torch": peak_mb(torch_stage)}
    del e, de

    # the whole step
    params = {k: torch.nn.Parameter(t.clone()) for k, t in w0.items() if "running" not in k and k != "hash.weight"}
    params["hash.weight"] = w0["hash.weight"]
    run = {k: t.clone() for k, t in w0.items() if "running" in k}
    opt = torch.optim.Adam([p for k, p in params.items() if k != "hash.weight"], lr=LR)

    def torch_loss(b):
        return F.binary_cross_entropy_with_logits(torch_logits(params, run, b[0], b[1], True), b[2])

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


def scoring(args, hp, dev, B=128, T=1024, C=100):
    torch.manual_seed(1)
    eng = make_engine(hp, B, T)
    w = dict(eng.model.state_dict())
    rng = np.random.default_rng(3)
    seq, cand = (torch.from_numpy(rng.integers(1, I + 1, s)).to(dev) for s in ((B, T), (B, C)))
    n = args.stage_iters

    def hip():
        for _ in range(n):
            z = eng.predict(seq, cand)
        return z

    def torch_ops():
        with torch.no_grad():
            return torch_logits(w, w, seq, cand, False)

    diff = rel(hip(), torch_ops())
    if diff > 1e-4:
        raise SystemExit(f"scoring: HIP and torch ops differ by {diff}")
    out = {"batch": B, "T": T, "C": C, "max_rel_diff_vs_torch_ops": diff}
    out.update(alternate({"hip": hip, "torch": torch_ops}, {"hip": n, "torch": 1}, args))
    out["speedup_vs_torch_ops"] = round(out["torch_us_median"] / out["hip_us_median"], 2)
    out["peak_mb_above_resident"] = {"hip": peak_mb(lambda: eng.predict(seq, cand)), "torch": peak_mb(torch_ops)}
    return out


def din_yardstick(args, hp, dev, T=256, C=4):
    """DIN's Adam step at its longest history: a time beside ETA's, not a comparison of like with like."""
    out = []
    for B in (128, 1024):
        eng = make_engine(hp, B, T, "DINEngine")
        rng = np.random.default_rng(B)
        batch = tuple(torch.from_numpy(a).to(dev) for a in (rng.integers(1, I + 1, (B, T)), rng.integers(1, I + 1, (B, C)),
                                                             (rng.random((B, C)) < 0.25).astype(np.float32)))

        def hip():
            for _ in range(args.steps):
                eng._enqueue_grad(batch)
                eng._enqueue_opt()

        out.append({"batch": B, "T": T, "C": C, **alternate({"din_step": hip}, {"din_step": args.steps}, args)})
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
        raise SystemExit("tools/bench_eta.py measures on the GPU; no GPU found and there is no CPU timing path")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_eta.py", "device": torch.cuda.get_device_name(0), "source_hash": __graft_entry__.source_hash(),
           "n_items": I, "emb_dim": D, "hash_bits": M, "top_k": K, "num_heads": H, "dnn_hidden": [200, 80], "optimizer": "adam",
           "steps_per_sample": args.steps, "stage_calls_per_sample": args.stage_iters, "repeats": args.repeats,
           "shapes": [measure(B, T, C, args, hp, dev) for B, T, C in SHAPES], "scoring": scoring(args, hp, dev),
           "din_yardstick": din_yardstick(args, hp, dev)}
    by_T = {(s["batch"], s["T"]): s for s in out["shapes"]}
    out["stage_T4096_over_T1024"] = {str(B): {k: round(by_T[B, 4096][f"hip_{k}_us_median"] / by_T[B, 1024][f"hip_{k}_us_median"], 3)
                                              for k in ("stage_fwd", "stage")} for B in (128, 1024)}
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
