"""Measure DIEN on the GPU: the evolution stage of csrc/dien.hip (attention + AUGRU, forward and forward + backward), a
scoring call and the whole Adam step of the HIP engine, each against the same computation in torch ops with autograd on the
same card: ``tests/dien_torch.py``, a Python loop over the positions on a ``[B C, D]`` state.

    python tools/bench_dien.py [--steps 3] [--stage-iters 20] [--warmup 2] [--repeats 5] [--out profiles/dien_step.json]

43 097 items, D 64, dnn_hidden [200, 80], Dice tower, B 128 / 1024, T 50 / 200, C 4.
  stage     ``DIEN.evolve_stage`` without / with ``dhT`` (att.weight q and the projection through the grouped GEMM, the
            recurrence with its attention; the reverse recurrence, the folds and its GEMM group) vs ``dien_torch.evolve``
            without / with ``torch.autograd.grad``; both sides produce ``hT``, ``d h1``, ``d q`` and the gradients of
            ``att.weight`` and ``evolve.*``
  extract   ``DIEN.extract_stage`` without / with ``dh1`` (the projection GEMM, the recurrence at one candidate, its reverse and
            the weight-gradient group) vs ``dien_torch.recurrence`` and vs ``torch.nn.GRU`` on the same rows and weights.  The
            library GRU mixes ``u`` the other way round and has no mask for a left padding (it walks all positions of every
            row), so it is a time yardstick, not a numerical one
  scoring   ``DIENEngine.predict`` vs the restatement in eval mode under ``no_grad`` at B 128, T 50, C 100, forward only
  step      ``hiprec_dien_grad`` + the dense optimizer sweep vs the restatement's ops + both losses + ``torch.optim.Adam``
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

I, D, LR, AUX = 43097, 64, 1e-3, 1.0
SHAPES = [(B, T, 4) for T in (50, 200) for B in (128, 1024)]
STAGE = ("att.weight", "evolve.weight_ih", "evolve.weight_hh", "evolve.bias")
EXTRACT = ("extractor.weight_ih", "extractor.weight_hh", "extractor.bias")


def make_engine(hp, B, T):
    model = {"n_items": I, "emb_dim": D, "maxlen": T, "batch_size": B, "lr": LR, "optimizer": "adam", "device_str": "cuda:0",
             "aux_weight": AUX}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.DIENEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_bench_runs"}})
    with torch.no_grad():
        eng.model.item_emb.weight.data.mul_(5.0)      # rows of order 0.5, the fixtures' scale
    return eng


def extract_stage(m, w0, seq, mask, n, args, dt, dev, gen):
    """``DIEN.extract_stage`` against the torch loop and against ``torch.nn.GRU`` on the same rows and weights."""
    B, T = seq.shape
    x = m.item_emb.weight.data[seq].contiguous()
    dh1 = torch.randn(B, T, D, device=dev, generator=gen) * mask[:, :, None]
    gru = torch.nn.GRU(D, D, batch_first=True).to(dev)
    with torch.no_grad():      # the same gate order r | u | n; one bias vector here, so bias_hh is 0
        gru.weight_ih_l0.copy_(w0[EXTRACT[0]])
        gru.weight_hh_l0.copy_(w0[EXTRACT[1]])
        gru.bias_ih_l0.copy_(w0[EXTRACT[2]])
        gru.bias_hh_l0.zero_()

    def hip_fwd():
        for _ in range(n):
            out = m.extract_stage(x, mask)
        return out

    def hip_fwd_bwd():
        for _ in range(n):
            out = m.extract_stage(x, mask, dh1)
        return out

    def torch_fwd():
        with torch.no_grad():
            return dt.recurrence(x, mask, *(w0[k] for k in EXTRACT))

    def torch_fwd_bwd():
        xl = x.detach().requires_grad_()
        wl = [w0[k].detach().requires_grad_() for k in EXTRACT]
        h = dt.recurrence(xl, mask, *wl)
        return h, torch.autograd.grad(h, [xl] + wl, dh1)

    def gru_fwd():
        with torch.no_grad():
            for _ in range(n):
                h = gru(x)[0]
        return h

    def gru_fwd_bwd():
        for _ in range(n):
            xl = x.detach().requires_grad_()
            h = gru(xl)[0]
            out = torch.autograd.grad(h, [xl, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0], dh1)
        return h, out

    h1, dx, g = hip_fwd_bwd()
    h_t, grads_t = torch_fwd_bwd()
    diff = max([rel(h1, h_t), rel(dx, grads_t[0])] + [rel(g[k], gt) for k, gt in zip(EXTRACT, grads_t[1:])])
    if diff > 1e-4:
        raise SystemExit(f"B {B} T {T}: the HIP extractor stage and the torch ops differ by {diff}")
    out = {"max_rel_diff_vs_torch_ops": diff}
    sides = {"hip_fwd": hip_fwd, "torch_fwd": torch_fwd, "gru_fwd": gru_fwd, "hip": hip_fwd_bwd, "torch": torch_fwd_bwd,
             "gru": gru_fwd_bwd}
    out.update(alternate(sides, {k: 1 if k.startswith("torch") else n for k in sides}, args))
    for other in ("torch", "gru"):
        out[f"fwd_speedup_vs_{other}"] = round(out[f"{other}_fwd_us_median"] / out["hip_fwd_us_median"], 2)
        out[f"speedup_vs_{other}"] = round(out[f"{other}_us_median"] / out["hip_us_median"], 2)
    out["peak_mb_above_resident"] = {"hip": peak_mb(lambda: m.extract_stage(x, mask, dh1)), "torch": peak_mb(torch_fwd_bwd),
                                     "gru": peak_mb(gru_fwd_bwd)}
    return out


def measure(B, T, C, args, hp, dev):
    import dien_torch as dt

    torch.manual_seed(B + T)
    eng = make_engine(hp, B, T)
    m = eng.model
    cfg = {"dnn_hidden": m.dnn_hidden, "aux_weight": AUX}
    w0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(B * 1000 + T)
    batches = []
    for _ in range(args.steps):
        seq = rng.integers(1, I + 1, (B, T))
        seq[np.arange(T)[None, :] < rng.integers(0, T // 2, B)[:, None]] = 0      # left padding of mixed lengths
        neg = np.where(seq != 0, rng.integers(1, I + 1, (B, T)), 0)
        cand, label = rng.integers(1, I + 1, (B, C)), (rng.random((B, C)) < 0.25).astype(np.float32)
        batches.append(tuple(torch.from_numpy(a).to(dev) for a in (seq, neg, cand, label)))
    seq, _, cand, _ = batches[0]
    n = args.stage_iters
    gen = torch.Generator(device=dev).manual_seed(7)
    h1 = torch.randn(B, T, D, device=dev, generator=gen) * 0.5
    q, mask = m.item_emb.weight.data[cand].contiguous(), seq != 0
    dhT = torch.randn(B, C, D, device=dev, generator=gen)

    def hip_fwd():
        for _ in range(n):
            out = m.evolve_stage(h1, q, mask)
        return out

    def hip_fwd_bwd():
        for _ in range(n):
            out = m.evolve_stage(h1, q, mask, dhT)
        return out

    def torch_fwd():
        with torch.no_grad():
            return dt.evolve(h1, q, mask, w0)[0]

    def torch_fwd_bwd():
        hl, ql = h1.detach().requires_grad_(), q.detach().requires_grad_()
        wl = {k: w0[k].detach().requires_grad_() for k in STAGE}
        hT = dt.evolve(hl, ql, mask, wl)[0]
        return hT, torch.autograd.grad(hT, [hl, ql] + [wl[k] for k in STAGE], dhT)

    hT, _, dh1, dq, g = hip_fwd_bwd()
    hT_t, grads_t = torch_fwd_bwd()
    diff = max([rel(hT, hT_t), rel(dh1, grads_t[0]), rel(dq, grads_t[1])] + [rel(g[k], gt) for k, gt in zip(STAGE, grads_t[2:])])
    if diff > 1e-4:
        raise SystemExit(f"B {B} T {T}: the HIP stage and the torch ops differ by {diff}")
    out = {"batch": B, "T": T, "C": C, "tiles": m.tiles(C), "stage_max_rel_diff_vs_torch_ops": diff}
    sides = {"hip_stage_fwd": hip_fwd, "torch_stage_fwd": torch_fwd, "hip_stage": hip_fwd_bwd, "torch_stage": torch_fwd_bwd}
    out.update(alternate(sides, {k: n if k.startswith("hip") else 1 for k in sides}, args))
    out["stage_fwd_speedup"] = round(out["torch_stage_fwd_us_median"] / out["hip_stage_fwd_us_median"], 2)
    out["stage_speedup"] = round(out["torch_stage_us_median"] / out["hip_stage_us_median"], 2)
    out["stage_peak_mb_above_resident"] = {"hip": peak_mb(lambda: m.evolve_stage(h1, q, mask, dhT)), "torch": peak_mb(torch_fwd_bwd)}

    out["extract"] = extract_stage(m, w0, seq, mask, n, args, dt, dev, gen)

    # the whole step
    params ={k: torch.nn.Parameter(t.clone()) for k, t in w0.items() if "running" not in k}
    run = {k: t.clone() for k, t in w0.items() if "running" in k}
    opt = torch.optim.Adam(params.values(), lr=LR)

    def torch_loss(b):
        z, live, aux = dt.forward(params, cfg, b[0], b[1], b[2], run, True)
        return F.binary_cross_entropy_with_logits(z.reshape(-1)[live], b[3].reshape(-1)[live]) + AUX * aux

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
    import dien_torch as dt

    torch.manual_seed(1)
    eng = make_engine(hp, B, T)
    m = eng.model
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
            return dt.forward(w, {"dnn_hidden": m.dnn_hidden}, seq, None, cand, w, False)[0]

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
    ap.add_argument("--stage-iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_dien.py measures on the GPU; no GPU found and there is no CPU timing path")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_dien.py", "device": torch.cuda.get_device_name(0), "source_hash": __graft_entry__.source_hash(),
           "n_items": I, "emb_dim": D, "dnn_hidden": [200, 80], "aux_weight": AUX, "optimizer": "adam",
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
