"""Measure the NextItNet training step on the GPU: the HIP engine against the same step written as torch ops, and the
fused convolution stage alone against the im2col + grouped-GEMM form it replaces.

    python tools/bench_nextitnet.py [--steps 4] [--warmup 3] [--repeats 7] [--out profiles/nextitnet_step.json]

Shapes (43 097 items, B 128, T 50, kernel 3, dilations [1, 4] x 5 blocks, Adam lr 1e-3, no l2):
  d64_all    D 64, every position labelled          d64_last   D 64, the last position of every sequence labelled
  d128_all   D 128, every position labelled
``--steps`` batches of synthetic sequences are staged on the device once.  One sample is the HIP-event time of a pass
over those batches divided by their number; the sides alternate ``--repeats`` times in one process after ``--warmup``
passes each, and the medians are reported with their spread.  Sides:
  hip     NextItNetEngine's launches (hiprec_nextitnet_grad + the dense optimizer sweep), no host sync
  torch   the same model as torch ops with autograd (F.conv2d with dilation on left-padded input, F.layer_norm,
          F.cross_entropy over the labelled rows against the tied table, torch.optim.Adam), fp32, TF32 off
  conv    one stage (conv2 of block 0: dilation 2, with the residual) on the step's [B, T, D] activations:
          ``fused`` is hiprec_nextitnet_conv (shifted rows staged in LDS, LayerNorm + ReLU + residual in the epilogue),
          ``im2col`` gathers the k shifted copies into [B T, k D] with torch, multiplies through hiprec_gemm_f32 (the
          grouped exact-fp32 GEMM, bias in its epilogue) and applies F.layer_norm, relu and the residual with torch ops
Before anything is timed both sides compute the first batch's loss from the same weights; the tool stops if they differ
by more than 1e-4 relative, and the two convolution forms must agree to 1e-5 of the output's scale.  Needs a GPU.
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

I, B, T, K, DILATIONS, BLOCK_NUM, LR = 43097, 128, 50, 3, [1, 4], 5, 1e-3
SHAPES = {"d64_all": dict(D=64, loss="all"), "d64_last": dict(D=64, loss="last"), "d128_all": dict(D=128, loss="all")}


def causal_conv(x, weight, bias, dil):
    k = weight.shape[-1]
    xp = F.pad(x.transpose(1, 2).unsqueeze(2), ((k - 1) * dil, 0))
    return F.conv2d(xp, weight, bias, dilation=(1, dil)).squeeze(2).transpose(1, 2)


class TorchNextItNet(torch.nn.Module):
    """The model of include/hiprec.h's NextItNet block as torch ops; parameters keyed like the engine's state_dict."""

    def __init__(self, w, D, loss):
        super().__init__()
        self.names = list(w)
        self.params = torch.nn.ParameterList(torch.nn.Parameter(v.clone()) for v in w.values())
        self.D, self.loss = D, loss

    def forward(self, seq, pos):
        w, D = dict(zip(self.names, self.params)), self.D
        x = F.embedding(seq, w["item_emb.weight"], padding_idx=0)
        for r, d in enumerate(DILATIONS * BLOCK_NUM):
            p = f"blocks.{r}."
            h = F.relu(F.layer_norm(causal_conv(x, w[p + "conv1.weight"], w[p + "conv1.bias"], d), (D,),
                                    w[p + "ln1.weight"], w[p + "ln1.bias"], 1e-8))
            x = F.relu(F.layer_norm(causal_conv(h, w[p + "conv2.weight"], w[p + "conv2.bias"], 2 * d), (D,),
                                    w[p + "ln2.weight"], w[p + "ln2.bias"], 1e-8)) + x
        f = F.linear(x, w["final_layer.weight"], w["final_layer.bias"])
        if self.loss == "last":
            f, pos = f[:, -1], pos[:, -1]
        f, pos = f.reshape(-1, D), pos.reshape(-1)
        keep = pos != 0
        return F.cross_entropy(f[keep] @ w["item_emb.weight"][1:].T, pos[keep] - 1)


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


def measure(name, D, loss, args, hp, dev):
    from beta_recsys_amd import _lib

    torch.manual_seed(0)
    cfg = {"model": {"n_items": I, "emb_dim": D, "kernel_size": K, "dilations": DILATIONS, "block_num": BLOCK_NUM,
                     "maxlen": T, "loss_positions": loss, "lr": LR, "optimizer": "adam", "device_str": "cuda:0"},
           "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    rng = np.random.default_rng(1)
    batches = []
    for _ in range(args.steps):
        walk = rng.integers(1, I + 1, (B, T + 1))
        walk[np.arange(T + 1)[None, :] < rng.integers(0, T // 2, B)[:, None]] = 0      # left padding of mixed lengths
        seq, pos = walk[:, :-1], np.where(walk[:, :-1] != 0, walk[:, 1:], 0)
        batches.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (seq, pos)))
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.NextItNetEngine(cfg)
    w0 = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
    step_batches = [(None, s, p, None) for s, p in batches]
    first = {"hip": float(eng.backward_only(step_batches[0])[0])}
    ref = TorchNextItNet(w0, D, loss).to(dev)
    opt = torch.optim.Adam(ref.parameters(), lr=LR)
    with torch.no_grad():
        first["torch"] = float(ref(*batches[0]))
    if abs(first["torch"] - first["hip"]) > 1e-4 * abs(first["torch"]):
        raise SystemExit(f"{name}: the two sides do not compute the same loss from the same weights: {first}")

    def hip():
        for b in step_batches:
            eng._enqueue_step(b)

    def torch_steps():
        for b in batches:
            opt.zero_grad()
            ref(*b).backward()
            opt.step()

    out = {"emb_dim": D, "loss_positions": loss, "first_batch_loss": first}
    step = alternate({"hip": hip, "torch": torch_steps}, len(batches), args)
    out.update({k.replace("_us", "_us_per_step"): v for k, v in step.items()})
    out["hip_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
    out["workspace_mb"] = round(eng.model._ws.numel() / 1e6, 1)

    # one convolution stage alone: conv2 of block 0 (dilation 2 DILATIONS[0]) with the residual
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    dil = 2 * DILATIONS[0]
    wt, bias = w0["blocks.0.conv2.weight"], w0["blocks.0.conv2.bias"]
    g, be = w0["blocks.0.ln2.weight"], w0["blocks.0.ln2.bias"]
    x = torch.randn(B, T, D, device=dev)
    fused_out = torch.empty_like(x)
    w_cols = wt[:, :, 0, :].permute(0, 2, 1).reshape(D, K * D).contiguous()      # [D_out, (j, D_in)]
    cols, pre = torch.empty(B * T, K * D, device=dev), torch.empty(B * T, D, device=dev)

    def fused():
        _lib.check(lib.hiprec_nextitnet_conv(_lib.ptr(x), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(g), _lib.ptr(be),
                                             _lib.ptr(x), B, T, D, K, dil, _lib.ptr(fused_out), st))

    def im2col():
        xp = F.pad(x, (0, 0, (K - 1) * dil, 0))
        torch.cat([xp[:, j * dil:j * dil + T] for j in range(K)], 2, out=cols.view(B, T, K * D))
        _lib.check(lib.hiprec_gemm_f32(0, B * T, D, K * D, _lib.ptr(cols), K * D, _lib.ptr(w_cols), K * D, _lib.ptr(pre), D,
                                       _lib.ptr(bias), 0, None, 0, st))
        return F.relu(F.layer_norm(pre, (D,), g, be, 1e-8)).view(B, T, D) + x

    fused()
    err = float((fused_out - im2col()).abs().max() / fused_out.abs().max())
    if err > 1e-5:
        raise SystemExit(f"{name}: the fused convolution and the im2col form differ by {err:.3e} of the output's scale")
    conv = alternate({"fused": lambda: [fused() for _ in range(args.steps)],
                      "im2col": lambda: [im2col() for _ in range(args.steps)]}, args.steps, args)
    conv["fused_vs_im2col_max_rel_diff"] = err
    conv["fused_speedup_vs_im2col"] = round(conv["im2col_us_median"] / conv["fused_us_median"], 2)
    out["conv_stage"] = conv
    del eng
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_nextitnet.py measures on the GPU; no GPU found and there is no CPU timing path")
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_nextitnet.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "n_items": I, "batch": B, "seq_len": T, "kernel_size": K,
           "dilations": DILATIONS, "block_num": BLOCK_NUM, "optimizer": "adam", "steps_per_sample": args.steps,
           "repeats": args.repeats, "shapes": {}}
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
