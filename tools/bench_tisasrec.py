"""Measure the TiSASRec training step on the GPU: the HIP engine against the reference's own op sequence on torch.

    python tools/bench_tisasrec.py [--steps 4] [--windows 6] [--warmup 1] [--repeats 5] [--out profiles/tisasrec_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_tisasrec.py --hip-only --repeats 1   # kernel times

Shapes: the reference's default (configs/tisasrec_default.json: B 128, T 150, D 64, H 2, 2 blocks, time_span 128, dropout
0.1, here drawn on the device; I 3416, Adam lr 1e-3), the same without dropout, and a short one (B 64, T 50, D 32, H 1,
time_span 64).  ``--steps`` batches of synthetic left-padded timestamped sequences are staged on the device once, their
relation matrices included (both sides get them ready-made, as the reference's sampler hands them over).  A window is
``--windows`` passes over those batches between two device synchronisations; after each side was built and warmed up
(``--warmup`` untimed passes, which is also where its peak memory is read), the sides alternate ``--repeats`` times in
one process, so both see the same machine state.  Sides:
  hip     TiSASRecEngine's launches (hiprec_tisasrec_grad + the dense optimizer sweep), python-looped, no host sync
  torch   the reference's op sequence (models/tisasrec.py:101-165, 238-335, 375-392 restated here, nothing imported from
          the reference: the two gathered [B, T, T, D] tensors, their dropouts, the batched mat-vecs, autograd,
          torch.optim.Adam) WITHOUT the host sync the reference pays per step (``loss.item()``) and with the ``pos != 0``
          indices staged on the device
Peak memory of a side is ``torch.cuda.max_memory_allocated`` over its construction and warm-up beyond what was
allocated before it existed (the staged batches, and for the torch side the HIP engine built before it): parameters,
optimizer state, workspace or autograd's saved tensors, and the dropout masks.  If the torch
side cannot allocate at a shape, that is recorded as the result for that shape.  There is no earlier number for this
model and no speed-up was promised: the yardstick is the torch side of the same run.  Needs a GPU.
"""
import argparse
import contextlib
import gc
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

I, NB, LR, L2 = 3416, 2, 1e-3, 0.0
SHAPES = {"default": dict(B=128, T=150, D=64, H=2, span=128, p=0.1),
          "default_no_dropout": dict(B=128, T=150, D=64, H=2, span=128, p=0.0),
          "short_d32_h1": dict(B=64, T=50, D=32, H=1, span=64, p=0.0)}


class TorchTiSASRec(torch.nn.Module):
    """models/tisasrec.py:168-335 on whatever device it is moved to."""

    def __init__(self, T, D, H, span, p):
        super().__init__()
        nn = torch.nn
        self.H, self.hd = H, D // H
        self.item_emb = nn.Embedding(I + 1, D, padding_idx=0)
        self.abs_pos_K_emb, self.abs_pos_V_emb = nn.Embedding(T, D), nn.Embedding(T, D)
        self.time_matrix_K_emb, self.time_matrix_V_emb = nn.Embedding(span + 1, D), nn.Embedding(span + 1, D)
        self.drops = nn.ModuleList(nn.Dropout(p) for _ in range(5))
        self.attention_layernorms, self.forward_layernorms = nn.ModuleList(), nn.ModuleList()
        self.Q_w, self.K_w, self.V_w = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        self.conv1, self.conv2 = nn.ModuleList(), nn.ModuleList()
        self.attn_drop, self.drop1, self.drop2 = nn.Dropout(p), nn.Dropout(p), nn.Dropout(p)
        self.last_layernorm = nn.LayerNorm(D, eps=1e-8)
        for _ in range(NB):
            self.attention_layernorms.append(nn.LayerNorm(D, eps=1e-8))
            self.Q_w.append(nn.Linear(D, D)), self.K_w.append(nn.Linear(D, D)), self.V_w.append(nn.Linear(D, D))
            self.forward_layernorms.append(nn.LayerNorm(D, eps=1e-8))
            self.conv1.append(nn.Conv1d(D, D, kernel_size=1))
            self.conv2.append(nn.Conv1d(D, D, kernel_size=1))

    def state_for_engine(self):
        out = {"last_layernorm.weight": self.last_layernorm.weight, "last_layernorm.bias": self.last_layernorm.bias}
        for name in ("item_emb", "abs_pos_K_emb", "abs_pos_V_emb", "time_matrix_K_emb", "time_matrix_V_emb"):
            out[name + ".weight"] = getattr(self, name).weight
        for b in range(NB):
            for name, mod in (("attention_layernorms", self.attention_layernorms[b]),
                              ("forward_layernorms", self.forward_layernorms[b])):
                out[f"{name}.{b}.weight"], out[f"{name}.{b}.bias"] = mod.weight, mod.bias
            for name, mod in (("Q_w", self.Q_w[b]), ("K_w", self.K_w[b]), ("V_w", self.V_w[b])):
                out[f"attention_layers.{b}.{name}.weight"], out[f"attention_layers.{b}.{name}.bias"] = mod.weight, mod.bias
            for name, conv in (("conv1", self.conv1[b]), ("conv2", self.conv2[b])):
                out[f"forward_layers.{b}.{name}.weight"], out[f"forward_layers.{b}.{name}.bias"] = conv.weight, conv.bias
        return {k: v.detach().clone() for k, v in out.items()}

    def attention(self, b, queries, keys, time_mask, attn_mask, tk, tv, pk, pv):
        """TimeAwareMultiHeadAttention.forward (tisasrec.py:101-165), op for op."""
        hs = self.hd
        Q, K, V = self.Q_w[b](queries), self.K_w[b](keys), self.V_w[b](keys)
        heads = lambda a, dim: torch.cat(torch.split(a, hs, dim=dim), dim=0)   # noqa: E731
        Q_, K_, V_ = heads(Q, 2), heads(K, 2), heads(V, 2)
        tk_, tv_, pk_, pv_ = heads(tk, 3), heads(tv, 3), heads(pk, 2), heads(pv, 2)
        w = Q_.matmul(torch.transpose(K_, 1, 2))
        w = w + Q_.matmul(torch.transpose(pk_, 1, 2))
        w = w + tk_.matmul(Q_.unsqueeze(-1)).squeeze(-1)
        w = w / (K_.shape[-1] ** 0.5)
        time_mask = time_mask.unsqueeze(-1).repeat(self.H, 1, 1).expand(-1, -1, w.shape[-1])
        attn_mask = attn_mask.unsqueeze(0).expand(w.shape[0], -1, -1)
        paddings = torch.ones(w.shape, device=w.device) * (-(2 ** 32) + 1)
        w = torch.where(time_mask, paddings, w)
        w = torch.where(attn_mask, paddings, w)
        w = self.attn_drop(torch.softmax(w, dim=-1))
        out = w.matmul(V_)
        out = out + w.matmul(pv_)
        out = out + w.unsqueeze(2).matmul(tv_).reshape(out.shape).squeeze(2)
        return torch.cat(torch.split(out, Q.shape[0], dim=0), dim=2)

    def forward(self, seq, tm, pos, neg, positions, causal):
        x = self.drops[0](self.item_emb(seq) * self.item_emb.embedding_dim ** 0.5)
        pk, pv = self.drops[1](self.abs_pos_K_emb(positions)), self.drops[2](self.abs_pos_V_emb(positions))
        tk, tv = self.drops[3](self.time_matrix_K_emb(tm)), self.drops[4](self.time_matrix_V_emb(tm))
        pad = seq == 0
        x = x * ~pad.unsqueeze(-1)
        for b in range(NB):
            q = self.attention_layernorms[b](x)
            x = q + self.attention(b, q, x, pad, causal, tk, tv, pk, pv)
            x = self.forward_layernorms[b](x)
            y = self.drop2(self.conv2[b](torch.relu(self.drop1(self.conv1[b](x.transpose(-1, -2))))))
            x = (y.transpose(-1, -2) + x) * ~pad.unsqueeze(-1)
        feats = self.last_layernorm(x)
        return (feats * self.item_emb(pos)).sum(-1), (feats * self.item_emb(neg)).sum(-1)


def batches_on(dev, steps, B, T, span, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        seq, pos, neg, ts = (np.zeros((B, T), dtype=np.int64) for _ in range(4))
        for b in range(B):
            n = int(min(T, max(2, rng.geometric(1.0 / 100))))      # ML-1M-like: long histories, most of them capped at T
            items = rng.integers(1, I + 1, n + 1)
            seq[b, T - n:], pos[b, T - n:], neg[b, T - n:] = items[:-1], items[1:], rng.integers(1, I + 1, n)
            ts[b, T - n:] = 1 + np.cumsum(rng.geometric(1.0 / 8, n))
        tm = np.minimum(np.abs(ts[:, :, None] - ts[:, None, :]), span)
        out.append((torch.from_numpy(seq).to(dev), torch.from_numpy(tm).to(dev), torch.from_numpy(pos).to(dev),
                    torch.from_numpy(neg).to(dev)))
    return out


def measure(name, B, T, D, H, span, p, args, hp, dev):
    gc.collect()                         # the previous shape's closures hold its batches until they are collected
    torch.cuda.empty_cache()
    torch.manual_seed(0)
    ref = TorchTiSASRec(T, D, H, span, p)
    w0 = ref.state_for_engine()
    cfg = {"model": {"n_users": 6040, "n_items": I, "emb_dim": D, "maxlen": T, "time_span": span, "num_blocks": NB,
                     "num_heads": H, "dropout_rate": p, "batch_size": B, "l2_emb": L2, "optimizer": "adam", "lr": LR,
                     "device_str": "cuda:0", "dropout_rng": "device", "dropout_seed": 1},
           "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    batches = batches_on(dev, args.steps, B, T, span)
    hip_batches = [(None, b[0], None, b[1].to(torch.int32), b[2], b[3]) for b in batches]
    positions = torch.arange(T, device=dev).unsqueeze(0).expand(B, T)
    causal = ~torch.tril(torch.ones((T, T), dtype=torch.bool, device=dev))
    valid = [torch.nonzero(b[2] != 0, as_tuple=True) for b in batches]
    bce = torch.nn.BCEWithLogitsLoss()
    torch.cuda.synchronize()
    baseline = torch.cuda.memory_allocated()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.windows):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (args.windows * len(batches)) * 1e6   # us per step

    def build(make):
        """Build a side and warm it up; its peak memory is what it took beyond what was allocated before it existed."""
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn = make()
        for _ in range(max(args.warmup, 1)):
            fn()
        torch.cuda.synchronize()
        return fn, torch.cuda.max_memory_allocated() - before

    def make_hip():
        with contextlib.redirect_stdout(io.StringIO()):
            eng = hp.TiSASRecEngine(cfg)
        eng.model.load_state_dict(w0)
        engines.append(eng)

        def fn():
            for b in hip_batches:
                eng._enqueue_step(b)
        return fn

    def make_torch():
        ref.to(dev)
        opt = torch.optim.Adam(ref.parameters(), lr=LR)

        def fn():
            for b, idx in zip(batches, valid):
                opt.zero_grad()
                pl, nl = ref(*b, positions, causal)
                loss = bce(pl[idx], torch.ones_like(pl[idx])) + bce(nl[idx], torch.zeros_like(nl[idx]))
                loss = loss + L2 * torch.norm(ref.item_emb.weight)
                loss.backward()
                opt.step()
        return fn

    M = B * T
    engines = []
    out = {"batch": B, "maxlen": T, "emb_dim": D, "heads": H, "time_span": span, "dropout": p,
           "allocated_before_mb": round(baseline / 1e6, 1), "one_gathered_tensor_mb": round(B * T * T * D * 4 / 1e6, 1),
           "hip_time_mask_mb": round(2 * B * T * T * D / 1e6, 1) if p > 0 else 0.0,
           # Q / K / V projections and the FFN: forward + dgrad + wgrad, 2 flops per multiply-add
           "gemm_gflop_per_step": round(NB * 5 * 2 * M * D * D * 3 / 1e9, 2),
           # causal half of: scores and outputs with their gathered terms forward (4), their gradients backward (10)
           "attention_gflop_per_step": round(NB * 14 * 2 * B * T * T * D / 2 / 1e9, 2)}
    sides = {}
    sides["hip"], peak = build(make_hip)
    out["hip_peak_mb"] = round(peak / 1e6, 1)
    if not args.hip_only:
        try:
            sides["torch"], peak = build(make_torch)
            out["torch_peak_mb"] = round(peak / 1e6, 1)
        except torch.cuda.OutOfMemoryError as e:
            out["torch"] = "could not allocate at this shape: " + str(e).splitlines()[0]
            ref.to("cpu")
            torch.cuda.empty_cache()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn))
    out["last_loss_hip"] = engines[0]._sync_stats().loss
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 1) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
    if "torch" in times:
        out["hip_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
        out["torch_peak_over_hip_peak"] = round(out["torch_peak_mb"] / max(out["hip_peak_mb"], 1e-9), 2)
    sides.clear()
    del engines[:]
    ref.to("cpu")
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_tisasrec.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_tisasrec.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "n_items": I, "blocks": NB, "optimizer": "adam",
           "steps_per_window": args.windows * args.steps, "repeats": args.repeats, "shapes": {}}
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
