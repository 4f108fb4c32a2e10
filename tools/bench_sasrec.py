"""Measure the SASRec training step on the GPU: the HIP engine against the reference's own op sequence on torch.

    python tools/bench_sasrec.py [--steps 8] [--windows 3] [--warmup 1] [--repeats 5] [--out profiles/sasrec_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sasrec.py --hip-only --repeats 1   # kernel times

Shapes: the reference's default (B 128, T 200, D 64, H 2, 2 blocks, I 1682, Adam lr 1e-3) without dropout and with
dropout 0.1 drawn on the device, and D 32 / H 1 without dropout.  ``--steps`` batches of synthetic left-padded sequences
are staged on the device once.  A window is ``--windows`` passes over those batches between two device synchronisations;
the sides alternate ``--repeats`` times in one process, so both see the same machine state.  Sides:
  hip     SASRecEngine's launches (hiprec_sasrec_grad + the dense optimizer sweep), python-looped, no host sync
  torch   the reference's op sequence (models/sasrec.py:92-224 restated here, nothing imported from the reference:
          nn.Embedding / nn.LayerNorm / nn.MultiheadAttention / nn.Conv1d + autograd + torch.optim.Adam) WITHOUT the
          host sync the reference pays per step (``loss.item()``) and with the ``pos != 0`` indices staged on the device
There is no earlier number for this model: the yardstick is the torch side of the same run.  Needs a GPU.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

I, B, T, NB, LR, L2 = 1682, 128, 200, 2, 1e-3, 0.0
SHAPES = {"default": dict(D=64, H=2, p=0.0), "default_dropout": dict(D=64, H=2, p=0.1), "d32_h1": dict(D=32, H=1, p=0.0)}


class TorchSASRec(torch.nn.Module):
    """models/sasrec.py:42-165 on whatever device it is moved to."""

    def __init__(self, D, H, p):
        super().__init__()
        nn = torch.nn
        self.item_emb = nn.Embedding(I + 1, D, padding_idx=0)
        self.pos_emb = nn.Embedding(T, D)
        self.emb_dropout = nn.Dropout(p)
        self.attention_layernorms, self.attention_layers = nn.ModuleList(), nn.ModuleList()
        self.forward_layernorms, self.conv1, self.conv2 = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        self.drop1, self.drop2 = nn.Dropout(p), nn.Dropout(p)
        self.last_layernorm = nn.LayerNorm(D, eps=1e-8)
        for _ in range(NB):
            self.attention_layernorms.append(nn.LayerNorm(D, eps=1e-8))
            self.attention_layers.append(nn.MultiheadAttention(D, H, p))
            self.forward_layernorms.append(nn.LayerNorm(D, eps=1e-8))
            self.conv1.append(nn.Conv1d(D, D, kernel_size=1))
            self.conv2.append(nn.Conv1d(D, D, kernel_size=1))

    def state_for_engine(self):
        out = {"item_emb.weight": self.item_emb.weight, "pos_emb.weight": self.pos_emb.weight,
               "last_layernorm.weight": self.last_layernorm.weight, "last_layernorm.bias": self.last_layernorm.bias}
        for b in range(NB):
            for name, mod in (("attention_layernorms", self.attention_layernorms[b]),
                              ("forward_layernorms", self.forward_layernorms[b])):
                out[f"{name}.{b}.weight"], out[f"{name}.{b}.bias"] = mod.weight, mod.bias
            mha = self.attention_layers[b]
            out[f"attention_layers.{b}.in_proj_weight"], out[f"attention_layers.{b}.in_proj_bias"] = (
                mha.in_proj_weight, mha.in_proj_bias)
            out[f"attention_layers.{b}.out_proj.weight"], out[f"attention_layers.{b}.out_proj.bias"] = (
                mha.out_proj.weight, mha.out_proj.bias)
            for name, conv in (("conv1", self.conv1[b]), ("conv2", self.conv2[b])):
                out[f"forward_layers.{b}.{name}.weight"], out[f"forward_layers.{b}.{name}.bias"] = conv.weight, conv.bias
        return {k: v.detach().clone() for k, v in out.items()}

    def forward(self, seq, pos, neg, positions, causal):
        x = self.item_emb(seq) * self.item_emb.embedding_dim ** 0.5
        x = x + self.pos_emb(positions)
        x = self.emb_dropout(x)
        live = (seq != 0).unsqueeze(-1)
        x = x * live
        for b in range(NB):
            x = torch.transpose(x, 0, 1)
            q = self.attention_layernorms[b](x)
            mha, _ = self.attention_layers[b](q, x, x, attn_mask=causal)
            x = torch.transpose(q + mha, 0, 1)
            x = self.forward_layernorms[b](x)
            y = self.drop2(self.conv2[b](torch.relu(self.drop1(self.conv1[b](x.transpose(-1, -2))))))
            x = (y.transpose(-1, -2) + x) * live
        feats = self.last_layernorm(x)
        return (feats * self.item_emb(pos)).sum(-1), (feats * self.item_emb(neg)).sum(-1)


def batches_on(dev, steps, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        seq, pos, neg = (np.zeros((B, T), dtype=np.int64) for _ in range(3))
        for b in range(B):
            n = int(min(T, max(2, rng.geometric(1.0 / 100))))      # ML-100K-like: a mean of ~100 events, capped at T
            items = rng.integers(1, I + 1, n + 1)
            seq[b, T - n:], pos[b, T - n:], neg[b, T - n:] = items[:-1], items[1:], rng.integers(1, I + 1, n)
        out.append(tuple(torch.from_numpy(a).to(dev) for a in (seq, pos, neg)))
    return out


def measure(name, D, H, p, args, hp, dev):
    torch.manual_seed(0)
    ref = TorchSASRec(D, H, p)
    w0 = ref.state_for_engine()
    ref.to(dev)
    opt = torch.optim.Adam(ref.parameters(), lr=LR)
    bce = torch.nn.BCEWithLogitsLoss()
    cfg = {"model": {"n_users": 943, "n_items": I, "emb_dim": D, "maxlen": T, "num_blocks": NB, "num_heads": H,
                     "dropout_rate": p, "batch_size": B, "l2_emb": L2, "optimizer": "adam", "lr": LR,
                     "device_str": "cuda:0", "dropout_rng": "device", "dropout_seed": 1},
           "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.SASRecEngine(cfg)
    eng.model.load_state_dict(w0)
    batches = batches_on(dev, args.steps)
    users = torch.zeros(B, dtype=torch.int64)
    positions = torch.arange(T, device=dev).unsqueeze(0).expand(B, T)
    causal = ~torch.tril(torch.ones((T, T), dtype=torch.bool, device=dev))
    valid = [torch.nonzero(b[1] != 0, as_tuple=True) for b in batches]

    def hip():
        for b in batches:
            eng._enqueue_step((users,) + b)

    def torch_steps():
        for b, idx in zip(batches, valid):
            opt.zero_grad()
            pl, nl = ref(*b, positions, causal)
            loss = bce(pl[idx], torch.ones_like(pl[idx])) + bce(nl[idx], torch.zeros_like(nl[idx]))
            loss = loss + L2 * torch.norm(ref.item_emb.weight)
            loss.backward()
            opt.step()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.windows):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (args.windows * len(batches)) * 1e6   # us per step

    sides = {"hip": hip}
    if not args.hip_only:
        sides["torch"] = torch_steps
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn))
    st = eng._sync_stats()
    M = B * T
    out = {"emb_dim": D, "heads": H, "dropout": p, "last_loss_hip": st.loss,
           # projections, FFN, attention: forward + dgrad + wgrad, 2 flops per multiply-add
           "gemm_gflop_per_step": round(NB * 3 * 2 * M * D * D * 6 / 1e9, 2),
           "attention_gflop_per_step": round(NB * (2 + 5) * 2 * B * T * T * D / 2 / 1e9, 2),
           "saved_activation_mb": round(NB * (9 * M * D + 2 * M * H + 4 * M) * 4 / 1e6, 1)}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 1) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
    if "torch" in times:
        out["hip_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
        out["hip_not_slower_than_torch"] = bool(out["hip_us_per_step_median"] <= 1.05 * out["torch_us_per_step_median"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_sasrec.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_sasrec.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "n_items": I, "batch": B, "maxlen": T, "blocks": NB,
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
