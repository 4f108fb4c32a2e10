"""Measure the BERT4Rec training step on the GPU: the HIP engine against the same step written as torch ops.

    python tools/bench_bert4rec.py [--steps 4] [--windows 2] [--warmup 1] [--repeats 3] [--out profiles/bert4rec_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_bert4rec.py --hip-only --repeats 1   # kernel times

Shapes (B 128, T 200, D 64, H 2, 2 blocks, ffn 256, Adam lr 1e-3, 20 % of the real positions masked): a catalogue of
1 682 items without dropout and with dropout 0.1 drawn on the device, and a catalogue of 100 000 items.  ``--steps``
batches of synthetic left-padded sequences are staged on the device once, the labelled positions as the compact list
the engine takes.  A window is ``--windows`` passes over those batches between two device synchronisations; the sides
alternate ``--repeats`` times in one process, so both see the same machine state.  Sides:
  hip     BERT4RecEngine's launches (hiprec_bert4rec_grad + the dense optimizer sweep), python-looped, no host sync;
          the labels arrive as a host array, as from data.ClozeSampler, and their compact list is uploaded every step
  torch   the same model as torch ops with autograd (F.layer_norm, F.gelu, explicit masked attention, F.cross_entropy
          over ``h E[1:I+1]^T + out_bias``, torch.optim.Adam), no host sync either, labelled positions staged
Peak memory is each side's own: ``torch.cuda.max_memory_allocated`` over the side's construction and its first steps,
less what was allocated before (the engine's workspace comes from the same allocator).  If the torch side cannot allocate,
that is recorded as its result.  Before anything is timed both sides compute the first batch's loss from the same initial
weights in eval mode; the two values are recorded and the tool stops if they differ by more than 1e-4 relative.  There is
no earlier number for this model.  Needs a GPU.
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, T, D, H, NB, FFN, LR, MASK_PROB = 128, 200, 64, 2, 2, 256, 1e-3, 0.2
SHAPES = {"items_1682": dict(I=1682, p=0.0), "items_1682_dropout": dict(I=1682, p=0.1), "items_100k": dict(I=100000, p=0.0)}


class TorchBERT4Rec(torch.nn.Module):
    """The model of include/hiprec.h's BERT4Rec block as torch ops; parameters keyed like the engine's state_dict."""

    def __init__(self, w, p):
        super().__init__()
        self.names = list(w)
        self.params = torch.nn.ParameterList(torch.nn.Parameter(v.clone()) for v in w.values())
        self.p = p

    def forward(self, seq, lab_pos, lab_item):
        w = dict(zip(self.names, self.params))
        Bq, Tq = seq.shape
        hd = D // H
        ln = lambda x, n: F.layer_norm(x, (D,), w[n + ".weight"], w[n + ".bias"], 1e-8)   # noqa: E731
        drop = lambda x: F.dropout(x, self.p, self.training)                               # noqa: E731
        x = drop(ln(w["item_emb.weight"][seq] + w["pos_emb.weight"][:Tq][None], "emb_layernorm"))
        closed = (seq == 0)[:, None, None, :]
        any_open = (~closed).any(-1, keepdim=True)
        for k in range(NB):
            a, f = f"attention_layers.{k}.", f"forward_layers.{k}."
            qkv = x @ w[a + "in_proj_weight"].T + w[a + "in_proj_bias"]
            q, kk, v = (t.reshape(Bq, Tq, H, hd).transpose(1, 2) for t in qkv.split(D, dim=-1))
            s = (q @ kk.transpose(-1, -2)) / hd ** 0.5
            s = s.masked_fill(closed & any_open, float("-inf"))       # an all-padding sequence keeps finite rows ...
            pr = torch.softmax(s, -1) * any_open                      # ... which are then zeroed
            o = (drop(pr) @ v).transpose(1, 2).reshape(Bq, Tq, D)
            x = ln(x + drop(o @ w[a + "out_proj.weight"].T + w[a + "out_proj.bias"]), f"attention_layernorms.{k}")
            z = F.gelu(x @ w[f + "fc1.weight"].T + w[f + "fc1.bias"]) @ w[f + "fc2.weight"].T + w[f + "fc2.bias"]
            x = ln(x + drop(z), f"forward_layernorms.{k}")
        h = ln(F.gelu(x.reshape(-1, D)[lab_pos] @ w["head.dense.weight"].T + w["head.dense.bias"]), "head.layernorm")
        n_items = w["out_bias"].shape[0] - 1
        logits = h @ w["item_emb.weight"][1:n_items + 1].T + w["out_bias"][1:]
        return F.cross_entropy(logits, lab_item - 1)


def batches_on(dev, steps, n_items, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        seq = np.zeros((B, T), dtype=np.int64)
        for b in range(B):
            n = int(min(T, max(2, rng.geometric(1.0 / 100))))      # ML-100K-like: a mean of ~100 events, capped at T
            seq[b, T - n:] = rng.integers(1, n_items + 1, n)
        masked = (seq != 0) & (rng.random(seq.shape) < MASK_PROB)
        masked[~masked.any(1), -1] = True
        labels = np.where(masked, seq, 0)
        seq = np.where(masked, n_items + 1, seq)
        at = np.flatnonzero(labels.reshape(-1))
        # labels stay on the host: the engine builds its compact list there, as it does for the sampler's batches
        out.append((torch.from_numpy(seq).to(dev), labels, torch.from_numpy(at).to(dev),
                    torch.from_numpy(labels.reshape(-1)[at]).to(dev)))
    return out


def measure(name, I, p, args, hp, dev):
    torch.manual_seed(0)
    cfg = {"model": {"n_users": 943, "n_items": I, "emb_dim": D, "maxlen": T, "num_blocks": NB, "num_heads": H,
                     "dropout_rate": p, "batch_size": B, "ffn_dim": FFN, "optimizer": "adam", "lr": LR,
                     "device_str": "cuda:0", "dropout_rng": "device", "dropout_seed": 1},
           "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    batches = batches_on(dev, args.steps, I)
    users = torch.zeros(B, dtype=torch.int64)
    n_lab = [int(b[2].numel()) for b in batches]
    torch.cuda.synchronize()
    peaks = {}

    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.BERT4RecEngine(cfg)
    w0 = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
    # the same step on both sides: the first batch's loss from the same weights, in eval mode (no dropout draws)
    eng.model.eval()
    first_loss = {"hip": float(eng.backward_only((users, batches[0][0], batches[0][1]))[0])}
    eng.model.train()
    eng.load_optimizer_state(0)

    def hip():
        for b in batches:
            eng._enqueue_step((users, b[0], b[1]))

    hip()
    torch.cuda.synchronize()
    peaks["hip"] = torch.cuda.max_memory_allocated() - base
    sides = {"hip": hip}
    torch_failure = None
    if not args.hip_only:
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        try:
            ref = TorchBERT4Rec({k: v.to(dev) for k, v in w0.items()}, p).to(dev)
            opt = torch.optim.Adam(ref.parameters(), lr=LR)
            ref.eval()
            with torch.no_grad():
                first_loss["torch"] = float(ref(batches[0][0], batches[0][2], batches[0][3]))
            ref.train()
            if abs(first_loss["torch"] - first_loss["hip"]) > 1e-4 * abs(first_loss["torch"]):
                raise SystemExit(f"{name}: the two sides do not compute the same loss from the same weights: {first_loss}")

            def torch_steps():
                for b in batches:
                    opt.zero_grad()
                    ref(b[0], b[2], b[3]).backward()
                    opt.step()

            torch_steps()
            torch.cuda.synchronize()
            peaks["torch"] = torch.cuda.max_memory_allocated() - base
            sides["torch"] = torch_steps
        except torch.cuda.OutOfMemoryError as e:
            torch_failure = "out of memory: " + str(e).split("\n")[0]

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.windows):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (args.windows * len(batches)) * 1e6   # us per step

    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn))
    st = eng._sync_stats()
    n_mean = float(np.mean(n_lab))
    out = {"n_items": I, "dropout": p, "labelled_rows_per_step": round(n_mean, 1), "last_loss_hip": st.loss,
           "first_batch_eval_loss": first_loss,      # both sides from the same initial weights; they must agree to 1e-4
           "score_matrix_mb_if_formed": round(n_mean * I * 4 / 1e6, 1),
           # scores: forward once, recomputed in each of the two backward kernels, plus their two products
           "cross_entropy_gflop_per_step": round(5 * 2 * n_mean * I * D / 1e9, 2),
           "workspace_mb": round(eng.model._ws.numel() / 1e6, 1)}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 1) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
        out[f"{k}_peak_memory_mb"] = round(peaks[k] / 1e6, 1)
    if torch_failure:
        out["torch_result"] = torch_failure
    if "torch" in times:
        out["hip_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
    del eng
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--windows", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_bert4rec.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_bert4rec.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "batch": B, "maxlen": T, "emb_dim": D, "heads": H, "blocks": NB,
           "ffn_dim": FFN, "optimizer": "adam", "steps_per_window": args.windows * args.steps, "repeats": args.repeats,
           "shapes": {}}
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
