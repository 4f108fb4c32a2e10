"""Measure the NARM training step on the GPU: the HIP engine against the reference's own op sequence on torch.

    python tools/bench_narm.py [--steps 4] [--windows 3] [--warmup 1] [--repeats 5] [--out profiles/narm_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_narm.py --hip-only --repeats 1   # kernel times

Shapes: ``default`` is configs/narm_default.json on ml_100k sizes (I 1682, B 1024, D 32, H 100, T 200, one layer);
``session_log`` a session-log shape (I 40 000, B 512, T 20); ``limits`` the kernels' limits (H 128, D 128, I 50 000,
B 1024, T 64).  All train with Adam and the default dropout rates (0.25 / 0.5), drawn on the device on the HIP side.
``--steps`` batches of synthetic sessions (lengths uniform in 1 .. T, sorted descending as ``collate_fn`` leaves them) are
staged on the device once.  A window is ``--windows`` passes over those batches between two device synchronisations; the
sides alternate ``--repeats`` times in one process, so both see the same machine state.  Sides:
  hip     NARMEngine's launches (hiprec_narm_grad + the dense optimizer sweep), python-looped, no host sync
  torch   the reference's op sequence (models/narm.py:50-142 restated here, nothing imported from the reference:
          nn.Embedding / nn.Dropout / pack_padded_sequence / nn.GRU / nn.Linear + autograd + CrossEntropyLoss +
          torch.optim.Adam) WITHOUT the host sync the reference pays per step (``loss.item()``)
Recorded per side: the median time per step and the peak device memory above what was allocated before the side's first
step.  There is no earlier number for this model: the yardstick is the torch side of the same run.  Needs a GPU.
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
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LR, P_IN, P_HID = 1e-2, 0.25, 0.5
SHAPES = {"default": dict(I=1682, B=1024, D=32, H=100, T=200, L=1),
          "session_log": dict(I=40000, B=512, D=32, H=100, T=20, L=1),
          "limits": dict(I=50000, B=1024, D=128, H=128, T=64, L=1)}


class TorchNARM(torch.nn.Module):
    """models/narm.py:17-94 on whatever device it is moved to."""

    def __init__(self, I, D, H, L):
        super().__init__()
        nn = torch.nn
        self.n_items, self.hidden_size, self.n_layers = I, H, L
        self.emb = nn.Embedding(I, D, padding_idx=0)
        self.emb_dropout = nn.Dropout(P_IN)
        self.gru = nn.GRU(D, H, L)
        self.a_1 = nn.Linear(H, H, bias=False)
        self.a_2 = nn.Linear(H, H, bias=False)
        self.v_t = nn.Linear(H, 1, bias=False)
        self.ct_dropout = nn.Dropout(P_HID)
        self.b = nn.Linear(D, 2 * H, bias=False)

    def forward(self, seq, lengths, arange):
        H = self.hidden_size
        hidden = torch.zeros((self.n_layers, seq.size(1), H), device=seq.device)
        embs = pack_padded_sequence(self.emb_dropout(self.emb(seq)), lengths)
        gru_out, hidden = self.gru(embs, hidden)
        gru_out, _ = pad_packed_sequence(gru_out)
        ht = hidden[-1]
        gru_out = gru_out.permute(1, 0, 2)
        q1 = self.a_1(gru_out.contiguous().view(-1, H)).view(gru_out.size())
        q2 = self.a_2(ht)
        mask = (seq.permute(1, 0) > 0).float()
        q2_masked = mask.unsqueeze(2).expand_as(q1) * q2.unsqueeze(1).expand_as(q1)
        alpha = self.v_t(torch.sigmoid(q1 + q2_masked).view(-1, H)).view(mask.size())
        c_local = torch.sum(alpha.unsqueeze(2).expand_as(gru_out) * gru_out, 1)
        c_t = self.ct_dropout(torch.cat([c_local, ht], 1))
        return torch.matmul(c_t, self.b(self.emb(arange)).permute(1, 0))


def batches_on(dev, steps, I, B, T, seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        lens = np.sort(rng.integers(1, T + 1, B))[::-1].copy()
        lens[0] = T
        seq = np.zeros((T, B), dtype=np.int64)
        real = np.arange(T)[:, None] < lens[None, :]
        seq[real] = rng.integers(1, I, int(real.sum()))
        target = rng.integers(1, I, B)
        out.append((torch.from_numpy(seq).to(dev), torch.from_numpy(target).to(dev), lens.tolist()))
    return out


def measure(name, I, B, D, H, T, L, args, hp, dev):
    torch.manual_seed(0)
    ref = TorchNARM(I, D, H, L)
    w0 = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    cfg = {"dataset": {"n_items": I},
           "model": {"hidden_size": H, "n_layers": L, "embedding_dim": D, "dropout_input": P_IN, "dropout_hidden": P_HID,
                     "batch_size": B, "optimizer": "adam", "lr": LR, "lr_dc_step": 80, "lr_dc": 0.1,
                     "device_str": "cuda:0", "dropout_rng": "device", "dropout_seed": 1},
           "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.NARMEngine(cfg)
    eng.model.load_state_dict(w0)
    eng.model.train()
    batches = batches_on(dev, args.steps, I, B, T)
    arange = torch.arange(I, device=dev)
    state = {}

    def hip():
        for b in batches:
            eng._enqueue_step(b)

    def torch_steps():
        if "opt" not in state:                  # built on first use, so that a side's peak memory is its own
            ref.to(dev)
            state["opt"] = torch.optim.Adam(ref.parameters(), lr=LR)
            state["ce"] = torch.nn.CrossEntropyLoss()
        for seq, target, lens in batches:
            state["opt"].zero_grad()
            loss = state["ce"](ref(seq, lens, arange), target)
            loss.backward()
            state["opt"].step()

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
    peak = {}
    for k, fn in sides.items():
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - before) / 1e6
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn))
    st = eng._sync_stats()
    M = B * T
    out = {"n_items": I, "batch": B, "emb_dim": D, "hidden": H, "seq_len": T, "layers": L, "last_loss_hip": st.loss,
           "mean_session_length": round(float(np.mean([np.mean(b[2]) for b in batches])), 1),
           # forward + dgrad + wgrad, 2 flops per multiply-add: the input projection, the recurrence, a_1, the catalogue
           "gemm_gflop_per_step": round(3 * 2 * (M * 3 * H * (D + H) + M * H * H + B * I * D) / 1e9, 2),
           "saved_activation_mb": round(L * M * (4 * H + H) * 4 / 1e6, 1)}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 1) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
        out[f"{k}_peak_memory_mb"] = round(peak[k], 1)
    if "torch" in times:
        out["hip_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
        out["hip_not_slower_than_torch"] = bool(out["hip_us_per_step_median"] <= 1.05 * out["torch_us_per_step_median"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_narm.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_narm.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "optimizer": "adam", "dropout": [P_IN, P_HID],
           "steps_per_window": args.windows * args.steps, "repeats": args.repeats, "shapes": {}}
    for name in args.shapes.split(","):
        out["shapes"][name] = measure(name, args=args, hp=hp, dev=dev, **SHAPES[name])
        print(name, json.dumps(out["shapes"][name]), flush=True)
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
