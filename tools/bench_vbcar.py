"""Measure the VBCAR training step on the GPU: the HIP engine against the reference's own op sequence on torch.

    python tools/bench_vbcar.py [--steps 8] [--warmup 2] [--repeats 5] [--out profiles/vbcar_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_vbcar.py --hip-only --repeats 1   # kernel times

Shapes: ``default`` is configs/vbcar_default.json (batch 256, n_neg 5, 512-wide random features, late_dim 256, emb_dim
64) on tafeng-like table sizes (U 30 000, I 20 000); ``batch4096`` the same widths at batch 4096; ``limits`` the
kernels' limits (emb_dim 128, late_dim 512) with 2048-wide features at batch 1024.  All train with RMSprop, alpha 0.001
and tanh, the reference's defaults.  ``--steps`` batches of uniformly drawn triples and negatives are staged on the device
once.  A window is as many passes over those batches as last a quarter of a second (calibrated per side on the warm-up)
between two device synchronisations; the sides alternate ``--repeats`` times in one process, so both see the same
machine state.  Sides:
  hip     VBCAREngine's launches (hiprec_vbcar_grad + the dense optimizer sweep) with ``noise_rng = "device"`` (one
          torch.randn per step on the GPU), python-looped, no host sync
  torch   the reference's op sequence (models/vbcar.py:55-178, 219-227 restated here, nothing imported from the
          reference: feature indexing / nn.Linear / torch.randn_like on the GPU / nn.Embedding / bmm / logsigmoid /
          kl_div + autograd + torch.optim.RMSprop) WITHOUT the two host syncs the reference pays per step
          (``KLD.item()``, ``GEN.item()``) and without ``loss.item()``
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LR, ALPHA, ACT = 5e-4, 0.001, "tanh"
SHAPES = {"default": dict(U=30000, I=20000, B=256, n_neg=5, D=64, L=256, Fu=512, Fi=512),
          "batch4096": dict(U=30000, I=20000, B=4096, n_neg=5, D=64, L=256, Fu=512, Fi=512),
          "limits": dict(U=30000, I=20000, B=1024, n_neg=5, D=128, L=512, Fu=2048, Fi=2048)}
MIN_WINDOW_S = 0.25


class TorchVBCAR(torch.nn.Module):
    """models/vbcar.py:9-178 on whatever device it is moved to."""

    def __init__(self, U, I, D, L, Fu, Fi, n_neg, batch_size, user_fea, item_fea):
        super().__init__()
        nn = torch.nn
        self.emb_dim, self.n_neg, self.batch_size, self.esp = D, n_neg, batch_size, 1e-10
        self.user_fea, self.item_fea = user_fea, item_fea
        self.user_emb = nn.Embedding(U, D)
        self.item_emb = nn.Embedding(I, D)
        self.item_emb.weight.data.uniform_(-0.1 * D ** -0.5, 0.1 * D ** -0.5)
        self.fc_u_1_mu = nn.Linear(Fu, L)
        self.fc_u_2_mu = nn.Linear(L, 2 * D)
        self.fc_i_1_mu = nn.Linear(Fi, L)
        self.fc_i_2_mu = nn.Linear(L, 2 * D)

    def to(self, dev):
        self.user_fea, self.item_fea = self.user_fea.to(dev), self.item_fea.to(dev)
        return super().to(dev)

    def encode(self, fea, fc1, fc2, index):
        x = fc2(torch.tanh(fc1(fea[index])))
        return x[:, :self.emb_dim], x[:, self.emb_dim:]

    @staticmethod
    def reparameterize(gaussian):
        mu, std = gaussian
        std = torch.exp(0.5 * std)
        return mu + std * torch.randn_like(std)

    def kl_div(self, dis):
        mean1, std1 = dis
        mean2, std2 = torch.zeros_like(mean1), torch.ones_like(mean1)
        var1, var2 = std1.pow(2) + self.esp, std2.pow(2) + self.esp
        mean_pow2 = (mean2 - mean1) * (1.0 / var2) * (mean2 - mean1)
        return (torch.log(var2 / var1) - 1 + (1.0 / var2) * var1 + mean_pow2).mul(0.5).sum(dim=1).mean()

    def forward(self, batch):
        pos_u, pos_i_1, pos_i_2, neg_u, neg_i_1, neg_i_2 = batch
        D2, n = 2 * self.emb_dim, self.n_neg
        ue = lambda ix: self.encode(self.user_fea, self.fc_u_1_mu, self.fc_u_2_mu, ix)   # noqa: E731
        ie = lambda ix: self.encode(self.item_fea, self.fc_i_1_mu, self.fc_i_2_mu, ix)   # noqa: E731
        du, d1, d2 = ue(pos_u), ie(pos_i_1), ie(pos_i_2)
        emb_u = torch.cat((self.reparameterize(du), self.user_emb(pos_u)), dim=1)
        emb_1 = torch.cat((self.reparameterize(d1), self.item_emb(pos_i_1)), dim=1)
        emb_2 = torch.cat((self.reparameterize(d2), self.item_emb(pos_i_2)), dim=1)
        dnu, dn1, dn2 = ue(neg_u.view(-1)), ie(neg_i_1.view(-1)), ie(neg_i_2.view(-1))
        neg_eu = torch.cat((self.reparameterize(dnu), self.user_emb(neg_u.view(-1))), dim=1).view(-1, n, D2)
        neg_e1 = torch.cat((self.reparameterize(dn1), self.item_emb(neg_i_1.view(-1))), dim=1).view(-1, n, D2)
        neg_e2 = torch.cat((self.reparameterize(dn2), self.item_emb(neg_i_2.view(-1))), dim=1).view(-1, n, D2)
        total = 0.0
        for e, other, neg in ((emb_u, emb_1 + emb_2, neg_eu), (emb_1, emb_u + emb_2, neg_e1), (emb_2, emb_u + emb_1, neg_e2)):
            pos = F.logsigmoid(torch.sum(torch.mul(e, other).squeeze(), dim=1))
            ng = F.logsigmoid(-1 * torch.bmm(neg, e.unsqueeze(2)).squeeze())
            total = total + -1 * (torch.sum(pos) + torch.sum(ng))
        GEN = total / (3 * self.batch_size)
        KLD = sum(self.kl_div(d) for d in (du, d1, d2, dnu, dn1, dn2)) / (3 * self.batch_size)
        return (1 - ALPHA) * GEN + ALPHA * KLD


def batches_on(dev, steps, U, I, B, n_neg, seed=1):
    rng = np.random.default_rng(seed)
    return [tuple(torch.from_numpy(rng.integers(0, n, shape)).to(dev)
                  for n, shape in ((U, B), (I, B), (I, B), (U, (B, n_neg)), (I, (B, n_neg)), (I, (B, n_neg))))
            for _ in range(steps)]


def measure(name, U, I, B, n_neg, D, L, Fu, Fi, args, hp, dev):
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    fea = (torch.from_numpy(rng.standard_normal((U, Fu)).astype(np.float32)),
           torch.from_numpy(rng.standard_normal((I, Fi)).astype(np.float32)))
    ref = TorchVBCAR(U, I, D, L, Fu, Fi, n_neg, B, *fea)
    w0 = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    cfg = {"model": {"n_users": U, "n_items": I, "late_dim": L, "emb_dim": D, "n_neg": n_neg, "batch_size": B,
                     "alpha": ALPHA, "activator": ACT, "optimizer": "rmsprop", "lr": LR, "device_str": "cuda:0",
                     "noise_rng": "device"},
           "user_fea": fea[0], "item_fea": fea[1], "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.VBCAREngine(cfg)
    eng.model.load_state_dict(w0)
    eng.model.train()
    batches = batches_on(dev, args.steps, U, I, B, n_neg)
    state = {}

    def hip():
        for b in batches:
            eng._enqueue_step(b)

    def torch_steps():
        if "opt" not in state:                  # built on first use, so that a side's peak memory is its own
            ref.to(dev)
            state["opt"] = torch.optim.RMSprop(ref.parameters(), lr=LR)
        for b in batches:
            state["opt"].zero_grad()
            ref(b).backward()
            state["opt"].step()

    def window(fn, passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(passes):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    sides = {"hip": hip}
    if not args.hip_only:
        sides["torch"] = torch_steps
    peak, passes = {}, {}
    for k, fn in sides.items():
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - before) / 1e6
        passes[k] = max(1, int(np.ceil(MIN_WINDOW_S / max(window(fn, 1), 1e-6))))
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn, passes[k]) / (passes[k] * len(batches)) * 1e6)   # us per step
    st = eng._sync_stats()
    Ru, Ri = B * (1 + n_neg), 2 * B * (1 + n_neg)
    out = {"n_users": U, "n_items": I, "batch": B, "n_neg": n_neg, "emb_dim": D, "late_dim": L, "fea": [Fu, Fi],
           "user_rows": Ru, "item_rows": Ri, "last_rec_loss_hip": st.loss, "last_kl_loss_hip": st.reg,
           # 2 flops per multiply-add: fc_1 forward + wgrad (no dX), fc_2 forward + dgrad + wgrad
           "gemm_gflop_per_step": round(2 * (2 * L * (Ru * Fu + Ri * Fi) + 3 * (Ru + Ri) * L * 2 * D) / 1e9, 3),
           "workspace_mb": round(eng.model._ws.numel() / 1e6, 1),
           "steps_per_window": {k: passes[k] * len(batches) for k in sides}}
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
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_vbcar.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_vbcar.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "optimizer": "rmsprop", "alpha": ALPHA, "activator": ACT,
           "min_window_s": MIN_WINDOW_S, "repeats": args.repeats, "shapes": {}}
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
