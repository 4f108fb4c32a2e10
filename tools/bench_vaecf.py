"""Measure the VAECF training step on the GPU: the HIP engine against the reference's own op sequence on torch.

    python tools/bench_vaecf.py [--steps 4] [--warmup 2] [--repeats 5] [--out profiles/vaecf_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_vaecf.py --sides hip_strided --repeats 1 --shapes default

Shapes: ``default`` is configs/vaecf_default.json on ml_100k (943 users x 1682 items, batch 1000: one step holds all 943
rows, ~100 nonzeros each); ``large_catalogue`` has n_items = 50 000 at B = 1000 with ~100 nonzeros per row; ``limits``
the kernels' limits (z_dim 256, three hidden layers of 512) on 20 000 items at B = 1000.  All train mult / tanh / beta 1
with Adam, the reference's defaults, at lr 1e-3 (a window repeats the same few batches thousands of times; at the default
0.05 the widest shape's KL term overflows).  ``--steps`` batches of rows are staged once: as a device CSR for the HIP
sides, as a scipy CSR matrix on the host for the torch side.  A window is as many passes over those batches as last a quarter of a
second (calibrated per side on the warm-up) between two device synchronisations; the sides alternate ``--repeats`` times
in one process, so all see the same machine state.  Sides:
  hip_strided  VAECFEngine's launches (hiprec_vaecf_grad + the dense optimizer sweep) with ``noise_rng = "device"``,
               python-looped, no host sync; the first layer gathers the columns of W0 as they lie
  hip_shadow   the same with ``w0_gather = "shadow"``: W0 is transposed into the workspace every step
  torch        the reference's op sequence (vaecf.py:45-87, 134-163 restated here, nothing imported from the reference):
               per step ``matrix[uids].toarray()`` on the host, the upload, nn.Linear / softmax / log / autograd /
               torch.optim.Adam on the GPU -- the host densification is part of what a user of the reference pays --
               without ``loss.item()``
Recorded per side: the median time per step and the peak device memory above what was allocated before the side's first
step; for the HIP sides also the time of the first-layer gather alone (the kernel the two forms differ in, plus the
transpose of the shadow form).  There is no earlier number for this model: the yardstick is the torch side of the same
run.  Needs a GPU.
"""
import argparse
import contextlib
import ctypes
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

LR, BETA, ACT, LIK = 1e-3, 1.0, "tanh", "mult"
SHAPES = {"default": dict(U=943, I=1682, B=1000, nnz_row=100, Z=10, hidden=[20]),
          "large_catalogue": dict(U=4000, I=50000, B=1000, nnz_row=100, Z=10, hidden=[20]),
          "limits": dict(U=4000, I=20000, B=1000, nnz_row=100, Z=256, hidden=[512, 512, 512])}
MIN_WINDOW_S = 0.25


class TorchVAE(torch.nn.Module):
    """models/vaecf.py:9-87 (mult, tanh) on whatever device it is moved to."""

    def __init__(self, I, Z, hidden):
        super().__init__()
        nn = torch.nn
        enc = [I] + hidden
        self.encoder = nn.Sequential()
        for i in range(len(enc) - 1):
            self.encoder.add_module(f"fc{i}", nn.Linear(enc[i], enc[i + 1]))
            self.encoder.add_module(f"act{i}", nn.Tanh())
        self.enc_mu = nn.Linear(enc[-1], Z)
        self.enc_logvar = nn.Linear(enc[-1], Z)
        dec = [Z] + enc[::-1]
        self.decoder = nn.Sequential()
        for i in range(len(dec) - 1):
            self.decoder.add_module(f"fc{i}", nn.Linear(dec[i], dec[i + 1]))
            if i != len(dec) - 2:
                self.decoder.add_module(f"act{i}", nn.Tanh())

    def forward(self, x):
        h = self.encoder(x)
        mu, logvar = self.enc_mu(h), self.enc_logvar(h)
        std = torch.exp(0.5 * logvar)
        z = mu + torch.randn_like(mu) * std
        x_ = torch.softmax(self.decoder(z), dim=1)
        ll = torch.sum(x * torch.log(x_ + 1e-10), dim=1)
        std = torch.exp(0.5 * logvar)
        kld = torch.sum(-0.5 * (1 + 2.0 * torch.log(std) - mu.pow(2) - std.pow(2)), dim=1)
        return torch.mean(BETA * kld - ll)


def interactions(U, I, nnz_row, seed=1):
    from scipy.sparse import csr_matrix

    rng = np.random.default_rng(seed)
    cols = rng.integers(0, I, (U, nnz_row))
    rows = np.repeat(np.arange(U), nnz_row)
    m = csr_matrix((np.ones(U * nnz_row, dtype=np.float32), (rows, cols.ravel())), shape=(U, I))
    m.data[:] = 1.0
    return m


def measure(name, U, I, B, nnz_row, Z, hidden, args, hp, dev):
    from beta_recsys_amd import _lib
    from beta_recsys_amd.vaecf import _Csr, _history_csr

    torch.manual_seed(0)
    matrix = interactions(U, I, nnz_row)
    ref = TorchVAE(I, Z, hidden)
    w0 = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    starts = [(s * B) % max(1, U - min(B, U) + 1) for s in range(args.steps)]
    rows = min(B, U)
    engines = {}
    for gather in ("strided", "shadow"):
        cfg = {"model": {"n_users": U, "n_items": I, "activation": ACT, "likelihood": LIK, "batch_size": B, "lr": LR,
                         "beta": BETA, "weight_decay": 0.0, "optimizer": "adam", "device_str": "cuda:0", "z_dim": Z,
                         "hidden": hidden, "noise_rng": "device", "w0_gather": gather},
               "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
        with contextlib.redirect_stdout(io.StringIO()):
            eng = hp.VAECFEngine(cfg)
        eng.model.load_state_dict(w0)
        eng.model.train()
        engines[gather] = eng
    ptr, items, values = _history_csr(matrix, U, dev)
    batches = [_Csr(ptr[s:s + rows + 1], items, values, rows, items.numel()) for s in starts]
    state = {}

    def hip(gather):
        def run():
            for b in batches:
                engines[gather]._enqueue_step(b)
        return run

    def torch_steps():
        if "opt" not in state:                  # built on first use, so that a side's peak memory is its own
            ref.to(dev)
            state["opt"] = torch.optim.Adam(ref.parameters(), lr=LR, weight_decay=0.0)
        for s in starts:
            u_batch = matrix[np.arange(s, s + rows), :]
            u_batch.data = np.ones(len(u_batch.data))
            x = torch.tensor(u_batch.toarray(), dtype=torch.float32, device=dev)
            state["opt"].zero_grad()
            ref(x).backward()
            state["opt"].step()

    def first_layer(gather):
        """The gather alone (and the shadow's transpose): hiprec_vaecf_encode stops after it only in a profile, so the
        two forms are compared on the inference encoder, whose other stages are the same small GEMMs for both."""
        m = engines[gather].model

        def run():
            for b in batches:
                m._encode_csr(b[0], b[1], b[2], b[3], b[4])
        return run

    def window(fn, passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(passes):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    sides = {"hip_strided": hip("strided"), "hip_shadow": hip("shadow"),
             "encode_strided": first_layer("strided"), "encode_shadow": first_layer("shadow")}
    if not args.hip_only:
        sides["torch"] = torch_steps
    if args.sides:
        sides = {k: sides[k] for k in args.sides.split(",")}
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
    st = engines["strided"]._sync_stats() if "hip_strided" in sides else engines["shadow"]._sync_stats()
    h0 = hidden[0]
    lib = _lib.load()
    out = {"n_users": U, "n_items": I, "rows_per_step": rows, "nnz_per_step": int(matrix[:rows].nnz), "z_dim": Z,
           "hidden": hidden, "last_ll_hip": st.loss, "last_kld_hip": st.reg,
           # 2 flops per multiply-add: the last layer's logits twice (pass A, pass B), dHd and dW_L
           "last_layer_gflop_per_step": round(2 * 4 * rows * I * h0 / 1e9, 3),
           "workspace_mb": {g: round(lib.hiprec_vaecf_workspace_bytes(ctypes.byref(engines[g].model.shape), rows,
                                                                      int(matrix[:rows].nnz)) / 1e6, 2)
                            for g in engines},
           "dense_batch_mb": round(4 * rows * I / 1e6, 1),
           "steps_per_window": {k: passes[k] * len(batches) for k in sides}}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 1) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
        out[f"{k}_peak_memory_mb"] = round(peak[k], 1)
    if "hip_strided" in times and "hip_shadow" in times:
        out["faster_gather"] = min(("hip_strided", "hip_shadow"), key=lambda k: out[f"{k}_us_per_step_median"])
    if "torch" in times and "hip_strided" in times:
        out["hip_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_strided_us_per_step_median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--sides", default=None, help="comma-separated subset of the sides (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_vaecf.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    out = {"tool": "tools/bench_vaecf.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "optimizer": "adam", "beta": BETA, "activation": ACT,
           "likelihood": LIK, "min_window_s": MIN_WINDOW_S, "repeats": args.repeats, "shapes": {}}
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
