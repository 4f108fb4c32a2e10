"""Measure the BUIR training step on the GPU: the HIP engine against the reference's step written in torch autograd.

    python tools/bench_buir.py [--repeats 5] [--out profiles/buir_step.json]

Two shapes, Adam, L 3 (the reference's hard-coded depth), the shapes of profiles/simgcl_step.json:
  * ``ml100k``: 943 x 1682, D 64, B 1000, 100 000 interactions;
  * ``ml1m``: 6040 x 3706, D 64, B 4096, 1 000 000 interactions.
The interactions are random with Zipf item degrees; the graph is D^-1/2 A D^-1/2 (tools/bench_simgcl.random_graph).  The
yardstick is the reference's op sequence (buir.py:56-77, :149-178, :215-233 restated here in torch ops: BOTH encoders
propagate with ``torch.sparse.mm`` in every step, the target without gradient, one ``nn.Linear``, four ``F.normalize``;
nothing imported from the reference) with ``backward()`` and ``torch.optim.Adam``, on the same GPU.  Unlike the
reference, the restatement keeps ``norm_adj`` on the device -- the reference's own path does not run on a GPU at all.

Windows, warm-up, repeats, peak memory and the kernel shares are tools/bench_simgcl.py's.  ``spmm_per_step`` is derived,
not measured, and asserted: L forward + L backward here against 2 L + L.  Needs a GPU.

Not measured: hardware counters, anything multi-GPU, the moving target (``update_target``: one elementwise pass more).
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
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_simgcl import kernel_shares, random_graph, timed_window  # noqa: E402

LR, MOMENTUM, L = 0.001, 0.995, 3
#            U     I     D   B     interactions
SHAPES = {"ml100k": (943, 1682, 64, 1000, 100_000), "ml1m": (6040, 3706, 64, 4096, 1_000_000)}


class TorchBUIR(torch.nn.Module):
    """The step of models/buir.py in torch ops, on whatever device it is moved to."""

    def __init__(self, U, I, D, adj):
        super().__init__()
        self.U, self.I, self.adj = U, I, adj
        self.online = torch.nn.ParameterList([torch.nn.Parameter(torch.nn.init.xavier_uniform_(torch.empty(n, D)))
                                              for n in (U, I)])
        self.target = torch.nn.ParameterList([torch.nn.Parameter(p.detach().clone(), requires_grad=False)
                                              for p in self.online])
        self.predictor = torch.nn.Linear(D, D)
        self.spmm_calls = 0

    def encode(self, tables, users, items):
        e = torch.cat(list(tables), dim=0)
        hops = [e]
        for _ in range(L):
            e = torch.sparse.mm(self.adj, e)
            self.spmm_calls += 1
            hops.append(e)
        ru, ri = torch.split(torch.mean(torch.stack(hops, dim=1), dim=1), [self.U, self.I])
        return ru[users], ri[items]

    def forward(self, users, pos, neg):
        xu, xi = self.encode(self.online, users, pos)
        tu, ti = self.encode(self.target, users, pos)
        yu, yi = F.normalize(self.predictor(xu), dim=-1), F.normalize(self.predictor(xi), dim=-1)
        tu, ti = F.normalize(tu, dim=-1), F.normalize(ti, dim=-1)
        return ((2 - 2 * (yu * ti).sum(dim=-1)) + (2 - 2 * (yi * tu).sum(dim=-1))).mean()


def run_shape(name, args, dev):
    import beta_recsys_amd as hp

    U, I, D, B, n_inter = SHAPES[name]
    rng = np.random.default_rng(B)
    users, items, adj = random_graph(U, I, n_inter, rng)
    n_batches = 8
    picks = [rng.integers(0, users.size, B) for _ in range(n_batches)]
    batches = [(torch.from_numpy(users[p]).to(dev), torch.from_numpy(items[p]).to(dev),
                torch.from_numpy(rng.integers(0, I, B)).to(dev)) for p in picks]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    torch.manual_seed(0)
    model = dict(n_users=U, n_items=I, emb_dim=D, n_layers=L, momentum=MOMENTUM, norm_adj=adj, optimizer="adam", lr=LR,
                 device_str="cuda:0", batch_size=B)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.BUIREngine({"model": model, "system": {"run_dir": "/tmp/hiprec_bench_runs"}})
    eng.model.train()
    eng._setup()

    def hip_steps(n):
        for s in range(n):
            eng._enqueue_step(batches[s % n_batches])

    sides = {"hip": hip_steps}
    peaks, times, steps = {}, {"hip": []}, {}
    hip_steps(args.warmup)
    steps["hip"] = max(args.warmup, int(args.min_window * 1e6 / timed_window(hip_steps, args.warmup)))
    torch.cuda.synchronize()
    peaks["hip"] = torch.cuda.max_memory_allocated() - base
    hip_resident = torch.cuda.memory_allocated() - base
    spmm = {"forward": L, "backward": L, "reference": 3 * L}
    if not args.hip_only:
        base_t = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        coo = adj.tocoo()
        tadj = torch.sparse_coo_tensor(np.vstack([coo.row, coo.col]).astype(np.int64), coo.data, (U + I, U + I)).coalesce().to(dev)
        ref = TorchBUIR(U, I, D, tadj).to(dev)
        opt = torch.optim.Adam([p for p in ref.parameters() if p.requires_grad], lr=LR)

        def torch_steps(n):
            for s in range(n):
                opt.zero_grad()
                ref(*batches[s % n_batches]).backward()
                opt.step()

        sides["torch"] = torch_steps
        times["torch"] = []
        torch_steps(max(2, args.warmup // 4))
        ref.spmm_calls = 0
        torch_steps(1)
        # the reference's forward calls 2 L SpMMs; autograd adds L for the online chain (the target takes no gradient)
        assert ref.spmm_calls == 2 * L and spmm["reference"] == ref.spmm_calls + L
        steps["torch"] = max(2, int(args.min_window * 1e6 / timed_window(torch_steps, 2)))
        torch.cuda.synchronize()
        peaks["torch"] = torch.cuda.max_memory_allocated() - base_t
    assert spmm["forward"] + spmm["backward"] == 2 * L < spmm["reference"]
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(timed_window(fn, steps[k]))
    st = eng._sync_stats()
    out = {"n_users": U, "n_items": I, "nnz": int(adj.nnz), "emb_dim": D, "n_layers": L, "batch": B, "optimizer": "adam",
           "repeats": args.repeats, "steps_per_window": steps, "spmm_per_step": spmm,
           "workspace_bytes": int(eng.model._ws["ws"].numel() * 4),
           "batch_workspace_bytes": int(eng.model._ws["batch_ws"].numel() * 4), "hip_resident_bytes": int(hip_resident),
           "last_loss_hip": st.loss}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 1) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 1)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
        out[f"{k}_peak_bytes"] = int(peaks[k])
    if "torch" in times:
        out["speedup_vs_torch"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
        out["hip_beats_torch_beyond_spread"] = bool(max(times["hip"]) < min(times["torch"]))
        out["peak_bytes_saved"] = int(peaks["torch"] - peaks["hip"])
    out["kernel_shares"] = None if args.no_shares else kernel_shares(hip_steps)
    out["not_measured"] = ["hardware counters", "multi-GPU", "update_target"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--min-window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side")
    ap.add_argument("--no-shares", action="store_true", help="skip the per-kernel shares")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_buir.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__

    dev = torch.device("cuda:0")
    result = {"tool": "tools/bench_buir.py", "device": torch.cuda.get_device_name(0),
              "source_hash": __graft_entry__.source_hash(), "shapes": {}}
    for name in args.shapes.split(","):
        result["shapes"][name] = run_shape(name, args, dev)
        print(json.dumps({name: result["shapes"][name]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
