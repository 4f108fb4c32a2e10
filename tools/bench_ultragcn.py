"""Measure the UltraGCN training step on the GPU: the HIP engine against the reference's own op sequence on torch.

    python tools/bench_ultragcn.py [--epochs 3] [--warmup 1] [--repeats 5] [--out profiles/ultragcn_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_ultragcn.py --hip-only --repeats 1   # kernel times

Two shapes on ML-100K-sized tables (943 x 1682, D 64, B 1000, K 10): the reference's default N = 20 and the paper's
N = 300.  A window is ``--epochs`` whole epochs over the resident (user, pos, neg[N]) arrays (100 steps each) between two
device synchronisations; HIP and torch windows alternate ``--repeats`` times in one process, so both see the same machine
state.  There is no earlier number for this model, so the yardstick is the reference's op sequence (nn.Embedding +
autograd + torch.optim.Adam, models/ultragcn.py:72-165 restated here, nothing imported from the reference) WITHOUT the
``.item()`` the reference pays per step.  Needs a GPU: there is no CPU timing path.

Byte model printed with the result: gather / scatter bytes B (2 + N + K) 4D per step (what the gradient kernel adds by
float atomics; bound: the chip-wide float-atomic rate) and sweep bytes 32 (U + I) D for Adam (bound: HBM).
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

ATOMIC_RATE = 1.3e12   # B/s of added bytes, chip-wide float-atomic rate of the MI355X
HBM_RATE = 6.29e12     # B/s measured float4 copy
HP = {"w1": 1e-7, "w2": 1.0, "w3": 1e-7, "w4": 1.0, "negative_weight": 200.0, "gamma": 1e-4, "lambda": 1e-3}
U, I, D, B, K = 943, 1682, 64, 1000, 10
SHAPES = {"default_n20": 20, "paper_n300": 300}


def frame(seed=0, per_user=106):
    """~100k interactions with skewed item popularity; every user and item occurs."""
    rng = np.random.default_rng(seed)
    pop = 1.0 / np.arange(1, I + 1) ** 0.8
    pop /= pop.sum()
    items = np.concatenate([rng.choice(I, per_user, replace=False, p=pop) for _ in range(U)])
    users = np.repeat(np.arange(U), per_user)
    items[:I] = np.arange(I)
    return users, items


def constants(users, items):
    import scipy.sparse as sp

    import beta_recsys_amd as hp

    M = sp.csr_matrix((np.ones(len(users), dtype=np.float32), (users, items)), shape=(U, I))
    M.data[:] = 1.0
    items_D, users_D = np.asarray(M.sum(axis=0)).reshape(-1), np.asarray(M.sum(axis=1)).reshape(-1)
    bu = (np.sqrt(users_D + 1) / users_D).astype(np.float32)
    bi = (1 / np.sqrt(items_D + 1)).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        nbr, sim = hp.get_ii_constraint_mat(M, K)
    return M, bu, bi, nbr, sim


class TorchUltraGCN(torch.nn.Module):
    """The reference's op sequence (models/ultragcn.py:72-165) on whatever device it is moved to."""

    def __init__(self, bu, bi, nbr, sim):
        super().__init__()
        self.user_embeds = torch.nn.Embedding(U, D)
        self.item_embeds = torch.nn.Embedding(I, D)
        for name, t in (("bu", bu), ("bi", bi), ("nbr", nbr), ("sim", sim)):
            self.register_buffer(name, torch.as_tensor(t))

    def forward(self, users, pos, neg):
        F = torch.nn.functional
        pos_w = HP["w1"] + HP["w2"] * (self.bu[users] * self.bi[pos])
        neg_w = HP["w3"] + HP["w4"] * (torch.repeat_interleave(self.bu[users], neg.size(1)) * self.bi[neg.flatten()])
        ue, pe, ne = self.user_embeds(users), self.item_embeds(pos), self.item_embeds(neg)
        pos_scores = (ue * pe).sum(dim=-1)
        neg_scores = (ue.unsqueeze(1) * ne).sum(dim=-1)
        neg_loss = F.binary_cross_entropy_with_logits(neg_scores, torch.zeros_like(neg_scores),
                                                      weight=neg_w.view(neg_scores.size()), reduction="none").mean(dim=-1)
        pos_loss = F.binary_cross_entropy_with_logits(pos_scores, torch.ones_like(pos_scores), weight=pos_w,
                                                      reduction="none")
        loss = (pos_loss + neg_loss * HP["negative_weight"]).sum()
        norm = sum(torch.sum(p ** 2) for p in self.parameters()) / 2
        nb = self.item_embeds(self.nbr[pos])
        loss_i = (-self.sim[pos] * (ue.unsqueeze(1) * nb).sum(dim=-1).sigmoid().log()).sum()
        return loss + HP["gamma"] * norm + HP["lambda"] * loss_i


def hip_engine(bu, bi, nbr, sim, w0):
    import beta_recsys_amd as hp

    model = dict(n_users=U, n_items=I, emb_dim=D, batch_size=B, regs=[1e-5], optimizer="adam", lr=1e-3,
                 device_str="cuda:0", constraint_mat={"beta_uD": bu, "beta_iD": bi}, ii_neighbor_num=K,
                 ii_neighbor_mat=nbr, ii_constraint_mat=sim, **HP)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.UltraGCNEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_bench_runs"}})
    eng.model.load_state_dict(w0)
    return eng


def run_shape(name, n_neg, args, users, items, consts, dev):
    _, bu, bi, nbr, sim = consts
    rng = np.random.default_rng(n_neg)
    cols = [torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev),
            torch.from_numpy(rng.integers(0, I, (len(users), n_neg))).to(dev)]
    steps = (len(users) + B - 1) // B
    torch.manual_seed(0)
    ref = TorchUltraGCN(bu, bi, nbr, sim)
    w0 = {"user_embeds.weight": ref.user_embeds.weight.detach().clone() * 0.5,
          "item_embeds.weight": ref.item_embeds.weight.detach().clone() * 0.5}
    ref.load_state_dict(w0, strict=False)
    ref.to(dev)
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    eng = hip_engine(bu, bi, nbr, sim, w0)

    def hip_epoch():
        eng.enqueue_epoch(cols[0], cols[1], cols[2], B)

    def torch_epoch():
        for off in range(0, len(users), B):
            opt.zero_grad()
            loss = ref(cols[0][off:off + B], cols[1][off:off + B], cols[2][off:off + B])
            loss.backward()
            opt.step()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.epochs):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (args.epochs * steps) * 1e6   # us per step

    sides = {"hip": hip_epoch} if args.hip_only else {"hip": hip_epoch, "torch": torch_epoch}
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn))
    st = eng._sync_stats()
    gather = B * (2 + n_neg + K) * 4 * D
    sweep = 32 * (U + I) * D
    floor_us = (gather / ATOMIC_RATE + sweep / HBM_RATE) * 1e6
    out = {"shape": name, "n_users": U, "n_items": I, "emb_dim": D, "batch": B, "n_neg": n_neg, "n_neighbors": K,
           "optimizer": "adam", "steps_per_epoch": steps, "epochs_per_window": args.epochs, "repeats": args.repeats,
           "gather_scatter_bytes_per_step": gather, "sweep_bytes_per_step": sweep,
           "floor_us": round(floor_us, 2),
           "floor_is": "atomic rate (gradient scatter) + HBM (optimizer sweep), two dependent launches",
           "last_epoch_loss_sum_hip": st.loss_sum}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 2) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 2)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
    out["fraction_of_floor"] = round(floor_us / out["hip_us_per_step_median"], 4)
    if "torch" in times:
        out["speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out["hip_us_per_step_median"], 2)
        out["hip_beats_torch_beyond_spread"] = bool(max(times["hip"]) < min(times["torch"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_ultragcn.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__

    dev = torch.device("cuda:0")
    users, items = frame()
    consts = constants(users, items)
    result = {"tool": "tools/bench_ultragcn.py", "device": torch.cuda.get_device_name(0),
              "source_hash": __graft_entry__.source_hash(), "shapes": []}
    for name in args.shapes.split(","):
        result["shapes"].append(run_shape(name, SHAPES[name], args, users, items, consts, dev))
        print(json.dumps(result["shapes"][-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
