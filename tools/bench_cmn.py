"""Measure the CMN training step on the GPU: the HIP engine against the reference's own op sequence on torch.

    python tools/bench_cmn.py [--steps 20] [--windows 3] [--warmup 1] [--repeats 5] [--out profiles/cmn_step.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_cmn.py --hip-only --repeats 1   # kernel times

Shape: ``cmn_default.json`` hyper-parameters (D 64, batch 1024, neg_count 4, Adam lr 1e-4, grad_clip 5, lambda 1e-3) on a
synthetic ML-100K-shaped graph (943 x 1682, 100 000 interactions, Zipf item popularity).  ``--steps`` batches are staged
on the device once: every positive ``neg_count`` times in a row with uniform negatives, as ``cmn_train_loader`` emits
them, for the torch side also as the padded ``[B, max_neighbors]`` neighbourhood matrices the loader builds.  A window is
``--windows`` passes over those batches between two device synchronisations; the sides alternate ``--repeats`` times in
one process, so all see the same machine state.  Sides:
  hip_csr      hiprec_cmn_epoch: resident triples, lists from the item -> users CSR, every step enqueued from C
  hip_padded   train_single_batch's launches on the padded matrices, python-looped, no host sync
  torch        the reference's op sequence (models/cmn.py:69-200, models/vlml.py restated here, nothing imported from
               the reference: nn.Embedding + autograd + clip_grad_norm_ + torch.optim.Adam) WITHOUT the two host syncs
               the reference pays per step (``torch.max(seq_length).item()`` and ``batch_loss.item()``): the longest
               list of every batch is handed over as a python int
There is no earlier number for this model: the condition is hip <= torch beyond the run-to-run spread.  Needs a GPU.

Printed with the result: the batches' total and longest list lengths and the float-atomic bytes of a step,
sum over queries of L * D * 4 * 2 (one add per list slot into dM, one into dC: both hops' terms are combined first)
+ 2 * 2B * D * 4 for the query rows; bound: the chip-wide float-atomic rate.
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
U, I, D, B, NEG = 943, 1682, 64, 1024, 4
LR, LAM, CLIP = 1e-4, 1e-3, 5.0


def frame(seed=0, n=100_000):
    """~100 000 unique (user, item) pairs with Zipf item popularity; every item occurs."""
    rng = np.random.default_rng(seed)
    pop = 1.0 / np.arange(1, I + 1) ** 0.8
    pop /= pop.sum()
    key = np.unique(rng.integers(0, U, 3 * n) * I + rng.choice(I, 3 * n, p=pop))
    every_item = rng.integers(0, U, I) * I + np.arange(I)
    keep = np.unique(np.concatenate([key[rng.permutation(key.size)][:n - I], every_item]))
    return keep // I, keep % I


class TorchCMN(torch.nn.Module):
    """models/cmn.py:12-121 + models/vlml.py on whatever device it is moved to."""

    def __init__(self, max_neighbors):
        super().__init__()
        nn = torch.nn
        self.user_memory, self.item_memory, self.user_output = nn.Embedding(U, D), nn.Embedding(I, D), nn.Embedding(U, D)
        self.hop = nn.Linear(D, D)
        self.dense = nn.Linear(2 * D, D)
        self.out = nn.Linear(D, 1, bias=False)
        self.max_neighbors = max_neighbors

    def attend(self, memory, output_memory, query, lens, cur_max):
        scores = (query.unsqueeze(-1).transpose(2, 1) * memory).sum(2)
        maxlen = self.max_neighbors
        mask = (torch.arange(maxlen, device=lens.device).expand(len(lens), maxlen) < lens.unsqueeze(1)).float()
        finfo = np.finfo(np.float32)
        lower = float(finfo.max) * mask + float(finfo.min) * (mask < 1).float()
        scores = torch.min(scores[:, :cur_max], lower[:, :cur_max])
        attention = torch.nn.functional.softmax(scores, dim=-1)
        return (output_memory.transpose(2, 1) * attention.unsqueeze(1)).sum(2)

    def query(self, cur_user, cur_item, nbr, lens, cur_max):
        memory, output_memory = self.user_memory(nbr)[:, :cur_max], self.user_output(nbr)[:, :cur_max]
        z = cur_user + cur_item
        o = self.attend(memory, output_memory, z, lens, cur_max)
        z = torch.relu(self.hop(z) + o)
        o = self.attend(memory, output_memory, z, lens, cur_max)
        return self.out(torch.relu(self.dense(torch.cat((cur_user * cur_item, o), 1)))).squeeze()

    def forward(self, users, pos, neg, pn, pl, nn_, nl, pmax, nmax):
        cur_user = self.user_memory(users)
        return (self.query(cur_user, self.item_memory(pos), pn, pl, pmax),
                self.query(cur_user, self.item_memory(neg), nn_, nl, nmax))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true", help="skip the torch side (for a kernel-trace run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_cmn.py measures on the GPU; no GPU found and there is no CPU timing path")
    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    users, items = frame()
    by_item = np.argsort(items, kind="stable")
    cuts = np.searchsorted(items[by_item], np.arange(I + 1))
    lists = {i: users[by_item[cuts[i]:cuts[i + 1]]].tolist() for i in range(I)}
    lens = np.diff(cuts)
    max_neighbors = int(lens.max())
    rng = np.random.default_rng(1)
    n = args.steps * B
    pick = np.repeat(rng.permutation(len(users))[:n // NEG], NEG)
    tu, tp, tn = users[pick], items[pick], rng.integers(0, I, n)

    def padded(item_ids):
        nbr = np.zeros((len(item_ids), max_neighbors), dtype=np.int64)
        for r, i in enumerate(item_ids):
            nbr[r, :lens[i]] = lists[i]
        return nbr

    cols = [torch.from_numpy(a).to(dev) for a in (tu, tp, tn)]
    batches = []
    for off in range(0, n, B):
        sl = slice(off, off + B)
        batches.append(tuple(torch.from_numpy(a).to(dev) for a in (tu[sl], tp[sl], tn[sl], padded(tp[sl]), lens[tp[sl]],
                                                                   padded(tn[sl]), lens[tn[sl]]))
                       + (int(lens[tp[sl]].max()), int(lens[tn[sl]].max())))
    list_total = [int(lens[tp[o:o + B]].sum() + lens[tn[o:o + B]].sum()) for o in range(0, n, B)]
    list_longest = [max(b[7], b[8]) for b in batches]

    torch.manual_seed(0)
    ref = TorchCMN(max_neighbors)
    with torch.no_grad():
        for emb in (ref.user_memory, ref.item_memory, ref.user_output):
            emb.weight.mul_(0.01)
    w0 = {"user_memory.weight": ref.user_memory.weight, "item_memory.weight": ref.item_memory.weight,
          "user_output.weight": ref.user_output.weight, "mem_layer.hop_mapping.1.weight": ref.hop.weight,
          "mem_layer.hop_mapping.1.bias": ref.hop.bias, "dense.weight": ref.dense.weight, "dense.bias": ref.dense.bias,
          "out.weight": ref.out.weight}
    w0 = {k: v.detach().clone() for k, v in w0.items()}
    ref.to(dev)
    opt = torch.optim.Adam(ref.parameters(), lr=LR)
    cfg = {"emb_dim": D, "device_str": "cuda:0", "regs": [1e-5], "batch_size": B, "lr": LR, "momentum": 0.9,
           "training_l2_lambda": LAM, "grad_clip": CLIP, "neg_count": NEG,
           "model": {"optimizer": "adam", "lr": LR, "device_str": "cuda:0"}, "system": {"run_dir": "/tmp/hiprec_bench_runs"}}
    engines = {}
    for side in ("hip_csr", "hip_padded"):
        with contextlib.redirect_stdout(io.StringIO()):
            engines[side] = hp.cmnEngine(dict(cfg), w0["user_memory.weight"].numpy(), w0["item_memory.weight"].numpy(), lists)
        engines[side].model.load_state_dict(w0)

    def hip_csr():
        engines["hip_csr"].enqueue_epoch(*cols)

    def hip_padded():
        for b in batches:
            engines["hip_padded"]._enqueue_step(b[:7])

    def torch_steps():
        for b in batches:
            opt.zero_grad()
            pos_s, neg_s = ref(*b)
            loss = torch.mean(-1 * torch.log(torch.sigmoid(pos_s - neg_s) + 1e-12))
            loss = loss + LAM * torch.sqrt(ref.hop.weight.pow(2).sum())
            loss.backward()
            torch.nn.utils.clip_grad_norm_(ref.parameters(), CLIP)
            opt.step()

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.windows):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (args.windows * len(batches)) * 1e6   # us per step

    sides = {"hip_csr": hip_csr, "hip_padded": hip_padded}
    if not args.hip_only:
        sides["torch"] = torch_steps
    for fn in sides.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in sides}
    for _ in range(args.repeats):
        for k, fn in sides.items():
            times[k].append(window(fn))
    st = engines["hip_csr"]._sync_stats()
    engines["hip_padded"]._sync_stats()
    atomic = [t * D * 4 * 2 + 2 * 2 * B * D * 4 for t in list_total]
    out = {"tool": "tools/bench_cmn.py", "device": torch.cuda.get_device_name(0),
           "source_hash": __graft_entry__.source_hash(), "n_users": U, "n_items": I, "emb_dim": D, "batch": B,
           "neg_count": NEG, "optimizer": "adam", "interactions": int(len(users)), "max_neighbors": max_neighbors,
           "steps_per_window": args.windows * len(batches), "repeats": args.repeats,
           "list_slots_per_step_mean": float(np.mean(list_total)), "list_slots_per_step_max": int(max(list_total)),
           "longest_list_in_a_batch": int(max(list_longest)),
           "atomic_bytes_per_step_mean": float(np.mean(atomic)),
           "atomic_floor_us": round(float(np.mean(atomic)) / ATOMIC_RATE * 1e6, 2),
           "last_loss_hip": st.loss}
    for k, v in times.items():
        med = float(np.median(v))
        out[f"{k}_us_per_step"] = [round(x, 2) for x in v]
        out[f"{k}_us_per_step_median"] = round(med, 2)
        out[f"{k}_spread"] = round((max(v) - min(v)) / med, 4)
    if "torch" in times:
        for k in ("hip_csr", "hip_padded"):
            out[f"{k}_speedup_vs_torch_ops"] = round(out["torch_us_per_step_median"] / out[f"{k}_us_per_step_median"], 2)
            out[f"{k}_not_slower_than_torch"] = bool(out[f"{k}_us_per_step_median"] <= 1.05 * out["torch_us_per_step_median"])
    print(json.dumps(out), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
