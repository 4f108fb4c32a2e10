"""ETA end to end on synthetic users whose telling items lie further back than DIN can see: ``CandidateLoader`` -> epochs of
``ETAEngine.train_an_epoch`` -> ``rerank`` of each user's held-out item among 99 sampled negatives -> hit-rate@10 next to chance
and its 4-sigma margin, and the share of the retrieved positions that fall in the burst before and after training.

    python examples/eta_end_to_end.py                      # 512 users, 1000 items, histories of 1024
    python examples/eta_end_to_end.py --users 192 --items 400 --clusters 16 --group 8 --maxlen 288 --emb-dim 16

The first ``--clusters x --group`` items fall into clusters, the rest are background.  A history is background noise but
for a burst of ``--burst`` events from the user's own cluster that starts at position ``--burst-at``: more than 256 positions
before the end, so a model that reads the last 256 events (DIN, DIEN) sees noise only.  The held-out item belongs to the
cluster and is in neither the user's burst nor their training targets; other users of the cluster carry it.

Prints one JSON line with the mean loss per epoch, the hit rate, the ``top / (1 + negatives)`` of a random order, ``margin``
(four binomial standard deviations of that chance rate at this number of users) and ``burst_share_before`` / ``_after``: of
the positions the held-out item retrieves, the share inside the burst (``burst / maxlen`` for a random selection).
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def burst_users(n_users, n_items, clusters, group, maxlen, burst_at, burst, seed):
    """``(histories [n_users, maxlen], held_out [n_users], train targets: a list per user)``."""
    rng = np.random.default_rng(seed)
    first_bg = clusters * group + 1
    seq = rng.integers(first_bg, n_items + 1, (n_users, maxlen))
    held, targets = np.zeros(n_users, dtype=np.int64), []
    for u in range(n_users):
        own = 1 + (u % clusters) * group + np.arange(group)
        held[u] = rng.choice(own)
        rest = own[own != held[u]]
        seq[u, burst_at:burst_at + burst] = rng.choice(rest, burst)
        targets.append(rest.tolist())
    return seq, held, targets


def burst_share(model, seq, items, lo, hi):
    """Of the positions ``items`` retrieve from their histories, the share in ``[lo, hi)``."""
    import torch

    E = model.item_emb.weight.data
    seq_t, item_t = torch.as_tensor(seq, device=E.device), torch.as_tensor(items, device=E.device)
    sel = model.retrieve_stage(E[seq_t], E[item_t][:, None, :], seq_t != 0)[2]
    return float(((sel >= lo) & (sel < hi)).sum()) / max(int((sel >= 0).sum()), 1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--items", type=int, default=1000)
    ap.add_argument("--clusters", type=int, default=32)
    ap.add_argument("--group", type=int, default=10)
    ap.add_argument("--maxlen", type=int, default=1024)
    ap.add_argument("--burst-at", type=int, default=8)
    ap.add_argument("--burst", type=int, default=24)
    ap.add_argument("--top-k", type=int, default=16)
    ap.add_argument("--hash-bits", type=int, default=64)
    ap.add_argument("--num-heads", type=int, default=2)
    ap.add_argument("--emb-dim", type=int, default=32)
    ap.add_argument("--n-neg", type=int, default=4)
    ap.add_argument("--negatives", type=int, default=99)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-2)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    if args.maxlen - (args.burst_at + args.burst) < 256:
        raise SystemExit("the burst must end more than 256 positions before the end of the history")

    import torch

    import beta_recsys_amd as hp
    import beta_recsys_amd.data      # noqa: F401

    seq, held, targets = burst_users(args.users, args.items, args.clusters, args.group, args.maxlen, args.burst_at, args.burst,
                                     args.seed)
    out_seqs = [seq[u] for u in range(args.users) for _ in targets[u]]
    labels = [t for u in range(args.users) for t in targets[u]]

    torch.manual_seed(args.seed)
    cfg = {"model": {"n_items": args.items, "emb_dim": args.emb_dim, "maxlen": args.maxlen, "lr": args.lr, "optimizer": "adam",
                     "batch_size": args.batch_size, "device_str": "cuda:0", "top_k": args.top_k, "hash_bits": args.hash_bits,
                     "num_heads": args.num_heads, "hash_seed": args.seed},
           "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    loader = hp.data.CandidateLoader(out_seqs, labels, args.batch_size, args.maxlen, args.items, args.n_neg, shuffle=True,
                                     seed=args.seed)
    lo, hi = args.burst_at, args.burst_at + args.burst
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.ETAEngine(cfg)
        before = burst_share(eng.model, seq, held, lo, hi)
        losses = [float(eng.train_an_epoch(loader, e)) for e in range(args.epochs)]
    after = burst_share(eng.model, seq, held, lo, hi)
    held_out = hp.data.CandidateLoader([], [], 1, args.maxlen, args.items, args.negatives, seed=args.seed + 1)
    top, _ = eng.rerank(seq, held_out.candidates(held), args.top)
    hit = float((top.cpu().numpy() == held[:, None]).any(axis=1).mean())
    chance = args.top / (1 + args.negatives)
    margin = 4.0 * float(np.sqrt(chance * (1.0 - chance) / args.users))
    result = {"example": "eta_end_to_end", "users": args.users, "items": args.items, "maxlen": args.maxlen,
              "burst": [lo, hi], "epochs": args.epochs, "steps_per_epoch": len(loader), "loss_per_epoch": losses,
              f"hit_rate@{args.top}": hit, "random_hit_rate": chance, "margin": margin, "burst_share_before": before,
              "burst_share_after": after, "burst_share_random": args.burst / args.maxlen}
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
