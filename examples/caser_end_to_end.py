"""Caser end to end on a synthetic log: sequences -> ``data.WindowSampler`` -> epochs of ``CaserEngine.train_an_epoch``
-> ``recommend_next`` -> hit-rate@10 on each user's held-out last item.

    python examples/caser_end_to_end.py                      # 943 users, 1682 items, L 5, T 3, 30 epochs
    python examples/caser_end_to_end.py --users 192 --items 60 --group 10 --epochs 30

The log has sequential structure: the catalogue is cut into groups of ``--group`` items, a user stays inside one group
and walks its ring -- the next item is one to three places further four times out of five, any item of the group
otherwise (one time in twenty any item at all).  The last ``L`` items therefore tell the next one, which is what the
horizontal filters pick up; the user embedding learns the group.

Prints one JSON line with the mean loss per epoch, the hit rate, the ``top / n_items`` of a random ranking and
``margin``: four binomial standard deviations of that chance rate at this number of users -- a hit rate above
``random_hit_rate + margin`` is not luck.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def synthetic_log(n_users, n_items, group, min_len, max_len, seed):
    """user -> list of item ids in 1 .. n_items (time order)."""
    rng = np.random.default_rng(seed)
    n_groups = max(1, n_items // group)
    out = {}
    for u in range(n_users):
        g = int(rng.integers(0, n_groups))
        lo = g * group                                   # the group's items are lo + 1 .. lo + group
        n = int(rng.integers(min_len, max_len + 1))
        at = int(rng.integers(0, group))
        items = [lo + at + 1]
        while len(items) < n:
            r = rng.random()
            if r < 0.8:
                at = (at + int(rng.integers(1, 4))) % group
                items.append(lo + at + 1)
            elif r < 0.95:
                at = int(rng.integers(0, group))
                items.append(lo + at + 1)
            else:
                items.append(int(rng.integers(1, n_items + 1)))
        out[u] = items
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--users", type=int, default=943)
    ap.add_argument("--items", type=int, default=1682)
    ap.add_argument("--group", type=int, default=29)
    ap.add_argument("--L", type=int, default=5)
    ap.add_argument("--T", type=int, default=3)
    ap.add_argument("--neg-samples", type=int, default=3)
    ap.add_argument("--emb-dim", type=int, default=50)
    ap.add_argument("--n-v", type=int, default=4)
    ap.add_argument("--n-h", type=int, default=16)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--l2", type=float, default=1e-6)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--epochs", type=int, default=30)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    import torch

    import beta_recsys_amd as hp
    from beta_recsys_amd.data import WindowSampler, last_window

    torch.manual_seed(args.seed)
    log = synthetic_log(args.users, args.items, args.group, args.L + args.T + 2, 60, args.seed)
    train = {u: items[:-1] for u, items in log.items()}          # the last item of every user is held out
    target = np.array([log[u][-1] for u in range(args.users)])
    cfg = {"model": {"n_users": args.users, "n_items": args.items, "emb_dim": args.emb_dim, "L": args.L, "T": args.T,
                     "neg_samples": args.neg_samples, "n_v": args.n_v, "n_h": args.n_h, "ac_conv": "relu",
                     "ac_fc": "relu", "dropout_rate": args.dropout, "l2": args.l2, "lr": args.lr, "optimizer": "adam",
                     "batch_size": args.batch_size, "device_str": "cuda:0", "dropout_rng": "device",
                     "dropout_seed": args.seed},
           "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.CaserEngine(cfg)
    sampler = WindowSampler(train, args.users, args.items, args.batch_size, args.L, args.T, args.neg_samples,
                            seed=args.seed)
    losses = []
    for epoch in range(args.epochs):
        with contextlib.redirect_stdout(io.StringIO()):
            losses.append(float(eng.train_an_epoch(sampler, epoch)))
    sampler.close()

    # the last L items of every user's training history.  Nothing is excluded: the walk revisits items, so the held-out
    # one has usually been seen
    users, queries = last_window(train, args.L)
    top, _ = eng.recommend_next(queries, users, args.top)
    top = top.cpu().numpy()
    hit = float((top == target[users][:, None]).any(axis=1).mean())
    chance = args.top / args.items
    margin = 4.0 * float(np.sqrt(chance * (1.0 - chance) / args.users))
    result = {"example": "caser_end_to_end", "users": args.users, "items": args.items, "L": args.L, "T": args.T,
              "epochs": args.epochs, "steps_per_epoch": len(sampler), "mean_loss_per_epoch": losses,
              f"hit_rate@{args.top}": hit, "random_hit_rate": chance, "margin": margin}
    print(json.dumps(result))
    return result, top


if __name__ == "__main__":
    main()
