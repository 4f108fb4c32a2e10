"""BERT4Rec end to end on a synthetic log: sequences -> ``data.ClozeSampler`` -> epochs of
``BERT4RecEngine.train_an_epoch`` -> ``recommend_next`` -> hit-rate@10 on each user's held-out last item.

    python examples/bert4rec_end_to_end.py                      # 943 users, 1682 items, maxlen 50, 60 epochs of 7 steps
    python examples/bert4rec_end_to_end.py --users 192 --items 60 --group 10 --maxlen 12 --epochs 60

The log has structure on both sides of every position: the catalogue is cut into groups of ``--group`` items, a user
stays inside one group, and walks its ring -- the next item is one to three places further four times out of five,
any item of the group otherwise (one time in twenty any item at all).  A masked item is therefore told by its left AND
its right neighbours, which is what the cloze task trains; the held-out last item is the case with a left context only,
which the sampler's forced last-position mask covers.

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
    ap.add_argument("--maxlen", type=int, default=50)
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--mask-prob", type=float, default=0.2)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    import torch

    import beta_recsys_amd as hp
    from beta_recsys_amd.data import ClozeSampler

    torch.manual_seed(args.seed)
    log = synthetic_log(args.users, args.items, args.group, 6, 2 * args.maxlen, args.seed)
    train = {u: items[:-1] for u, items in log.items()}          # the last item of every user is held out
    target = np.array([log[u][-1] for u in range(args.users)])
    cfg = {"model": {"n_users": args.users, "n_items": args.items, "emb_dim": args.emb_dim, "maxlen": args.maxlen,
                     "num_blocks": args.blocks, "num_heads": args.heads, "dropout_rate": args.dropout,
                     "batch_size": args.batch_size, "mask_prob": args.mask_prob, "optimizer": "adam", "lr": args.lr,
                     "device_str": "cuda:0", "dropout_rng": "device", "dropout_seed": args.seed},
           "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.BERT4RecEngine(cfg)
    sampler = ClozeSampler(train, args.users, args.items, args.batch_size, args.maxlen, mask_prob=args.mask_prob,
                           seed=args.seed)
    losses = []
    for epoch in range(args.epochs):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            eng.train_an_epoch(sampler, epoch)
        losses.append(float(out.getvalue().strip().rsplit("Loss ", 1)[1]) / max(eng.num_batch, 1))
    sampler.close()

    # every user's training history; recommend_next cuts it to maxlen - 1 and appends [MASK].  Nothing is excluded:
    # the walk revisits items, so the held-out one has usually been seen
    eng.model.eval()
    top, _ = eng.recommend_next([train[u] for u in range(args.users)], args.top)
    top = top.cpu().numpy()
    hit = float((top == target[:, None]).any(axis=1).mean())
    chance = args.top / args.items
    margin = 4.0 * float(np.sqrt(chance * (1.0 - chance) / args.users))
    result = {"example": "bert4rec_end_to_end", "users": args.users, "items": args.items, "maxlen": args.maxlen,
              "epochs": args.epochs, "steps_per_epoch": eng.num_batch, "mean_loss_per_epoch": losses,
              f"hit_rate@{args.top}": hit, "random_hit_rate": chance, "margin": margin}
    print(json.dumps(result))
    return result, top


if __name__ == "__main__":
    main()
