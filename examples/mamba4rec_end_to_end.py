"""Mamba4Rec end to end on a synthetic log: prefix sampling -> epochs of ``Mamba4RecEngine.train_single_batch`` ->
``recommend_next`` -> hit-rate@10 on each user's held-out last item.

    python examples/mamba4rec_end_to_end.py                      # 943 users, 1682 items, maxlen 50, 20 epochs
    python examples/mamba4rec_end_to_end.py --users 192 --items 60 --group 10 --emb-dim 16 --maxlen 12 --num-blocks 1

The log is ``nextitnet_end_to_end.synthetic_log``'s: a user walks the ring of one group of items, so the last items tell
the next one.  A training row is a random prefix of a user's history (the published code trains on every prefix), its next
item as ``pos`` and a random item the user never took as ``neg``.

Prints one JSON line with the summed loss per epoch, the hit rate, the ``top / n_items`` of a random ranking and ``margin``:
four binomial standard deviations of that chance rate at this number of users.
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

from nextitnet_end_to_end import synthetic_log      # noqa: E402


def prefix_batch(train, users, n_items, maxlen, rng):
    """``(u, seq [B, maxlen], pos [B], neg [B])``: for every user a cut 1 <= c < len, the items before it, the item at it."""
    seq = np.zeros((len(users), maxlen), dtype=np.int64)
    pos, neg = np.zeros(len(users), dtype=np.int64), np.zeros(len(users), dtype=np.int64)
    for r, u in enumerate(users):
        items = train[u]
        c = int(rng.integers(1, len(items)))
        tail = items[max(0, c - maxlen):c]
        seq[r, maxlen - len(tail):] = tail
        pos[r] = items[c]
        neg[r] = rng.integers(1, n_items + 1)
        while neg[r] in items:
            neg[r] = rng.integers(1, n_items + 1)
    return users, seq, pos, neg


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--users", type=int, default=943)
    ap.add_argument("--items", type=int, default=1682)
    ap.add_argument("--group", type=int, default=29)
    ap.add_argument("--maxlen", type=int, default=50)
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--num-blocks", type=int, default=2)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    import torch

    import beta_recsys_amd as hp

    torch.manual_seed(args.seed)
    rng = np.random.default_rng(args.seed)
    log = synthetic_log(args.users, args.items, args.group, 6, args.maxlen + 10, args.seed)
    train = {u: items[:-1] for u, items in log.items()}          # the last item of every user is held out
    target = np.array([log[u][-1] for u in range(args.users)])
    cfg = {"model": {"n_users": args.users, "n_items": args.items, "emb_dim": args.emb_dim, "maxlen": args.maxlen,
                     "num_blocks": args.num_blocks, "dropout_rate": args.dropout, "dropout_seed": args.seed, "lr": args.lr,
                     "optimizer": "adam", "batch_size": args.batch_size, "device_str": "cuda:0"},
           "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.Mamba4RecEngine(cfg)
    losses = []
    for _ in range(args.epochs):
        order = rng.permutation(args.users)
        total = 0.0
        for k in range(eng.num_batch):
            users = order[k * args.batch_size:(k + 1) * args.batch_size]
            total += eng.train_single_batch(prefix_batch(train, users, args.items, args.maxlen, rng))
        losses.append(float(total))

    # the last maxlen items of every user's training history; shorter ones are left-padded by the model
    queries = np.zeros((args.users, args.maxlen), dtype=np.int64)
    for u in range(args.users):
        tail = train[u][-args.maxlen:]
        queries[u, args.maxlen - len(tail):] = tail
    top, _ = eng.recommend_next(queries, args.top)
    top = top.cpu().numpy()
    hit = float((top == target[:, None]).any(axis=1).mean())
    chance = args.top / args.items
    margin = 4.0 * float(np.sqrt(chance * (1.0 - chance) / args.users))
    result = {"example": "mamba4rec_end_to_end", "users": args.users, "items": args.items, "maxlen": args.maxlen,
              "epochs": args.epochs, "steps_per_epoch": eng.num_batch, "loss_per_epoch": losses,
              f"hit_rate@{args.top}": hit, "random_hit_rate": chance, "margin": margin}
    print(json.dumps(result))
    return result, top


if __name__ == "__main__":
    main()
