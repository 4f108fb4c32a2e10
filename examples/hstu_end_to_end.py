"""HSTU end to end on a timestamped synthetic log: ``data.TimeSequenceSampler`` -> epochs of
``HSTUEngine.train_an_epoch`` -> ``recommend_next`` -> hit-rate@10 on each user's held-out last item.

    python examples/hstu_end_to_end.py                      # 943 users, 1682 items, maxlen 50, 20 epochs
    python examples/hstu_end_to_end.py --users 192 --items 60 --group 10 --emb-dim 16 --maxlen 12 --num-blocks 1

The log is ``nextitnet_end_to_end.synthetic_log``'s: a user walks the ring of one group of items, so the last items tell
the next one.  Every event carries an integer time stamp: bursts of seconds apart inside a session, hours between sessions.

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


def stamped(log, seed):
    """user -> list of ``[item, time]``: gaps of 1 .. 60 s inside a session, of hours between sessions."""
    rng = np.random.default_rng(seed + 1)
    out = {}
    for u, items in log.items():
        gaps = np.where(rng.random(len(items)) < 0.2, rng.integers(3600, 200000, len(items)), rng.integers(1, 61, len(items)))
        times = 1_600_000_000 + np.cumsum(gaps)
        out[u] = [[int(i), int(t)] for i, t in zip(items, times)]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--users", type=int, default=943)
    ap.add_argument("--items", type=int, default=1682)
    ap.add_argument("--group", type=int, default=29)
    ap.add_argument("--maxlen", type=int, default=50)
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--num-heads", type=int, default=2)
    ap.add_argument("--attention-dim", type=int, default=32)
    ap.add_argument("--linear-dim", type=int, default=32)
    ap.add_argument("--num-blocks", type=int, default=2)
    ap.add_argument("--rel-bias", default="pos_time", choices=("pos_time", "pos"))
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    import torch

    import beta_recsys_amd as hp
    from beta_recsys_amd.data import SequenceSampler, TimeSequenceSampler

    torch.manual_seed(args.seed)
    log = stamped(synthetic_log(args.users, args.items, args.group, 6, args.maxlen + 10, args.seed), args.seed)
    train = {u: pairs[:-1] for u, pairs in log.items()}          # the last event of every user is held out
    target = np.array([log[u][-1][0] for u in range(args.users)])
    timed = args.rel_bias == "pos_time"
    cfg = {"model": {"n_users": args.users, "n_items": args.items, "emb_dim": args.emb_dim, "maxlen": args.maxlen,
                     "num_blocks": args.num_blocks, "num_heads": args.num_heads, "attention_dim": args.attention_dim,
                     "linear_dim": args.linear_dim, "rel_bias": args.rel_bias, "dropout_rate": args.dropout,
                     "dropout_seed": args.seed, "lr": args.lr, "optimizer": "adam", "batch_size": args.batch_size,
                     "device_str": "cuda:0"},
           "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    if timed:
        sampler = TimeSequenceSampler(train, args.users, args.items, args.batch_size, args.maxlen, 1, args.seed)
    else:
        sampler = SequenceSampler({u: [p[0] for p in pairs] for u, pairs in train.items()}, args.users, args.items,
                                  args.batch_size, args.maxlen, args.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.HSTUEngine(cfg)
        losses = [float(eng.train_an_epoch(sampler, e)) for e in range(args.epochs)]

    # the last maxlen events of every user's training history, left-padded
    queries, stamps = (np.zeros((args.users, args.maxlen), dtype=np.int64) for _ in range(2))
    for u in range(args.users):
        tail = train[u][-args.maxlen:]
        queries[u, args.maxlen - len(tail):] = [p[0] for p in tail]
        stamps[u, args.maxlen - len(tail):] = [p[1] for p in tail]
    top, _ = eng.recommend_next(queries, args.top, time_seq=stamps if timed else None)
    top = top.cpu().numpy()
    hit = float((top == target[:, None]).any(axis=1).mean())
    chance = args.top / args.items
    margin = 4.0 * float(np.sqrt(chance * (1.0 - chance) / args.users))
    result = {"example": "hstu_end_to_end", "users": args.users, "items": args.items, "maxlen": args.maxlen,
              "rel_bias": args.rel_bias, "epochs": args.epochs, "steps_per_epoch": eng.num_batch, "loss_per_epoch": losses,
              f"hit_rate@{args.top}": hit, "random_hit_rate": chance, "margin": margin}
    print(json.dumps(result))
    return result, top


if __name__ == "__main__":
    main()
