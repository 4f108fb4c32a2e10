"""TiSASRec end to end on a synthetic timestamped ML-100K-shaped log: ``[item, time]`` sequences ->
``data.TimeSequenceSampler`` -> epochs of ``TiSASRecEngine.train_an_epoch`` -> ``recommend_next`` -> hit-rate@10 on each
user's held-out last item.

    python examples/tisasrec_end_to_end.py                     # 943 users, 1682 items, maxlen 50, 60 epochs of 7 steps
    python examples/tisasrec_end_to_end.py --users 200 --items 300 --epochs 3

The log is the noisy walk of ``examples/sasrec_end_to_end.py`` with a clock: a user's next item is the previous one plus a
small step four times out of five, and then it follows after a short interval; a uniformly random item follows after a
long one, so the interval says how much the last item tells.  The sampler's batches carry no prebuilt relation table: the
``[B, T, T]`` matrix is ``min(|t_i - t_j|, time_span)`` of each batch's time stamps.  Prints one JSON line with the mean
loss per epoch, the hit rate and the 10 / n_items of a random ranking next to it; the default number of steps brings the
training loss down but is far too small for the held-out hit rate to leave that floor: raise --epochs for a ranking that
means something.
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


def synthetic_log(n_users, n_items, min_len, max_len, time_span, seed):
    """user -> list of [item id in 1 .. n_items, integer time stamp] (time order)."""
    rng = np.random.default_rng(seed)
    out = {}
    for u in range(n_users):
        n = int(rng.integers(min_len, max_len + 1))
        events = [[int(rng.integers(1, n_items + 1)), 1]]
        while len(events) < n:
            item, now = events[-1]
            if rng.random() < 0.8:
                events.append([(item - 1 + int(rng.integers(1, 4))) % n_items + 1, now + int(rng.integers(0, 3))])
            else:
                events.append([int(rng.integers(1, n_items + 1)), now + int(rng.integers(time_span // 2, time_span))])
        out[u] = events
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--users", type=int, default=943)
    ap.add_argument("--items", type=int, default=1682)
    ap.add_argument("--maxlen", type=int, default=50)
    ap.add_argument("--time-span", type=int, default=32)
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=2)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    import torch

    import beta_recsys_amd as hp
    from beta_recsys_amd.data import TimeSequenceSampler, time_relation

    torch.manual_seed(args.seed)
    log = synthetic_log(args.users, args.items, 12, 2 * args.maxlen, args.time_span, args.seed)
    train = {u: events[:-1] for u, events in log.items()}        # the last event of every user is held out
    target = np.array([log[u][-1][0] for u in range(args.users)])
    cfg = {"model": {"n_users": args.users, "n_items": args.items, "emb_dim": args.emb_dim, "maxlen": args.maxlen,
                     "time_span": args.time_span,
                     "num_blocks": args.blocks, "num_heads": args.heads, "dropout_rate": args.dropout,
                     "batch_size": args.batch_size, "l2_emb": 0.0, "optimizer": "adam", "lr": args.lr,
                     "device_str": "cuda:0", "dropout_rng": "device", "dropout_seed": args.seed},
           "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.TiSASRecEngine(cfg)
    sampler = TimeSequenceSampler(train, args.users, args.items, args.batch_size, args.maxlen, args.time_span,
                                  seed=args.seed)
    losses = []
    for epoch in range(args.epochs):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            eng.train_an_epoch(sampler, epoch)
        losses.append(float(out.getvalue().strip().rsplit("Loss ", 1)[1]) / max(eng.num_batch, 1))
    sampler.close()

    # every user's last maxlen training items, left-padded, then the k best unseen next items
    eng.model.eval()
    seqs, times = (np.zeros((args.users, args.maxlen), dtype=np.int64) for _ in range(2))
    rows, seen = [], []
    for u in range(args.users):
        events = train[u][-args.maxlen:]
        seqs[u, args.maxlen - len(events):] = [e[0] for e in events]
        times[u, args.maxlen - len(events):] = [e[1] for e in events]
        past = sorted({e[0] for e in train[u]} - {int(target[u])})          # a repeated target stays recommendable
        rows += [u] * len(past)
        seen += past
    rows, seen = np.array(rows), np.array(seen)
    top = np.zeros((args.users, args.top), dtype=np.int64)
    for lo in range(0, args.users, args.batch_size):           # the matrices of a slice of users at a time
        hi = min(args.users, lo + args.batch_size)
        mine = (rows >= lo) & (rows < hi)
        part, _ = eng.recommend_next(seqs[lo:hi], time_relation(times[lo:hi], args.time_span), args.top,
                                     seen=(rows[mine] - lo, seen[mine]))
        top[lo:hi] = part.cpu().numpy()
    hit = float((top == target[:, None]).any(axis=1).mean())
    result = {"example": "tisasrec_end_to_end", "users": args.users, "items": args.items, "maxlen": args.maxlen,
              "time_span": args.time_span, "epochs": args.epochs, "steps_per_epoch": eng.num_batch, "mean_loss_per_epoch": losses,
              f"hit_rate@{args.top}": hit, "random_hit_rate": args.top / args.items}
    print(json.dumps(result))
    return result, top


if __name__ == "__main__":
    main()
