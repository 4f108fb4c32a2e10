"""DIEN end to end on synthetic users whose interest drifts: ``session_prefixes`` -> ``EvolutionLoader`` -> epochs of
``DIENEngine.train_an_epoch`` -> ``rerank`` of each user's held-out last item among 99 sampled negatives -> hit-rate@10 next to
chance and its 4-sigma margin.

    python examples/dien_end_to_end.py                      # 512 users, 600 items
    python examples/dien_end_to_end.py --users 96 --items 200 --group 10 --emb-dim 16 --maxlen 8

The items fall into clusters of ``--group``; a user walks through ``--clusters`` of them one after the other, every event a
random item of the cluster of its phase, so the held-out item belongs to the LAST cluster of the history and not to the
earlier ones: the order of the history matters, a bag of it does not tell which cluster comes next.

Prints one JSON line with the mean loss per epoch, the hit rate, the ``top / (1 + negatives)`` of a random order and
``margin``: four binomial standard deviations of that chance rate at this number of users.
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


def drifting_users(n_users, n_items, group, clusters, length, seed):
    """Per user a list of ``length`` items in ``1 .. n_items``: ``clusters`` distinct clusters of ``group`` items in a random
    order, each held for an equal share of the events."""
    rng = np.random.default_rng(seed)
    log = []
    for _ in range(n_users):
        own = rng.choice(n_items // group, clusters, replace=False)
        phase = np.minimum(np.arange(length) * clusters // length, clusters - 1)
        log.append((1 + own[phase] * group + rng.integers(0, group, length)).tolist())
    return log


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--items", type=int, default=600)
    ap.add_argument("--group", type=int, default=20)
    ap.add_argument("--clusters", type=int, default=2)
    ap.add_argument("--length", type=int, default=24)
    ap.add_argument("--maxlen", type=int, default=20)
    ap.add_argument("--emb-dim", type=int, default=32)
    ap.add_argument("--n-neg", type=int, default=4)
    ap.add_argument("--negatives", type=int, default=99)
    ap.add_argument("--batch-size", type=int, default=128)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    import torch

    import beta_recsys_amd as hp
    import beta_recsys_amd.data      # noqa: F401

    log = drifting_users(args.users, args.items, args.group, args.clusters, args.length, args.seed)
    train = [log[u][:-1] for u in range(args.users)]          # the last item of every user is held out
    target = np.array([log[u][-1] for u in range(args.users)])
    out_seqs, labels = hp.data.session_prefixes(train)
    queries = np.zeros((args.users, args.maxlen), dtype=np.int64)
    for u, items in enumerate(train):
        tail = items[-args.maxlen:]
        queries[u, args.maxlen - len(tail):] = tail

    torch.manual_seed(args.seed)
    cfg = {"model": {"n_items": args.items, "emb_dim": args.emb_dim, "maxlen": args.maxlen, "lr": args.lr, "optimizer": "adam",
                     "batch_size": args.batch_size, "device_str": "cuda:0"},
           "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    loader = hp.data.EvolutionLoader(out_seqs, labels, args.batch_size, args.maxlen, args.items, args.n_neg, shuffle=True,
                                     seed=args.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.DIENEngine(cfg)
        losses = [float(eng.train_an_epoch(loader, e)) for e in range(args.epochs)]
    held_out = hp.data.CandidateLoader([], [], 1, args.maxlen, args.items, args.negatives, seed=args.seed + 1)
    top, _ = eng.rerank(queries, held_out.candidates(target), args.top)
    hit = float((top.cpu().numpy() == target[:, None]).any(axis=1).mean())
    chance = args.top / (1 + args.negatives)
    margin = 4.0 * float(np.sqrt(chance * (1.0 - chance) / args.users))
    result = {"example": "dien_end_to_end", "users": args.users, "items": args.items, "maxlen": args.maxlen,
              "epochs": args.epochs, "steps_per_epoch": len(loader), "loss_per_epoch": losses, f"hit_rate@{args.top}": hit,
              "random_hit_rate": chance, "margin": margin}
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
