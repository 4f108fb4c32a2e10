"""SR-GNN end to end on synthetic sessions with revisits: sessions -> ``data.session_prefixes`` -> a shuffled
``data.SessionLoader`` -> epochs of ``SRGNNEngine.train_an_epoch`` -> ``recommend_next`` -> hit-rate@10 on each session's
held-out last event.

    python examples/srgnn_end_to_end.py                        # 2000 sessions, 2000 items, H 100, 6 epochs
    python examples/srgnn_end_to_end.py --sessions 384 --items 60 --group 10 --hidden 32 --epochs 8

The sessions have a planted transition structure: the catalogue (ids 1 .. items) is cut into groups of ``--group`` items,
a session stays inside one group and walks its ring -- the next item is one to three places further four times out of
five, any item of the group otherwise (one time in twenty any item at all).  A walk over a ring of ``--group`` items
revisits them, so the session graphs have cycles, self-loops and repeated transitions.

Prints one JSON line with the mean loss per epoch, the hit rate, the ``top / items`` of a random ranking and ``margin``:
four binomial standard deviations of that chance rate at this number of sessions -- a hit rate above
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


def synthetic_sessions(n_sessions, n_items, group, min_len, max_len, seed):
    """A list of id lists, ids in 1 .. n_items (time order)."""
    rng = np.random.default_rng(seed)
    n_groups = max(1, n_items // group)
    out = []
    for _ in range(n_sessions):
        lo = int(rng.integers(0, n_groups)) * group
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
                items.append(int(rng.integers(0, n_items)) + 1)
        out.append(items)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sessions", type=int, default=2000)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--step", type=int, default=1)
    ap.add_argument("--nonhybrid", action="store_true")
    ap.add_argument("--batch-size", type=int, default=100)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--l2", type=float, default=1e-5)
    ap.add_argument("--lr-dc-step", type=int, default=3)
    ap.add_argument("--lr-dc", type=float, default=0.1)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    import torch

    import beta_recsys_amd as hp
    from beta_recsys_amd.data import SessionLoader, session_prefixes

    torch.manual_seed(args.seed)
    sessions = synthetic_sessions(args.sessions, args.items, args.group, 4, 14, args.seed)
    train = [s[:-1] for s in sessions]                       # the last event of every session is held out
    target = np.array([s[-1] for s in sessions])
    out_seqs, labels = session_prefixes(train)
    cfg = {"model": {"hidden_size": args.hidden, "step": args.step, "nonhybrid": args.nonhybrid,
                     "batch_size": args.batch_size, "lr": args.lr, "l2": args.l2, "lr_dc_step": args.lr_dc_step,
                     "lr_dc": args.lr_dc, "optimizer": "adam", "device_str": "cuda:0"},
           "dataset": {"n_node": args.items + 1}, "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.SRGNNEngine(cfg)
    loader = SessionLoader(out_seqs, labels, args.batch_size, shuffle=True, seed=args.seed)
    losses = []
    for epoch in range(args.epochs):
        with contextlib.redirect_stdout(io.StringIO()):
            losses.append(float(eng.train_an_epoch(loader, epoch)))

    # nothing is excluded: the walk revisits items, so the held-out one has usually been seen
    top, _ = eng.recommend_next(train, args.top)
    top = top.cpu().numpy()
    hit = float((top == target[:, None]).any(axis=1).mean())
    chance = args.top / args.items
    margin = 4.0 * float(np.sqrt(chance * (1.0 - chance) / args.sessions))
    result = {"example": "srgnn_end_to_end", "sessions": args.sessions, "items": args.items, "hidden": args.hidden,
              "step": args.step, "epochs": args.epochs, "steps_per_epoch": len(loader), "mean_loss_per_epoch": losses,
              f"hit_rate@{args.top}": hit, "random_hit_rate": chance, "margin": margin}
    print(json.dumps(result))
    return result, top


if __name__ == "__main__":
    main()
