"""GRU4Rec end to end on synthetic sessions: sessions -> ``data.SessionParallelLoader`` -> epochs of
``GRU4RecEngine.train_an_epoch`` -> ``recommend_next`` -> hit-rate@10 on each session's held-out last event.

    python examples/gru4rec_end_to_end.py                      # 4000 sessions, 2000 items, layers [100], 10 epochs
    python examples/gru4rec_end_to_end.py --sessions 512 --items 60 --group 10 --layers 32 --epochs 30

The sessions have a planted transition structure: the catalogue is cut into groups of ``--group`` items, a session stays
inside one group and walks its ring -- the next item is one to three places further four times out of five, any item of
the group otherwise (one time in twenty any item at all).  The last event therefore tells the next one, and the carried
state tells the group.

Prints one JSON line with the mean loss per epoch, the hit rate, the ``top / n_items`` of a random ranking and
``margin``: four binomial standard deviations of that chance rate at this number of sessions -- a hit rate above
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
    """A list of id lists, ids in 0 .. n_items - 1 (time order)."""
    rng = np.random.default_rng(seed)
    n_groups = max(1, n_items // group)
    out = []
    for _ in range(n_sessions):
        lo = int(rng.integers(0, n_groups)) * group
        n = int(rng.integers(min_len, max_len + 1))
        at = int(rng.integers(0, group))
        items = [lo + at]
        while len(items) < n:
            r = rng.random()
            if r < 0.8:
                at = (at + int(rng.integers(1, 4))) % group
                items.append(lo + at)
            elif r < 0.95:
                at = int(rng.integers(0, group))
                items.append(lo + at)
            else:
                items.append(int(rng.integers(0, n_items)))
        out.append(items)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sessions", type=int, default=4000)
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--group", type=int, default=25)
    ap.add_argument("--layers", type=int, nargs="+", default=[100])
    ap.add_argument("--loss", default="bpr-max", choices=["bpr-max", "cross-entropy"])
    ap.add_argument("--bpreg", type=float, default=1.0)
    ap.add_argument("--elu-param", type=float, default=0.5)
    ap.add_argument("--logq", type=float, default=0.0)
    ap.add_argument("--n-sample", type=int, default=256)
    ap.add_argument("--sample-alpha", type=float, default=0.5)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--dropout-embed", type=float, default=0.0)
    ap.add_argument("--dropout-hidden", type=float, default=0.1)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    import torch

    import beta_recsys_amd as hp
    from beta_recsys_amd.data import SessionParallelLoader

    torch.manual_seed(args.seed)
    sessions = synthetic_sessions(args.sessions, args.items, args.group, 4, 14, args.seed)
    train = [s[:-1] for s in sessions]                       # the last event of every session is held out
    target = np.array([s[-1] for s in sessions])
    cfg = {"model": {"layers": args.layers, "constrained_embedding": True, "loss": args.loss, "bpreg": args.bpreg,
                     "elu_param": args.elu_param, "logq": args.logq, "n_sample": args.n_sample,
                     "sample_alpha": args.sample_alpha, "dropout_p_embed": args.dropout_embed,
                     "dropout_p_hidden": args.dropout_hidden, "batch_size": args.batch_size, "lr": args.lr,
                     "optimizer": "adam", "device_str": "cuda:0", "dropout_rng": "device", "dropout_seed": args.seed},
           "dataset": {"n_items": args.items}, "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.GRU4RecEngine(cfg)
    loader = SessionParallelLoader(train, args.items, args.batch_size, args.n_sample, args.sample_alpha, seed=args.seed)
    losses = []
    for epoch in range(args.epochs):
        with contextlib.redirect_stdout(io.StringIO()):
            losses.append(float(eng.train_an_epoch(loader, epoch)))
    loader.close()

    # nothing is excluded: the walk revisits items, so the held-out one has usually been seen
    top, _ = eng.recommend_next(train, args.top)
    top = top.cpu().numpy()
    hit = float((top == target[:, None]).any(axis=1).mean())
    chance = args.top / args.items
    margin = 4.0 * float(np.sqrt(chance * (1.0 - chance) / args.sessions))
    result = {"example": "gru4rec_end_to_end", "sessions": args.sessions, "items": args.items, "layers": args.layers,
              "loss": args.loss, "epochs": args.epochs, "steps_per_epoch": len(loader), "mean_loss_per_epoch": losses,
              f"hit_rate@{args.top}": hit, "random_hit_rate": chance, "margin": margin}
    print(json.dumps(result))
    return result, top


if __name__ == "__main__":
    main()
