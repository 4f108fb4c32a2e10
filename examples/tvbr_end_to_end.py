"""TVBR end to end on synthetic timestamped baskets: baskets with a time -> (u, i1, i2, T) triples -> N(0, 1) side
features -> alias samplers -> epochs of ``TVBREngine.train_an_epoch`` over the time steps -> ``engine.recommend`` over the
whole catalogue -> hit-rate@10 on each user's held-out item.

    python examples/tvbr_end_to_end.py                          # 2000 users, 1500 items, 10 time steps, 8 epochs
    python examples/tvbr_end_to_end.py --users 300 --items 200 --epochs 6

Users and items fall into groups; a basket holds items of its user's group nine times out of ten and carries a
timestamp.  The timestamps are cut into ``time_step`` equally filled bins, the ``T`` column of the triple frame, as the
reference's grocery loaders do.  One item per user is held out of every basket of that user; the rest of each basket
gives the ordered pairs (i1, i2) of its items.  The features are random (N(0, 1), 512 wide).  Negatives come from
frequency alias tables through ``engine.data.user_sampler`` / ``item_sampler``, as in the reference's epoch loop.  Prints
one JSON line with the epoch losses (``total_loss`` as ``train_an_epoch`` logs it), the hit rate of the trained model,
that of the untrained model and the 10 / n_items of a random ranking.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from vbcar_end_to_end import AliasSampler, hit_rate  # noqa: E402  (the same samplers and metric)


def synthetic_timed_baskets(n_users, n_items, n_groups, baskets_per_user, time_step, seed):
    """``(frame of (UID, TID1, TID2, T), held_out [n_users], seen (users, items))``: every user's held-out item is one of
    its own group's and occurs in none of its training baskets; ``T`` is the basket's timestamp bin."""
    import pandas as pd

    rng = np.random.default_rng(seed)
    by_group = [np.flatnonzero(np.arange(n_items) % n_groups == g) for g in range(n_groups)]
    rows, stamps, held_out, seen_u, seen_i = [], [], np.zeros(n_users, dtype=np.int64), [], []
    for u in range(n_users):
        own = by_group[u % n_groups]
        held_out[u] = rng.choice(own)
        for _ in range(baskets_per_user):
            stamp = rng.random()
            size = int(rng.integers(2, 6))
            inside = rng.random(size) < 0.9
            basket = np.unique(np.where(inside, rng.choice(own, size), rng.integers(0, n_items, size)))
            basket = basket[basket != held_out[u]]
            for a in basket:
                seen_u.append(u), seen_i.append(int(a))
                for b in basket:
                    if a != b:
                        rows.append((u, int(a), int(b)))
                        stamps.append(stamp)
    stamps = np.asarray(stamps)
    edges = np.quantile(stamps, np.linspace(0, 1, time_step + 1)[1:-1])
    frame = pd.DataFrame(rows, columns=["UID", "TID1", "TID2"])
    frame["T"] = np.searchsorted(edges, stamps).astype(np.int64)
    return frame, held_out, (np.asarray(seen_u), np.asarray(seen_i))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--users", type=int, default=2000)
    ap.add_argument("--items", type=int, default=1500)
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--baskets", type=int, default=6)
    ap.add_argument("--time-step", type=int, default=10)
    ap.add_argument("--fea-dim", type=int, default=512)
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--n-neg", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--alpha", type=float, default=0.001)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    import torch

    import beta_recsys_amd as hp

    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    torch.manual_seed(args.seed)
    U, I = args.users, args.items
    frame, held_out, seen = synthetic_timed_baskets(U, I, args.groups, args.baskets, args.time_step, args.seed)
    rng = np.random.default_rng(args.seed + 1)
    config = {"model": {"n_users": U, "n_items": I, "late_dim": 512, "emb_dim": args.emb_dim, "n_neg": args.n_neg,
                        "batch_size": args.batch_size, "alpha": args.alpha, "time_step": args.time_step,
                        "activator": "tanh", "optimizer": "rmsprop", "lr": args.lr, "device_str": "cuda:0",
                        "noise_rng": "device"},
              "user_fea": rng.standard_normal((U, args.fea_dim)), "item_fea": rng.standard_normal((I, args.fea_dim)),
              "system": {"run_dir": "/tmp/hiprec_tvbr_example"}}
    with contextlib.redirect_stdout(io.StringIO()):
        engine = hp.TVBREngine(config)
    engine.data = type("Data", (), {
        "user_sampler": AliasSampler(np.bincount(frame["UID"], minlength=U) + 1.0, args.seed + 2),
        "item_sampler": AliasSampler(np.bincount(frame["TID1"], minlength=I) + 1.0, args.seed + 3)})()
    untrained = hit_rate(engine, held_out, seen, args.top)
    losses = []
    steps = int(sum(n // args.batch_size for n in np.bincount(frame["T"], minlength=args.time_step)))
    for epoch in range(args.epochs):
        with contextlib.redirect_stdout(io.StringIO()):
            engine.train_an_epoch(frame, epoch)
        logged = dict((tag, v) for tag, v, step in engine.writer.scalars[-3:] if step == epoch)
        losses.append(float(logged["model/loss/total_loss"]))
    trained = hit_rate(engine, held_out, seen, args.top)
    print(json.dumps({"users": U, "items": I, "triples": int(len(frame)), "time_step": args.time_step,
                      "steps_per_epoch": steps, "total_loss_per_epoch": losses, f"hit_rate@{args.top}": trained,
                      f"untrained_hit_rate@{args.top}": untrained, "random_ranking": args.top / I}))


if __name__ == "__main__":
    main()
