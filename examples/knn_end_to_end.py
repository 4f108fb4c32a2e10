"""The two neighbourhood baselines, on the device: ItemKNN and UserKNN on a synthetic clustered log, recommendations for
every user with a held-out item, and hit-rate@10 against chance.

    python examples/knn_end_to_end.py [--users 2000] [--items 1500] [--neighbourhood-size 50]

Stages:
  * data              planted user / item groups (see siblings_end_to_end.py); one interaction of every user with more
                      than four is held out
  * prepare_model     both CSRs of the training frame with their multiplicities (torch), and for ItemKNN the
                      [n_items, n_items] similarity matrix (csrc/knn.hip: one block per row)
  * recommend         the 10 best items the user has not interacted with: ItemKNN adds the similarity rows of the user's
                      items; UserKNN finds the neighbours, adds their rows weighted by similarity -- one block per user,
                      nothing but the lists leaves the CU
  * hit-rate@10       share of users whose held-out item is among the 10; chance is 10 / (items the user has not seen)
Prints one JSON line per model, then a few lists.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from siblings_end_to_end import planted_interactions  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=2000)
    ap.add_argument("--items", type=int, default=1500)
    ap.add_argument("--interactions", type=int, default=120_000)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--neighbourhood-size", type=int, default=50)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--show-users", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    import beta_recsys_amd as hp

    U, I = args.users, args.items
    users, items = planted_interactions(U, I, args.interactions, args.groups, seed=1)
    rng = np.random.default_rng(2)
    order = np.lexsort((rng.random(users.size), users))
    rank = np.arange(users.size) - np.searchsorted(users[order], users[order])
    count = np.bincount(users, minlength=U)[users[order]]
    held = order[(rank < 1) & (count > 4)]                       # one held-out item per user
    mask = np.ones(users.size, dtype=bool)
    mask[held] = False
    train_users, train_items = users[mask], items[mask]
    test_users, test_items = users[held], items[held]
    unseen = I - np.bincount(train_users, minlength=U)[test_users]
    chance = float(np.mean(np.minimum(args.top / unseen, 1.0)))

    results = []
    for name, engine_cls in (("ItemKNN", hp.ItemKNNEngine), ("UserKNN", hp.UserKNNEngine)):
        cfg = {"model": dict(n_users=U, n_items=I, neighbourhood_size=args.neighbourhood_size, device_str="cuda:0")}
        with contextlib.redirect_stdout(io.StringIO()):
            eng = engine_cls(cfg)
            eng.train_an_epoch(None, 0)                           # "[Training Epoch 0] skipped": nothing to train
        eng.model.prepare_model((train_users, train_items))
        rec_items, rec_scores = eng.recommend(test_users, args.top, seen=eng.model.seen_csr())
        hits = (rec_items.cpu().numpy() == test_items[:, None]).any(axis=1)
        row = {"model": name, "users": int(test_users.size), f"hit_rate@{args.top}": round(float(hits.mean()), 4),
               "chance": round(chance, 4)}
        results.append(row)
        print(json.dumps(row), flush=True)
        for u, held_item, its, scs in list(zip(test_users.tolist(), test_items.tolist(), rec_items.cpu().tolist(),
                                               rec_scores.cpu().tolist()))[: args.show_users]:
            print(json.dumps({"model": name, "user": u, "held_out": held_item, "recommended": its,
                              "scores": [round(s, 4) for s in scs]}), flush=True)
    return results


if __name__ == "__main__":
    main()
