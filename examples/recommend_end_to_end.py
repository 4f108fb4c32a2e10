"""From a trained model to recommendations, on the device: train BPR-MF for a few epochs, evaluate it by ranking the
WHOLE catalogue (the protocol of the LightGCN / UltraGCN papers), and print the best unseen items of a few users.

    python examples/recommend_end_to_end.py [--epochs 5] [--top 10]

Stages:
  * training set / epochs   as in examples/mf_end_to_end.py (device-side negatives, one fused kernel per step)
  * evaluation              beta_recsys_amd.evaluate_full: candidates are every item not in the user's training rows,
                            truth is the held-out rows; recommend at max(k) + hiprec_topk_metrics, no candidate frame
  * recommendations         engine.recommend(users, k, seen=training rows): one fused pass over the item factors
                            (csrc/topk.hip), the seen items masked, only k ids and scores per user leave the CU
The data is synthetic with planted user / item groups (see siblings_end_to_end.py), so a model that learns puts a held-out
item of the user's group near the top.  Prints one JSON line per epoch, then the recommendations.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import types

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
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=2048)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--show-users", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    import beta_recsys_amd as hp

    torch.manual_seed(2020)
    U, I = args.users, args.items
    users, items = planted_interactions(U, I, args.interactions, args.groups, seed=1)
    # hold out two interactions of every user that has more than four
    rng = np.random.default_rng(2)
    order = np.lexsort((rng.random(users.size), users))
    rank = np.arange(users.size) - np.searchsorted(users[order], users[order])
    count = np.bincount(users, minlength=U)[users[order]]
    held = order[(rank < 2) & (count > 4)]
    mask = np.ones(users.size, dtype=bool)
    mask[held] = False
    train = {"col_user": users[mask], "col_item": items[mask], "col_rating": np.ones(int(mask.sum()), dtype=np.float32)}
    test = {"col_user": users[held], "col_item": items[held], "col_rating": np.ones(held.size, dtype=np.float32)}
    data = types.SimpleNamespace(train=train, n_users=U, n_items=I)

    cfg = {"model": dict(n_users=U, n_items=I, emb_dim=args.emb_dim, device_str="cuda:0", optimizer="adam", lr=args.lr,
                         batch_size=args.batch_size, loss="bpr"),
           "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.MFEngine(cfg)
    history = []
    for epoch in range(args.epochs):
        with contextlib.redirect_stdout(io.StringIO()):
            loader = hp.data.instance_bpr_loader(data, args.batch_size, "cuda:0")     # fresh negatives every epoch
            eng.train_an_epoch(loader, epoch)
        metrics = hp.evaluate_full(eng, test, train, metrics=["ndcg", "recall", "precision"], k_li=[5, 10, 20])
        row = {"epoch": epoch, "loss": round(eng.epoch_stats().loss_sum / max(len(loader), 1), 5),
               **{k: round(v, 4) for k, v in metrics.items()}}
        history.append(row)
        print(json.dumps(row), flush=True)

    show = np.unique(users[held])[: args.show_users]
    rec_items, rec_scores = eng.recommend(show, args.top, seen=(train["col_user"], train["col_item"]))
    for u, its, scs in zip(show.tolist(), rec_items.cpu().tolist(), rec_scores.cpu().tolist()):
        print(json.dumps({"user": u, "held_out": sorted(int(i) for i in items[held][users[held] == u]),
                          "recommended": its, "scores": [round(s, 4) for s in scs]}), flush=True)
    return history


if __name__ == "__main__":
    main()
