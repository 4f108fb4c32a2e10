"""Implicit ALS (WRMF) on the device, end to end: a synthetic clustered log, a few exact sweeps, full-catalogue
evaluation, recommendations, and factor rows for users the training frame never saw.

    python examples/als_end_to_end.py [--users 2000] [--items 1500] [--dim 32] [--epochs 5]

Stages:
  * data          planted user / item groups (see siblings_end_to_end.py); one interaction of every user with more than
                  four is held out; the last --fold-users of those users are kept out of the training frame altogether
  * prepare       both CSRs of the training frame with their multiplicities and the longest-first row orders (torch)
  * train         per epoch a user half-sweep, an item half-sweep (csrc/als.hip: a Gram launch and a solve launch each,
                  one block per row, the normal equation assembled on the fp32 MFMA and factored in LDS) and the loss
  * evaluate      evaluate_full on the held-out items; recommend() for hit-rate@10 against chance and against the
                  untrained tables
  * fold-in       the kept-out users' rows from one solve each against the trained item table, then the same hit-rate
Prints one JSON line per epoch, one summary line, then a few lists.
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


def hit_rate(rec_items, truth):
    return float((rec_items.cpu().numpy() == truth[:, None]).any(axis=1).mean())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=2000)
    ap.add_argument("--items", type=int, default=1500)
    ap.add_argument("--interactions", type=int, default=120_000)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--dim", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=40.0)
    ap.add_argument("--reg", type=float, default=0.1)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--fold-users", type=int, default=200)
    ap.add_argument("--show-users", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    import beta_recsys_amd as hp
    from beta_recsys_amd.knn import build_interaction_csr
    from beta_recsys_amd.recommend import topk_factors

    U, I = args.users, args.items
    users, items = planted_interactions(U, I, args.interactions, args.groups, seed=1)
    rng = np.random.default_rng(2)
    order = np.lexsort((rng.random(users.size), users))
    rank = np.arange(users.size) - np.searchsorted(users[order], users[order])
    count = np.bincount(users, minlength=U)[users[order]]
    held = order[(rank < 1) & (count > 4)]                       # one held-out item per user
    mask = np.ones(users.size, dtype=bool)
    mask[held] = False
    test_users, test_items = users[held], items[held]
    folded = np.sort(test_users)[test_users.size - args.fold_users:] if args.fold_users else np.zeros(0, dtype=np.int64)
    in_frame = mask & ~np.isin(users, folded)
    train_users, train_items = users[in_frame], items[in_frame]
    keep = ~np.isin(test_users, folded)
    eval_users, eval_items = test_users[keep], test_items[keep]
    chance = float(np.mean(np.minimum(args.top / (I - np.bincount(users[mask], minlength=U)[test_users]), 1.0)))

    torch.manual_seed(0)
    cfg = {"model": dict(n_users=U, n_items=I, emb_dim=args.dim, alpha=args.alpha, reg=args.reg, device_str="cuda:0"),
           "system": {"run_dir": "/tmp/hiprec_als_example"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.ALSEngine(cfg)
    eng.prepare((train_users, train_items))
    seen = eng.seen_csr()
    untrained = hit_rate(eng.recommend(eval_users, args.top, seen=seen)[0], eval_items)
    print(json.dumps({"epoch": -1, "loss": eng.loss()}), flush=True)
    for epoch in range(args.epochs):
        with contextlib.redirect_stdout(io.StringIO()):
            loss = eng.train_an_epoch(None, epoch)
        print(json.dumps({"epoch": epoch, "loss": loss, "regularizer": eng.last_regularizer}), flush=True)
    metrics = hp.evaluate_full(eng, {"col_user": eval_users, "col_item": eval_items},
                               {"col_user": train_users, "col_item": train_items}, k_li=(args.top,))
    rec_items, rec_scores = eng.recommend(eval_users, args.top, seen=seen)
    summary = {"model": "ALS", "users": int(eval_users.size), "dim": args.dim, "epochs": args.epochs,
               f"hit_rate@{args.top}": round(hit_rate(rec_items, eval_items), 4),
               f"untrained_hit_rate@{args.top}": round(untrained, 4), "chance": round(chance, 4),
               f"ndcg@{args.top}": round(float(metrics[f"ndcg@{args.top}"]), 4)}

    # fold-in: users the frame never held, from their lists alone (the held-out item is not in them)
    if folded.size:
        dev = eng.model.flat.device
        new_id = np.searchsorted(folded, users[mask & np.isin(users, folded)])
        f_ptr, f_idx, f_val = build_interaction_csr(torch.from_numpy(new_id).to(dev),
                                                    torch.from_numpy(items[mask & np.isin(users, folded)]).to(dev),
                                                    folded.size, I)
        before = eng.model.flat.clone()
        rows = eng.model.fold_in(f_ptr, f_idx, f_val)
        assert torch.equal(before, eng.model.flat)
        f_items, _ = topk_factors(rows, eng.model.ranking_factors()[1], 1.0, None,
                                  torch.arange(folded.size, device=dev), args.top, seen=(f_ptr, f_idx))
        truth = test_items[np.argsort(test_users)][np.searchsorted(np.sort(test_users), folded)]
        summary["folded_users"] = int(folded.size)
        summary[f"folded_hit_rate@{args.top}"] = round(hit_rate(f_items, truth), 4)
    print(json.dumps(summary), flush=True)
    for u, held_item, its, scs in list(zip(eval_users.tolist(), eval_items.tolist(), rec_items.cpu().tolist(),
                                           rec_scores.cpu().tolist()))[: args.show_users]:
        print(json.dumps({"user": u, "held_out": held_item, "recommended": its, "scores": [round(s, 4) for s in scs]}),
              flush=True)
    return summary


if __name__ == "__main__":
    main()
