"""SLIM on the device, end to end: a synthetic clustered log, the sparse non-negative item weights, full-catalogue
evaluation, recommendations, and lists for users the training frame never saw.

    python examples/slim_end_to_end.py [--users 2000] [--items 1500] [--l1 1] [--l2 50]

Stages:
  * data          planted user / item groups (see siblings_end_to_end.py); one interaction of every user with more than
                  four is held out; the last --fold-users of those users are kept out of the training frame altogether
  * prepare_model both CSRs of the training frame (torch), A = X^T X + l2 I by integer counting (csrc/ease.hip), then
                  csrc/slim.hip: every column of W by cyclic coordinate descent with a soft threshold, w >= 0
  * evaluate      evaluate_full on the held-out items; recommend() for hit-rate@10 against chance
  * held-out users  recommend_for() on the kept-out users' lists (the same score kernel on a temporary CSR)
Prints one summary line (with nnz and the sweep counts), then a few lists.
"""
import argparse
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
    ap.add_argument("--l1", type=float, default=1.0)
    ap.add_argument("--l2", type=float, default=50.0)      # planted groups make near-duplicate columns: l2 conditions them
    ap.add_argument("--tol", type=float, default=1e-5)
    ap.add_argument("--max-sweeps", type=int, default=300)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--fold-users", type=int, default=200)
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
    test_users, test_items = users[held], items[held]
    folded = np.sort(test_users)[test_users.size - args.fold_users:] if args.fold_users else np.zeros(0, dtype=np.int64)
    in_frame = mask & ~np.isin(users, folded)
    train_users, train_items = users[in_frame], items[in_frame]
    keep = ~np.isin(test_users, folded)
    eval_users, eval_items = test_users[keep], test_items[keep]
    chance = float(np.mean(np.minimum(args.top / (I - np.bincount(users[mask], minlength=U)[test_users]), 1.0)))

    eng = hp.SLIMEngine({"model": dict(n_users=U, n_items=I, l1_reg=args.l1, l2_reg=args.l2, tol=args.tol,
                                       max_sweeps=args.max_sweeps, device_str="cuda:0")})
    model = eng.model
    model.prepare_model((train_users, train_items))
    seen = model.seen_csr()
    metrics = hp.evaluate_full(eng, {"col_user": eval_users, "col_item": eval_items},
                               {"col_user": train_users, "col_item": train_items}, k_li=(args.top,))
    rec_items, rec_scores = eng.recommend(eval_users, args.top, seen=seen)
    sweeps = model.sweeps.cpu().numpy()
    summary = {"model": "SLIM", "users": int(eval_users.size), "items": I, "l1": args.l1, "l2": args.l2,
               "nnz": model.nnz, "density": round(model.nnz / (I * (I - 1)), 4),
               "sweeps": {"min": int(sweeps.min()), "median": float(np.median(sweeps)), "max": int(sweeps.max())},
               "n_unconverged": model.n_unconverged,
               f"hit_rate@{args.top}": round(hit_rate(rec_items, eval_items), 4), "chance": round(chance, 4),
               f"ndcg@{args.top}": round(float(metrics[f"ndcg@{args.top}"]), 4)}

    # users the frame never held, from their lists alone (the held-out item is not in them)
    if folded.size:
        sel = mask & np.isin(users, folded)
        by_user = np.argsort(np.searchsorted(folded, users[sel]), kind="stable")
        lengths = np.bincount(np.searchsorted(folded, users[sel]), minlength=folded.size)
        ptr = np.concatenate([[0], np.cumsum(lengths)])
        f_items, _ = model.recommend_for(ptr, items[sel][by_user], args.top)
        truth = test_items[np.argsort(test_users)][np.searchsorted(np.sort(test_users), folded)]
        summary["held_out_users"] = int(folded.size)
        summary[f"held_out_hit_rate@{args.top}"] = round(hit_rate(f_items, truth), 4)
    print(json.dumps(summary), flush=True)
    for u, held_item, its, scs in list(zip(eval_users.tolist(), eval_items.tolist(), rec_items.cpu().tolist(),
                                           rec_scores.cpu().tolist()))[: args.show_users]:
        print(json.dumps({"user": u, "held_out": held_item, "recommended": its, "scores": [round(s, 4) for s in scs]}),
              flush=True)
    return summary


if __name__ == "__main__":
    main()
