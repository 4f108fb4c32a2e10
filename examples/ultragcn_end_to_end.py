"""End-to-end run of UltraGCN on the device — what ``examples/train_ultragcn.py`` of the reference does per run, with
every stage on the MI355X.

    python examples/ultragcn_end_to_end.py [--epochs 8]

Stages (reference file:line -> here):
  * constraints      data/base_data.py:410-431 create_constraint_mat      -> beta_uD / beta_iD from the train matrix
                     models/ultragcn.py:9-33 get_ii_constraint_mat         -> beta_recsys_amd.get_ii_constraint_mat (sparse)
  * loader           data/base_data.py:254-288 instance_mul_neg_loader     -> beta_recsys_amd.data.instance_mul_neg_loader
                     (fresh device-side negatives every epoch, batches of (user, pos, neg[N]))
  * epochs           models/ultragcn.py:218-236 train_an_epoch             -> UltraGCNEngine.train_an_epoch: one C call
  * validation       core/eval_engine.py:49-87, 231-274                    -> model.predict + beta_recsys_amd.eval.rank_metrics
                     (leave-one-out: 1 held-out positive + sampled negatives per user)
The data is synthetic with planted structure (see siblings_end_to_end.py), so that a model that learns ranks a held-out
positive above sampled negatives.  Prints one JSON line per epoch.
"""
import argparse
import contextlib
import io
import json
import os
import sys
import types

import numpy as np
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from siblings_end_to_end import planted_interactions, validate  # noqa: E402


def constraint_mat(n_users, n_items, users, items):
    """base_data.py:410-431: the 0/1 train matrix (fp32) and the two degree vectors."""
    train_mat = sp.csr_matrix((np.ones(len(users), dtype=np.float32), (users, items)), shape=(n_users, n_items))
    train_mat.data[:] = 1.0
    items_D = np.asarray(train_mat.sum(axis=0)).reshape(-1)
    users_D = np.asarray(train_mat.sum(axis=1)).reshape(-1)
    with np.errstate(divide="ignore"):
        beta_uD = (np.sqrt(users_D + 1) / users_D).astype(np.float32)
    beta_uD[users_D == 0] = 0.0        # a user with no training row never occurs in a batch
    beta_iD = (1 / np.sqrt(items_D + 1)).astype(np.float32)
    return train_mat, {"beta_uD": beta_uD, "beta_iD": beta_iD}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=2000)
    ap.add_argument("--items", type=int, default=1500)
    ap.add_argument("--interactions", type=int, default=120_000)
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=1000)
    ap.add_argument("--negatives", type=int, default=20)
    ap.add_argument("--neighbors", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--lr", type=float, default=0.05)   # ultragcn_default.json
    ap.add_argument("--eval-negatives", type=int, default=50)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    import pandas as pd

    import beta_recsys_amd as hp

    U, I, dev = args.users, args.items, torch.device("cuda:0")
    users, items = planted_interactions(U, I, args.interactions, 8, seed=1)
    rng = np.random.default_rng(2)
    # leave-one-out: the last interaction of every user (in this order) is held out
    order = np.lexsort((rng.random(users.size), users))
    users, items = users[order], items[order]
    last = np.r_[users[1:] != users[:-1], True]
    tr_u, tr_i, te_u, te_i = users[~last], items[~last], users[last], items[last]
    k = args.eval_negatives
    all_u, all_i = torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev)
    neg = hp.data.sample_negatives(all_u, all_i, U, I, k=k, seed=3)[torch.from_numpy(np.flatnonzero(last)).to(dev)]
    ev_u = torch.from_numpy(te_u).to(dev).repeat_interleave(k + 1)
    # the positive goes LAST in its user's block: ties rank by first occurrence, so a constant scorer gets 0
    ev_i = torch.cat([neg, torch.from_numpy(te_i).to(dev)[:, None]], 1).reshape(-1)
    ratings = torch.tensor([0.0] * k + [1.0], device=dev).repeat(len(te_u))

    train_mat, cmat = constraint_mat(U, I, tr_u, tr_i)
    torch.manual_seed(0)
    # ultragcn_default.json: w1 1e-7, w2 1, w3 1e-7, w4 1, negative_weight 200, gamma 1e-4, lambda 1e-3
    cfg = {"model": dict(n_users=U, n_items=I, emb_dim=args.emb_dim, batch_size=args.batch_size, regs=[1e-5],
                         device_str="cuda:0", optimizer="adam", lr=args.lr, w1=1e-7, w2=1.0, w3=1e-7, w4=1.0,
                         negative_weight=200.0, gamma=1e-4, train_mat=train_mat, constraint_mat=cmat,
                         ii_neighbor_num=args.neighbors, **{"lambda": 1e-3}),
           "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.UltraGCNEngine(cfg)
    frame = types.SimpleNamespace(train=pd.DataFrame({"col_user": tr_u, "col_item": tr_i}), n_users=U, n_items=I)
    history = []
    for epoch in range(args.epochs):
        with contextlib.redirect_stdout(io.StringIO()):
            loader = hp.data.instance_mul_neg_loader(frame, args.batch_size, dev, args.negatives, seed=100 + epoch)
            eng.train_an_epoch(loader, epoch)
        ndcg, recall = validate(eng.model, ev_u, ev_i, ratings, hp)
        rec = {"model": "ultragcn", "epoch": epoch, "loss": eng.writer.scalars[-1][1] / len(tr_u), "ndcg@10": ndcg,
               "recall@10": recall}
        history.append(rec)
        print(json.dumps(rec), flush=True)
    return history


if __name__ == "__main__":
    main()
