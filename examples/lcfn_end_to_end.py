"""End-to-end run of LCFN on the device: clustered synthetic log -> spectral bases -> epochs of (user, pos, neg) batches
(training steps in csrc/lcfn.hip) -> full-catalogue ranking of the held-out items.

    python examples/lcfn_end_to_end.py [--epochs 8]

Stages (reference file:line -> here):
  * bases        data/deprecated_data_base.py:411-467 create_graph_embeddings: the low eigenvectors of the two
                 hypergraph Laplacians, cut at cut_off * n                               -> beta_recsys_amd.data.graph_embeddings
  * loader       data/base_data.py instance_bpr_loader: (user, pos, neg) batches          -> DeviceTripleBatcher, fresh
                 uniform negatives per epoch
  * epoch        models/lcfn.py:154-169 train_an_epoch                                    -> LCFNEngine.train_an_epoch
  * evaluation   the whole catalogue minus the training rows, NDCG@10                     -> beta_recsys_amd.evaluate_full
The data is synthetic with planted structure (siblings_end_to_end.planted_interactions: 90 % of a user's items lie in
the user's group), leave-one-out.  Prints one JSON line per epoch, epoch -1 being the untrained model, next to the NDCG@10
a random ranking of the candidates would reach.

The defaults are the reference's (configs/lcfn_default.json: Adam, lr 0.05, lamda 0.005).  The regulariser is a sum of
UNSQUARED norms, whose gradient does not shrink with the weights: at lr 0.02 it holds the tables at their tiny initial
scale and nothing is learnt (the fp32 restatement on the CPU behaves the same).

tests/test_lcfn_example_gpu.py runs the small default and asks that NDCG@10 ends above the untrained model's and above
chance.
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

from sgl_end_to_end import dataset  # noqa: E402


def chance_ndcg(n_items, train_per_user, k=10):
    """NDCG@k of a uniformly random ranking with ONE relevant item among the candidates a user has left."""
    n = max(n_items - train_per_user, 1.0)
    return float(sum(1.0 / np.log2(r + 1) for r in range(1, k + 1)) / n)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=300)
    ap.add_argument("--items", type=int, default=200)
    ap.add_argument("--interactions", type=int, default=6000)
    ap.add_argument("--emb-dim", type=int, default=32)
    ap.add_argument("--layer", type=int, default=1)
    ap.add_argument("--cut-off", type=float, default=0.1)
    ap.add_argument("--lamda", type=float, default=0.005)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--train-filters", action="store_true")
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    import beta_recsys_amd as hp
    from beta_recsys_amd.data import graph_embeddings

    tr_u, tr_i, te_u, te_i = dataset(args.users, args.items, args.interactions)
    bases = graph_embeddings(tr_u, tr_i, args.users, args.items, args.cut_off)
    torch.manual_seed(0)
    np.random.seed(0)            # the transformers' draws (the reference's generator)
    model = dict(n_users=args.users, n_items=args.items, emb_dim=args.emb_dim, layer=args.layer, lamda=args.lamda,
                 graph_embeddings=bases, train_filters=args.train_filters, optimizer="adam", lr=args.lr,
                 device_str="cuda:0", batch_size=args.batch_size)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.LCFNEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_example_runs"}})
    users_d, items_d = torch.from_numpy(tr_u).cuda(), torch.from_numpy(tr_i).cuda()
    train = {"col_user": tr_u, "col_item": tr_i, "col_rating": np.ones(tr_u.size, dtype=np.float32)}
    test = {"col_user": te_u, "col_item": te_i, "col_rating": np.ones(te_u.size, dtype=np.float32)}
    chance = chance_ndcg(args.items, tr_u.size / args.users)
    history = []
    for epoch in range(-1, args.epochs):
        loss, parts = None, None
        if epoch >= 0:
            neg = torch.randint(0, args.items, (tr_u.size,), device="cuda")
            loader = hp.DeviceTripleBatcher(users_d, items_d, neg, args.batch_size)
            with contextlib.redirect_stdout(io.StringIO()):
                eng.train_an_epoch(loader, epoch)
            loss = eng.writer.scalars[-1][1] / len(loader)
            parts = eng.last_losses()
        metrics = hp.evaluate_full(eng, test, train, metrics=["ndcg", "recall"], k_li=[10])
        rec = {"model": "lcfn", "epoch": epoch, "loss": loss, "last_parts": parts, "ndcg@10": float(metrics["ndcg@10"]),
               "recall@10": float(metrics["recall@10"]), "chance_ndcg@10": chance,
               "frequencies": [int(b.shape[1]) for b in bases]}
        history.append(rec)
        print(json.dumps(rec), flush=True)
    return history


if __name__ == "__main__":
    main()
