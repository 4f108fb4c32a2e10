"""End-to-end run of SimGCL on the device: clustered synthetic log -> graph -> epochs of (user, pos, neg) batches (training
steps in csrc/simgcl.hip, the noise drawn on the device) -> full-catalogue ranking of the held-out items.

    python examples/simgcl_end_to_end.py [--epochs 3]

Stages (reference file:line -> here):
  * graph        the "pre" adjacency D^-1/2 A D^-1/2 of the data layer                  -> sgl_end_to_end.sym_norm_adj
  * loader       data/base_data.py instance_bpr_loader: (user, pos, neg) batches         -> DeviceTripleBatcher, fresh
                 uniform negatives per epoch
  * epoch        models/simgcl.py:135-151 train_an_epoch                                 -> SimGCLEngine.train_an_epoch
  * evaluation   the whole catalogue minus the training rows, NDCG@10                    -> beta_recsys_amd.evaluate_full
The data is synthetic with planted structure (siblings_end_to_end.planted_interactions: 90 % of a user's items lie in
the user's group), leave-one-out.  Prints one JSON line per epoch, epoch -1 being the untrained model, next to the NDCG@10
a random ranking of the candidates would reach.

``predict`` -- and with it the ranking -- reads the RAW tables (simgcl.py:72-82) while the loss is computed on the
propagated ones, so the untrained model ranks at chance (N(0, 1) tables) and what the ranking learns reaches the raw rows
through the backward chain only.  That makes the ranking a by-product of the training, and a fragile one: the same step
in torch autograd on the CPU shows NDCG@10 of the raw tables rising for the first epochs and falling again as the loss
keeps improving, falling from the first epoch on at the reference's default lambda 0.5 with two layers, and rising most
with an odd number of layers (whose hops put item rows into user rows) and a small lambda.  The defaults here are that
regime: three layers, lambda 0.1, lr 0.02, three epochs (0.03 -> 0.10, 0.14, 0.12 in the CPU replay).

tests/test_simgcl_example_gpu.py runs the small default and asks that NDCG@10 ends above the untrained model's.
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

from lcfn_end_to_end import chance_ndcg  # noqa: E402
from sgl_end_to_end import dataset, sym_norm_adj  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=300)
    ap.add_argument("--items", type=int, default=200)
    ap.add_argument("--interactions", type=int, default=6000)
    ap.add_argument("--emb-dim", type=int, default=32)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--reg", type=float, default=1e-4)
    ap.add_argument("--cl-rate", type=float, default=0.1)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--user-view", default="reference", choices=["reference", "two_views"])
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    import beta_recsys_amd as hp

    tr_u, tr_i, te_u, te_i = dataset(args.users, args.items, args.interactions)
    adj = sym_norm_adj(args.users, args.items, tr_u, tr_i)
    torch.manual_seed(0)         # the tables, and the default noise_seed
    model = dict(n_users=args.users, n_items=args.items, emb_dim=args.emb_dim, n_layer=args.layers, eps=args.eps,
                 reg=args.reg, norm_adj=adj, optimizer="adam", lr=args.lr, device_str="cuda:0",
                 batch_size=args.batch_size, user_view=args.user_view)
    model["lambda"] = args.cl_rate
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.SimGCLEngine({"model": model, "system": {"run_dir": "/tmp/hiprec_example_runs"}})
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
            loss = [v for t, v, _ in eng.writer.scalars if t == "model/loss"][-1] / len(loader)
            parts = eng.last_losses()
        metrics = hp.evaluate_full(eng, test, train, metrics=["ndcg", "recall"], k_li=[10])
        rec = {"model": "simgcl", "epoch": epoch, "loss": loss, "last_parts": parts, "ndcg@10": float(metrics["ndcg@10"]),
               "recall@10": float(metrics["recall@10"]), "chance_ndcg@10": chance}
        history.append(rec)
        print(json.dumps(rec), flush=True)
    print(f"NDCG@10 before training {history[0]['ndcg@10']:.4f}, after {history[-1]['ndcg@10']:.4f}")
    return history


if __name__ == "__main__":
    main()
