"""End-to-end run of MixGCF on the device: graph -> (user, pos, candidates) batches -> training steps in
csrc/mixgcf.hip -> full-catalogue ranking of the held-out items.

    python examples/mixgcf_end_to_end.py [--epochs 6]

Stages (reference file:line -> here):
  * graph        data/deprecated_data_base.py:331-353 norm_adj D^-1 (A + I)  -> siblings_end_to_end.norm_adj
  * batches      data/base_data.py:254-288 instance_mul_neg_loader           -> ``epoch_batches``: (user, pos,
                 neg[K * n_negs]) drawn with numpy, so that a CPU run of the restatement sees the same batches
  * steps        models/mixgcf.py:176-220                                    -> MixGCFEngine.train_an_epoch (which, unlike
                 the reference's, also takes the gradient and steps the optimizer)
  * evaluation   the whole catalogue minus the training rows, NDCG@10        -> beta_recsys_amd.evaluate_full
The data is synthetic with planted structure (siblings_end_to_end.planted_interactions: 90 % of a user's items lie in
the user's group), leave-one-out.  Prints one JSON line per epoch, epoch -1 being the untrained model.

Margin: at the test's size (``--users 300 --items 200 --interactions 6000 --emb-dim 32 --epochs 6``) the numpy
restatement (tests/mixgcf_numpy.py), trained on the CPU from the same initial weights, batches and mixing seeds, takes
full-catalogue NDCG@10 from 0.045 untrained to 0.386 after six epochs (0.380 after the first: on this data the propagation
does most of the work once the tables stop being noise), a gain of 0.34.  tests/test_mixgcf_example_gpu.py asks the
device run for a gain of 0.2 and a falling loss (the restatement's mean step loss falls from 0.693 to 0.644).
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

from siblings_end_to_end import norm_adj, planted_interactions  # noqa: E402


def dataset(n_users, n_items, n_interactions, seed=1):
    """Leave-one-out split of the planted interactions: ``(train_users, train_items, test_users, test_items)``."""
    users, items = planted_interactions(n_users, n_items, n_interactions, 8, seed=seed)
    rng = np.random.default_rng(seed + 1)
    order = np.lexsort((rng.random(users.size), users))
    users, items = users[order], items[order]
    last = np.r_[users[1:] != users[:-1], True]
    return users[~last], items[~last], users[last], items[last]


def epoch_batches(tr_u, tr_i, n_items, batch_size, n_cand, seed):
    """One shuffled pass over the training rows with ``n_cand`` uniform candidate items per row."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(tr_u.size)
    neg = rng.integers(0, n_items, (tr_u.size, n_cand))
    return [(tr_u[perm[a:a + batch_size]], tr_i[perm[a:a + batch_size]], neg[perm[a:a + batch_size]])
            for a in range(0, tr_u.size, batch_size)]


def model_config(args, adj):
    return dict(n_users=args.users, n_items=args.items, emb_dim=args.emb_dim, pool="mean", context_hops=args.hops,
                mess_dropout=False, mess_dropout_rate=0.1, edge_dropout=False, edge_dropout_rate=0.5, norm_adj=adj,
                l2=1e-4, n_negs=args.n_negs, ns="mixgcf", K=args.K, optimizer="adam", lr=args.lr, device_str="cuda:0",
                batch_size=args.batch_size)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=2000)
    ap.add_argument("--items", type=int, default=1500)
    ap.add_argument("--interactions", type=int, default=120_000)
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--hops", type=int, default=3)
    ap.add_argument("--n-negs", type=int, default=8)
    ap.add_argument("--K", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--epochs", type=int, default=6)
    ap.add_argument("--lr", type=float, default=0.01)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    import beta_recsys_amd as hp

    tr_u, tr_i, te_u, te_i = dataset(args.users, args.items, args.interactions)
    adj = norm_adj(args.users, args.items, tr_u, tr_i)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.MixGCFEngine({"model": model_config(args, adj), "system": {"run_dir": "/tmp/hiprec_example_runs"}})
    train = {"col_user": tr_u, "col_item": tr_i, "col_rating": np.ones(tr_u.size, dtype=np.float32)}
    test = {"col_user": te_u, "col_item": te_i, "col_rating": np.ones(te_u.size, dtype=np.float32)}
    history = []
    for epoch in range(-1, args.epochs):
        loss = None
        if epoch >= 0:
            batches = epoch_batches(tr_u, tr_i, args.items, args.batch_size, args.K * args.n_negs, seed=100 + epoch)
            with contextlib.redirect_stdout(io.StringIO()):
                eng.train_an_epoch(batches, epoch)
            loss = eng.writer.scalars[-1][1] / len(batches)
        metrics = hp.evaluate_full(eng, test, train, metrics=["ndcg", "recall"], k_li=[10])
        rec = {"model": "mixgcf", "epoch": epoch, "loss": loss, "ndcg@10": float(metrics["ndcg@10"]),
               "recall@10": float(metrics["recall@10"])}
        history.append(rec)
        print(json.dumps(rec), flush=True)
    return history


if __name__ == "__main__":
    main()
