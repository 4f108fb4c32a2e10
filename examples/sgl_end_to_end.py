"""End-to-end run of SGL on the device: clustered synthetic log -> graph -> epochs (one sub-graph refresh each, training
steps in csrc/sgl.hip) -> full-catalogue ranking of the held-out items.

    python examples/sgl_end_to_end.py [--epochs 6]

Stages (reference file:line -> here):
  * graph        data/base_data.py create_sgl_mat / the "pre" adjacency D^-1/2 A D^-1/2     -> ``sym_norm_adj``
  * loader       data/base_data.py instance_bpr_loader: ``dataset.user_tensor`` /
                 ``dataset.pos_item_tensor`` + (user, pos, neg) batches                    -> ``Loader``
  * epoch        models/sgl.py:447-462 train_an_epoch: sub_mat_refresher, then every batch  -> SGLEngine.train_an_epoch
  * evaluation   the whole catalogue minus the training rows, NDCG@10                       -> beta_recsys_amd.evaluate_full
The data is synthetic with planted structure (siblings_end_to_end.planted_interactions: 90 % of a user's items lie in
the user's group), leave-one-out.  Prints one JSON line per epoch, epoch -1 being the untrained model.

tests/test_sgl_example_gpu.py runs ``--users 300 --items 200 --interactions 6000 --emb-dim 32 --epochs 6`` and asks that
NDCG@10 rises; on an MI355X it went from 0.05 untrained to 0.37 after the first epoch and 0.36 after the sixth.
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

from siblings_end_to_end import planted_interactions  # noqa: E402


def dataset(n_users, n_items, n_interactions, seed=1):
    """Leave-one-out split of the planted interactions (every pair once): ``(train_users, train_items, test_users,
    test_items)``."""
    users, items = planted_interactions(n_users, n_items, n_interactions, 8, seed=seed)
    key = np.unique(users.astype(np.int64) * n_items + items)
    users, items = key // n_items, key % n_items
    rng = np.random.default_rng(seed + 1)
    order = np.lexsort((rng.random(users.size), users))
    users, items = users[order], items[order]
    last = np.r_[users[1:] != users[:-1], True]
    return users[~last], items[~last], users[last], items[last]


def sym_norm_adj(n_users, n_items, users, items):
    """D^-1/2 A D^-1/2 over users + items as a scipy CSR matrix in fp32: what the reference's data layer hands SGL."""
    n = n_users + n_items
    a = sp.csr_matrix((np.ones(users.size, dtype=np.float32), (users, items + n_users)), shape=(n, n))
    a = a + a.T
    with np.errstate(divide="ignore"):
        d = np.power(np.asarray(a.sum(1)).flatten(), -0.5)
    d[np.isinf(d)] = 0.0
    return sp.diags(d).dot(a).dot(sp.diags(d)).tocsr().astype(np.float32)


class Loader:
    """What SGLEngine reads of a train loader: ``dataset.user_tensor`` / ``dataset.pos_item_tensor`` for the
    sub-graphs, and one shuffled pass of (user, pos, uniform negative) batches per iteration."""

    def __init__(self, users, items, n_items, batch_size, seed):
        self.dataset = types.SimpleNamespace(user_tensor=torch.from_numpy(users), pos_item_tensor=torch.from_numpy(items))
        self.users, self.items, self.n_items, self.batch_size = users, items, n_items, batch_size
        self.rng = np.random.default_rng(seed)

    def __len__(self):
        return (self.users.size + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        perm = self.rng.permutation(self.users.size)
        neg = self.rng.integers(0, self.n_items, self.users.size)
        for a in range(0, perm.size, self.batch_size):
            rows = perm[a:a + self.batch_size]
            yield self.users[rows], self.items[rows], neg[rows]


def model_config(args, adj):
    return dict(n_users=args.users, n_items=args.items, emb_dim=args.emb_dim, n_layers=args.layers, regs=1e-5,
                ssl_reg=args.ssl_reg, ssl_temp=0.5, ssl_mode="both_side", ssl_ratio=0.4, aug_type=1, is_subgraph=True,
                pretrain=0, norm_adj=adj, optimizer="adam", lr=args.lr, device_str="cuda:0", batch_size=args.batch_size)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=2000)
    ap.add_argument("--items", type=int, default=1500)
    ap.add_argument("--interactions", type=int, default=120_000)
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--ssl-reg", type=float, default=0.02)
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
    adj = sym_norm_adj(args.users, args.items, tr_u, tr_i)
    torch.manual_seed(0)
    np.random.seed(0)            # the sub-graphs' draws (sub_rng "numpy": the reference's generator)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.SGLEngine({"model": model_config(args, adj), "system": {"run_dir": "/tmp/hiprec_example_runs"}})
    loader = Loader(tr_u, tr_i, args.items, args.batch_size, seed=100)
    train = {"col_user": tr_u, "col_item": tr_i, "col_rating": np.ones(tr_u.size, dtype=np.float32)}
    test = {"col_user": te_u, "col_item": te_i, "col_rating": np.ones(te_u.size, dtype=np.float32)}
    history = []
    for epoch in range(-1, args.epochs):
        loss, parts = None, None
        if epoch >= 0:
            with contextlib.redirect_stdout(io.StringIO()):
                eng.train_an_epoch(loader, epoch)
            loss = eng.writer.scalars[-1][1] / len(loader)
            parts = eng.last_losses()
        metrics = hp.evaluate_full(eng, test, train, metrics=["ndcg", "recall"], k_li=[10])
        rec = {"model": "sgl", "epoch": epoch, "loss": loss, "last_parts": parts, "ndcg@10": float(metrics["ndcg@10"]),
               "recall@10": float(metrics["recall@10"])}
        history.append(rec)
        print(json.dumps(rec), flush=True)
    return history


if __name__ == "__main__":
    main()
