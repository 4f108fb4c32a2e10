"""End-to-end run of the Collaborative Memory Network on the device: both halves of what the reference's
``examples/train_cmn.py`` does per run.

    python examples/cmn_end_to_end.py [--pretrain-epochs 3] [--epochs 4]

Stages (reference file:line -> here):
  * pre-training     examples/train_cmn.py:62-99 train_gmf: PairwiseGMFEngine epochs, then the two tables are taken from
                     the model                                         -> PairwiseGMFEngine (csrc/pgmf.hip)
  * hand-over        examples/train_cmn.py:103-108 cmnEngine(config, user_embed, item_embed, data.item_users_list)
                                                                       -> cmnEngine (csrc/cmn.hip); the item -> users
                                                                          lists become a CSR on the device, once
  * negatives        data/deprecated_data.py:797-826 (neg_count uniform negatives per positive)
                                                                       -> beta_recsys_amd.data.sample_negatives(k=neg_count)
  * epochs           models/cmn.py:202-267 train_an_epoch               -> resident triples through hiprec_cmn_epoch
  * evaluation       full-catalogue ranking by predict = M[u] . E[i]    -> beta_recsys_amd.evaluate_full
  * recommendations                                                    -> engine.recommend
The data is synthetic with planted user / item groups (see siblings_end_to_end.py).  Prints one JSON line per epoch.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "examples")):
    if p not in sys.path:
        sys.path.insert(0, p)

from siblings_end_to_end import planted_interactions  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=943)
    ap.add_argument("--items", type=int, default=1682)
    ap.add_argument("--interactions", type=int, default=100_000)
    ap.add_argument("--groups", type=int, default=8)
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--batch-size", type=int, default=1024)
    ap.add_argument("--neg-count", type=int, default=4)
    ap.add_argument("--pretrain-epochs", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--lr", type=float, default=0.002)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--show-users", type=int, default=3)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    import beta_recsys_amd as hp

    torch.manual_seed(2020)
    U, I, D, B, K = args.users, args.items, args.emb_dim, args.batch_size, args.neg_count
    dev = torch.device("cuda:0")
    users, items = planted_interactions(U, I, args.interactions, args.groups, seed=1)
    rng = np.random.default_rng(2)
    order = np.lexsort((rng.random(users.size), users))
    rank = np.arange(users.size) - np.searchsorted(users[order], users[order])
    count = np.bincount(users, minlength=U)[users[order]]
    held = order[(rank < 2) & (count > 4)]
    mask = np.ones(users.size, dtype=bool)
    mask[held] = False
    train = {"col_user": users[mask], "col_item": items[mask], "col_rating": np.ones(int(mask.sum()), dtype=np.float32)}
    test = {"col_user": users[held], "col_item": items[held], "col_rating": np.ones(held.size, dtype=np.float32)}
    tu, ti = torch.from_numpy(train["col_user"]).to(dev), torch.from_numpy(train["col_item"]).to(dev)
    quiet = lambda: contextlib.redirect_stdout(io.StringIO())  # noqa: E731
    config = {"n_users": U, "n_items": I, "emb_dim": D, "device_str": "cuda:0", "regs": [1e-5], "batch_size": B,
              "lr": args.lr, "momentum": 0.9, "pretrain_l2_lambda": 1e-4, "training_l2_lambda": 1e-3, "grad_clip": 5.0,
              "neg_count": K, "model": {"device_str": "cuda:0", "optimizer": "adam", "lr": args.lr},
              "system": {"run_dir": "/tmp/hiprec_example_runs"}}
    history = []

    def triples(seed):
        """neg_count negatives per training pair, each positive ``neg_count`` times in a row as the loader emits them."""
        negs = hp.data.sample_negatives(tu, ti, U, I, k=K, seed=seed)
        return tu.repeat_interleave(K), ti.repeat_interleave(K), negs.reshape(-1)

    # ---- pre-training: PairwiseGMF on shuffled [B, 3] blocks ------------------------------------------------------
    with quiet():
        gmf = hp.PairwiseGMFEngine(config)
    for epoch in range(args.pretrain_epochs):
        rows = torch.stack(triples(100 + epoch), 1)
        rows = rows[torch.randperm(rows.shape[0], device=dev)]
        loader = [rows[s:s + B] for s in range(0, rows.shape[0], B)]
        with quiet():
            gmf.train_an_epoch(loader, epoch)
        history.append({"stage": "pairwise_gmf", "epoch": epoch, "loss": round(gmf.writer.scalars[-1][1] / len(loader), 5)})
        print(json.dumps(history[-1]), flush=True)
    user_embed = gmf.model.user_memory.weight.detach().cpu().numpy()
    item_embed = gmf.model.item_memory.weight.detach().cpu().numpy()

    # ---- hand-over: the tables and every item's neighbourhood (the users who interacted with it) ---------------------
    by_item = np.argsort(train["col_item"], kind="stable")
    cuts = np.searchsorted(train["col_item"][by_item], np.arange(I + 1))
    item_users_list = {i: train["col_user"][by_item[cuts[i]:cuts[i + 1]]].tolist() for i in range(I) if cuts[i + 1] > cuts[i]}
    with quiet():
        eng = hp.cmnEngine(config, user_embed, item_embed, item_users_list)

    # ---- CMN epochs: resident triples, the lists looked up in the CSR by the kernel -----------------------------------
    for epoch in range(args.epochs):
        loader = hp.data.DeviceTensorBatcher(triples(200 + epoch), B, shuffle=True)
        with quiet():
            eng.train_an_epoch(loader, epoch)
        metrics = hp.evaluate_full(eng, test, train, metrics=["ndcg", "recall"], k_li=[10, 20])
        history.append({"stage": "cmn", "epoch": epoch, "loss": round(eng.writer.scalars[-1][1] / len(loader), 5),
                        "max_neighbors": config["max_neighbors"], **{k: round(v, 4) for k, v in metrics.items()}})
        print(json.dumps(history[-1]), flush=True)

    show = np.unique(users[held])[: args.show_users]
    rec_items, rec_scores = eng.recommend(show, args.top, seen=(train["col_user"], train["col_item"]))
    for u, its in zip(show.tolist(), rec_items.cpu().tolist()):
        print(json.dumps({"user": u, "held_out": sorted(int(i) for i in items[held][users[held] == u]),
                          "recommended": its}), flush=True)
    return history, rec_items.cpu().numpy()


if __name__ == "__main__":
    main()
