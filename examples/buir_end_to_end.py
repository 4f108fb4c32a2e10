"""End-to-end run of BUIR on the device: clustered synthetic log -> graph -> epochs of (user, pos, neg) batches (training
steps in csrc/buir.hip) -> top-K recommendation over the whole catalogue.

    python examples/buir_end_to_end.py [--epochs 4] [--update-target]

Stages (reference file:line -> here):
  * graph        the "pre" adjacency D^-1/2 A D^-1/2 of the data layer                  -> sgl_end_to_end.sym_norm_adj
  * loader       data/base_data.py instance_bpr_loader: (user, pos, neg) batches         -> DeviceTripleBatcher (BUIR
                 unpacks the negatives and never uses them, buir.py:226-228)
  * epoch        models/buir.py:235-250 train_an_epoch                                   -> BUIREngine.train_an_epoch
  * ranking      models/buir.py:79-100 predict over every item                           -> recommend() on
                 ranking_factors(): [p(P_u), P_u] . [P_i, p(P_i)]
The data is synthetic with planted structure (siblings_end_to_end.planted_interactions), leave-one-out.  Prints one JSON
line per epoch and checks that the mean batch loss falls; the top-K lists exclude the training items.

``--update-target`` turns on the moving target (buir.py:48-54, which the reference defines and never calls).

tests/test_buir_example_gpu.py runs the small default.
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

from sgl_end_to_end import dataset, sym_norm_adj  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=300)
    ap.add_argument("--items", type=int, default=200)
    ap.add_argument("--interactions", type=int, default=6000)
    ap.add_argument("--emb-dim", type=int, default=32)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--momentum", type=float, default=0.995)
    ap.add_argument("--update-target", action="store_true")
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--lr", type=float, default=0.005)
    ap.add_argument("--topk", type=int, default=10)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    import beta_recsys_amd as hp

    tr_u, tr_i, te_u, te_i = dataset(args.users, args.items, args.interactions)
    adj = sym_norm_adj(args.users, args.items, tr_u, tr_i)
    torch.manual_seed(0)
    model = dict(n_users=args.users, n_items=args.items, emb_dim=args.emb_dim, n_layers=args.layers,
                 momentum=args.momentum, update_target=args.update_target, norm_adj=adj, optimizer="adam", lr=args.lr,
                 device_str="cuda:0", batch_size=args.batch_size)
    with contextlib.redirect_stdout(io.StringIO()):
        eng = hp.BUIREngine({"model": model, "system": {"run_dir": "/tmp/hiprec_example_runs"}})
    users_d, items_d = torch.from_numpy(tr_u).cuda(), torch.from_numpy(tr_i).cuda()
    history = []
    for epoch in range(args.epochs):
        neg = torch.randint(0, args.items, (tr_u.size,), device="cuda")
        loader = hp.DeviceTripleBatcher(users_d, items_d, neg, args.batch_size)
        with contextlib.redirect_stdout(io.StringIO()):
            eng.train_an_epoch(loader, epoch)
        loss = [v for t, v, _ in eng.writer.scalars if t == "model/loss"][-1] / len(loader)
        rec = {"model": "buir", "epoch": epoch, "loss": loss}
        history.append(rec)
        print(json.dumps(rec), flush=True)
    if not history[-1]["loss"] < history[0]["loss"]:
        raise SystemExit(f"the loss did not fall: {[h['loss'] for h in history]}")
    # top-K over the whole catalogue through ranking_factors, the training items excluded
    query = np.arange(args.users)
    top, _ = eng.recommend(query, args.topk, seen=(tr_u, tr_i))
    top = top.cpu().numpy()
    held = {int(u): int(i) for u, i in zip(te_u, te_i)}
    hits = sum(int(held[u] in top[u]) for u in held)
    print(json.dumps({"model": "buir", "recommended_user0": [int(i) for i in top[0]], "users": int(query.size),
                      "held_out": len(held), f"hit@{args.topk}": hits / max(len(held), 1)}))
    return history, top, (tr_u, tr_i)


if __name__ == "__main__":
    main()
