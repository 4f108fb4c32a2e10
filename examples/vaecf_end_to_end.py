"""VAECF (Mult-VAE) end to end on a synthetic frame: interactions -> ``data.instance_vae_loader`` -> epochs of
``VAECFEngine.train_an_epoch`` -> ``engine.recommend`` over the whole catalogue -> hit-rate@10 on each user's held-out
item.  Needs an MI355X (there is no CPU path).

    python examples/vaecf_end_to_end.py                          # 2000 users, 1500 items, 12 epochs
    python examples/vaecf_end_to_end.py --users 300 --items 200 --epochs 8

The users fall into ``--groups`` taste groups; a user's items come from the group's block of the catalogue nine times
out of ten.  One item per user is held out; the model never sees it, and ``recommend`` masks the items it has seen.
Prints one JSON line: the loss of every epoch, the hit rate and what a random ranking would score.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def synthetic_frame(n_users, n_items, groups, per_user, seed):
    """``(train_users, train_items, held_out[n_users])``: distinct items per user, the last one held out."""
    rng = np.random.default_rng(seed)
    block = n_items // groups
    users, items, held = [], [], np.empty(n_users, dtype=np.int64)
    for u in range(n_users):
        g = u % groups
        own = rng.choice(np.arange(g * block, (g + 1) * block), size=min(per_user, block - 1), replace=False)
        n_far = max(1, per_user // 10)
        far = rng.choice(n_items, size=n_far, replace=False)
        row = np.unique(np.concatenate([own, far]))
        held[u] = rng.choice(own)
        row = row[row != held[u]]
        users.append(np.full(len(row), u)), items.append(row)
    return np.concatenate(users), np.concatenate(items), held


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=2000)
    ap.add_argument("--items", type=int, default=1500)
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--per-user", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=500)
    ap.add_argument("--epochs", type=int, default=12)
    ap.add_argument("--lr", type=float, default=0.02)
    ap.add_argument("--beta", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()

    import torch

    import beta_recsys_amd as hp

    if not torch.cuda.is_available():
        raise SystemExit("examples/vaecf_end_to_end.py trains on the GPU; no GPU found and there is no CPU path")
    torch.manual_seed(args.seed)
    train_u, train_i, held = synthetic_frame(args.users, args.items, args.groups, args.per_user, args.seed)
    loader = hp.data.instance_vae_loader(train_u, train_i, args.users, args.items)
    config = {"model": {"n_users": args.users, "n_items": args.items, "activation": "tanh", "likelihood": "mult",
                        "batch_size": args.batch_size, "lr": args.lr, "beta": args.beta, "weight_decay": 0.0,
                        "optimizer": "adam", "device_str": "cuda:0", "noise_rng": "device"},
              "system": {"run_dir": "/tmp/hiprec_vaecf_example"}}
    with contextlib.redirect_stdout(io.StringIO()):
        engine = hp.VAECFEngine(config)
    k = 10
    users = np.arange(args.users)

    def hit_rate():
        rec, _ = engine.recommend(users, k, seen=(train_u, train_i))
        return float((rec.cpu().numpy() == held[:, None]).any(1).mean())

    engine.model.set_history(loader[1])
    untrained = hit_rate()
    losses = []
    for epoch in range(args.epochs):
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            engine.train_an_epoch(loader, epoch)
        losses.append(float(out.getvalue().strip().rsplit("Loss ", 1)[1]))
    seen_per_user = len(train_u) / args.users
    print(json.dumps({"users": args.users, "items": args.items, "interactions": int(len(train_u)),
                      "steps_per_epoch": -(-len(loader[0]) // args.batch_size), "loss_per_epoch": losses,
                      "untrained_hit_rate@10": untrained, "hit_rate@10": hit_rate(),
                      "chance_hit_rate@10": k / (args.items - seen_per_user)}))


if __name__ == "__main__":
    main()
