"""VBCAR end to end on synthetic baskets: baskets -> (u, i1, i2) triples -> N(0, 1) side features -> alias samplers ->
epochs of ``VBCAREngine.train_an_epoch`` -> ``engine.recommend`` over the whole catalogue -> hit-rate@10 on each user's
held-out item.

    python examples/vbcar_end_to_end.py                          # 2000 users, 1500 items, 8 epochs
    python examples/vbcar_end_to_end.py --users 300 --items 200 --epochs 6

Users and items fall into groups; a basket holds items of its user's group nine times out of ten.  One item per user is
held out of every basket of that user; the rest of each basket gives the ordered pairs (i1, i2) of its items, as the
reference's grocery loaders make them.  The features are random (``get_random_rep``: N(0, 1), 512 wide), so what the
model learns sits in the encoder weights and the two tables.  Negatives come from frequency alias tables through
``engine.data.user_sampler`` / ``item_sampler``, as in the reference's epoch loop.  Prints one JSON line with the epoch
losses (``total_loss`` as ``train_an_epoch`` logs it), the hit rate of the trained model, that of the untrained model and
the 10 / n_items of a random ranking.
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


class AliasSampler:
    """utils/alias_table.py::AliasTable's ``sample(count, obj_num)`` over item (or user) frequencies, vectorised:
    ``[obj_num, count]`` ids."""

    def __init__(self, freq, seed):
        freq = np.asarray(freq, dtype=np.float64)
        n = len(freq)
        prob = n * freq / freq.sum()
        alias = np.arange(n, dtype=np.int64)
        small = [i for i in range(n) if prob[i] < 1.0]
        large = [i for i in range(n) if not prob[i] < 1.0]
        while small and large:
            s, l = small.pop(), large.pop()
            alias[s] = l
            prob[l] -= 1.0 - prob[s]
            (small if prob[l] < 1.0 else large).append(l)
        self.prob_arr, self.alias_arr, self.rng = prob, alias, np.random.default_rng(seed)

    def sample(self, count, obj_num):
        col = self.rng.integers(0, len(self.prob_arr), (obj_num, count))
        return np.where(self.rng.random((obj_num, count)) < self.prob_arr[col], col, self.alias_arr[col])


def synthetic_baskets(n_users, n_items, n_groups, baskets_per_user, seed):
    """``(triples [N, 3], held_out [n_users], seen (users, items))``: every user's held-out item is one of its own
    group's and occurs in none of its training baskets."""
    rng = np.random.default_rng(seed)
    by_group = [np.flatnonzero(np.arange(n_items) % n_groups == g) for g in range(n_groups)]
    triples, held_out, seen_u, seen_i = [], np.zeros(n_users, dtype=np.int64), [], []
    for u in range(n_users):
        own = by_group[u % n_groups]
        held_out[u] = rng.choice(own)
        for _ in range(baskets_per_user):
            size = int(rng.integers(2, 6))
            inside = rng.random(size) < 0.9
            basket = np.unique(np.where(inside, rng.choice(own, size), rng.integers(0, n_items, size)))
            basket = basket[basket != held_out[u]]
            for a in basket:
                seen_u.append(u), seen_i.append(int(a))
                for b in basket:
                    if a != b:
                        triples.append((u, int(a), int(b)))
    return np.asarray(triples, dtype=np.int64), held_out, (np.asarray(seen_u), np.asarray(seen_i))


def hit_rate(engine, held_out, seen, top):
    users = np.arange(len(held_out))
    items, _ = engine.recommend(users, top, seen=seen)
    return float((items.cpu().numpy() == held_out[:, None]).any(1).mean())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--users", type=int, default=2000)
    ap.add_argument("--items", type=int, default=1500)
    ap.add_argument("--groups", type=int, default=10)
    ap.add_argument("--baskets", type=int, default=6)
    ap.add_argument("--fea-dim", type=int, default=512)
    ap.add_argument("--emb-dim", type=int, default=64)
    ap.add_argument("--late-dim", type=int, default=256)
    ap.add_argument("--n-neg", type=int, default=5)
    ap.add_argument("--batch-size", type=int, default=256)
    ap.add_argument("--alpha", type=float, default=0.001)
    ap.add_argument("--lr", type=float, default=2e-3)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    import torch

    import beta_recsys_amd as hp

    if not torch.cuda.is_available():
        raise SystemExit("needs an MI355X (torch.cuda.is_available() is False)")
    torch.manual_seed(args.seed)
    U, I = args.users, args.items
    triples, held_out, seen = synthetic_baskets(U, I, args.groups, args.baskets, args.seed)
    rng = np.random.default_rng(args.seed + 1)
    config = {"model": {"n_users": U, "n_items": I, "late_dim": args.late_dim, "emb_dim": args.emb_dim,
                        "n_neg": args.n_neg, "batch_size": args.batch_size, "alpha": args.alpha, "activator": "tanh",
                        "optimizer": "rmsprop", "lr": args.lr, "device_str": "cuda:0", "noise_rng": "device"},
              "user_fea": rng.standard_normal((U, args.fea_dim)), "item_fea": rng.standard_normal((I, args.fea_dim)),
              "system": {"run_dir": "/tmp/hiprec_vbcar_example"}}
    with contextlib.redirect_stdout(io.StringIO()):
        engine = hp.VBCAREngine(config)
    engine.data = type("Data", (), {
        "user_sampler": AliasSampler(np.bincount(triples[:, 0], minlength=U) + 1.0, args.seed + 2),
        "item_sampler": AliasSampler(np.bincount(triples[:, 1], minlength=I) + 1.0, args.seed + 3)})()
    untrained = hit_rate(engine, held_out, seen, args.top)
    losses = []
    B = args.batch_size
    for epoch in range(args.epochs):
        shuffled = torch.from_numpy(triples[rng.permutation(len(triples))])
        loader = [shuffled[s:s + B] for s in range(0, len(shuffled), B) if len(shuffled) - s >= 2]
        with contextlib.redirect_stdout(io.StringIO()):
            engine.train_an_epoch(loader, epoch)
        logged = dict((tag, v) for tag, v, step in engine.writer.scalars[-3:] if step == epoch)
        losses.append(float(logged["model/loss/total_loss"]))
    trained = hit_rate(engine, held_out, seen, args.top)
    print(json.dumps({"users": U, "items": I, "triples": int(len(triples)), "steps_per_epoch": len(loader),
                      "total_loss_per_epoch": losses, f"hit_rate@{args.top}": trained,
                      f"untrained_hit_rate@{args.top}": untrained, "random_ranking": args.top / I}))


if __name__ == "__main__":
    main()
