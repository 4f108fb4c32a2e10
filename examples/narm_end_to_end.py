"""NARM end to end on a synthetic session log: sessions -> ``data.session_prefixes`` -> ``data.SessionLoader`` -> epochs
of ``NARMEngine.train_an_epoch`` -> ``recommend_next`` -> hit-rate@10 on each session's held-out last item.

    python examples/narm_end_to_end.py                          # 2000 sessions, 1682 items, 12 epochs
    python examples/narm_end_to_end.py --sessions 300 --items 200 --epochs 4

The log is a noisy walk: a session's next item is the previous one plus a small step (mod the catalogue) four times out
of five and a uniformly random item otherwise, so the next item is predictable from the last one.  Every session's last
item is held out; the rest is cut into (prefix, next item) pairs as the reference does.  Prints one JSON line with the
mean loss per epoch (as ``train_an_epoch`` returns it), the hit rate of the trained model, that of the untrained model
and the 10 / n_items of a random ranking.
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


def synthetic_sessions(n_sessions, n_items, min_len, max_len, seed):
    """Lists of item ids in 1 .. n_items - 1 (0 is the padding id, which ``n_items`` counts)."""
    rng = np.random.default_rng(seed)
    real = n_items - 1
    out = []
    for _ in range(n_sessions):
        n = int(rng.integers(min_len, max_len + 1))
        items = [int(rng.integers(1, real + 1))]
        while len(items) < n:
            if rng.random() < 0.8:
                nxt = (items[-1] - 1 + int(rng.integers(1, 4))) % real + 1
            else:
                nxt = int(rng.integers(1, real + 1))
            items.append(nxt)
        out.append(items)
    return out


def hit_rate(engine, sessions, top):
    profiles = [s[:-1] for s in sessions]
    held_out = np.array([s[-1] for s in sessions])
    items, _ = engine.recommend_next(profiles, top)
    return float((items.cpu().numpy() == held_out[:, None]).any(1).mean())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sessions", type=int, default=2000)
    ap.add_argument("--items", type=int, default=1682)
    ap.add_argument("--max-len", type=int, default=19)
    ap.add_argument("--emb-dim", type=int, default=50)
    ap.add_argument("--hidden", type=int, default=100)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--batch-size", type=int, default=512)
    ap.add_argument("--dropout-input", type=float, default=0.25)
    ap.add_argument("--dropout-hidden", type=float, default=0.5)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--lr-dc-step", type=int, default=80)
    ap.add_argument("--lr-dc", type=float, default=0.1)
    ap.add_argument("--epochs", type=int, default=12)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    import torch

    import beta_recsys_amd as hp
    from beta_recsys_amd.data import SessionLoader, session_prefixes

    torch.manual_seed(args.seed)
    sessions = synthetic_sessions(args.sessions, args.items, 3, args.max_len, args.seed)
    out_seqs, labels = session_prefixes([s[:-1] for s in sessions])
    loader = SessionLoader(out_seqs, labels, args.batch_size)
    config = {"dataset": {"n_items": args.items},
              "model": {"hidden_size": args.hidden, "n_layers": args.layers, "embedding_dim": args.emb_dim,
                        "dropout_input": args.dropout_input, "dropout_hidden": args.dropout_hidden,
                        "batch_size": args.batch_size, "optimizer": "adam", "lr": args.lr,
                        "lr_dc_step": args.lr_dc_step, "lr_dc": args.lr_dc, "device_str": "cuda:0",
                        "dropout_rng": "device", "dropout_seed": args.seed},
              "system": {"run_dir": "/tmp/hiprec_narm_example"}}
    with contextlib.redirect_stdout(io.StringIO()):
        engine = hp.NARMEngine(config)
    untrained = hit_rate(engine, sessions, args.top)
    losses = []
    for epoch in range(args.epochs):
        with contextlib.redirect_stdout(io.StringIO()):
            losses.append(float(engine.train_an_epoch(loader, epoch)))
    trained = hit_rate(engine, sessions, args.top)
    print(json.dumps({"sessions": args.sessions, "pairs": len(out_seqs), "steps_per_epoch": len(loader),
                      "mean_loss_per_epoch": losses, f"hit_rate@{args.top}": trained,
                      f"untrained_hit_rate@{args.top}": untrained, "random_ranking": args.top / (args.items - 1)}))


if __name__ == "__main__":
    main()
