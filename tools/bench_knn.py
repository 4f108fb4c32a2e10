"""Measure ItemKNN / UserKNN on the GPU at a MovieLens-1M-like shape, next to the reference's op sequence on the host.

    python tools/bench_knn.py [--iters 3] [--warmup 1] [--repeats 3] [--out profiles/knn.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o knn -- python tools/bench_knn.py --hip-only --repeats 1
    python tools/bench_knn.py --kernel-stats DIR/knn_kernel_stats.csv --out profiles/knn.json      # + that trace's kernel times

Shape: 6040 users x 3706 items, about 1 M pairs (per-user counts log-normal around ML-1M's mean of 166, items drawn
from a Zipf(1.0) popularity without replacement; 1 % of the pairs occur twice), ``neighbourhood_size`` 100, 4096 query
users, lists of 10, the training rows masked.

Device side (a window is ``--iters`` calls between two device synchronisations, ``--repeats`` windows):
  * ``prepare_model``   ItemKNN: both CSRs (torch) + the [3706, 3706] similarity matrix; UserKNN: both CSRs
  * ``recommend``       4096 users, k = 10, seen = the training CSR (includes the read-back of the status word)
and the peak device memory of each (torch.cuda.max_memory_allocated, reset before the window).

Host side, the yardstick: the reference's op sequence on scipy, restated here -- ``getcol(i).nonzero()[0]`` /
``get_sparse_vector`` / ``B.T.dot`` / the masked divide per item for ``generate_item_sim_matrix``; per query user
``similarity_with_users``, ``top_k`` (argpartition), ``get_sparse_vector``, ``B.T.dot``, the -inf mask (UserKNN) or the
row-by-row ``np.add`` over the similarity matrix (ItemKNN), each followed by an argpartition for the 10 best.  It is
timed on a SAMPLE of ``--host-sample`` rows and scaled to the full count (``*_extrapolated_s``: an extrapolation, named as
one); the sequence is fed the user's items (see beta_recsys_amd/knn.py on the reference's ``nonzero()[0]``).
The sampled rows are also compared: the device's similarity rows bit for bit, the device's lists against the host's.
Needs a GPU: there is no CPU timing path for the device side.
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_USERS, N_ITEMS, MEAN_LEN, K_NEIGH, N_QUERY, TOP = 6040, 3706, 166, 100, 4096, 10


def synthetic_log(seed=5):
    rng = np.random.default_rng(seed)
    counts = np.clip(rng.lognormal(np.log(MEAN_LEN) - 0.5, 1.0, N_USERS).astype(np.int64), 20, 2300)
    pop = 1.0 / np.arange(1, N_ITEMS + 1)
    pop = (pop / pop.sum())[rng.permutation(N_ITEMS)]
    users = np.repeat(np.arange(N_USERS), counts)
    items = np.concatenate([rng.choice(N_ITEMS, size=n, replace=False, p=pop) for n in counts])
    dup = rng.random(users.size) < 0.01
    users, items = np.concatenate([users, users[dup]]), np.concatenate([items, items[dup]])
    perm = rng.permutation(users.size)
    return users[perm].astype(np.int64), items[perm].astype(np.int64)


# ---- the reference's op sequence on scipy (models/itemKNN.py, models/userKNN.py)
def get_sparse_vector(ids, length, values=None):
    import scipy.sparse as ssp

    n = len(ids)
    return ssp.coo_matrix((np.ones(n) if values is None else values, (ids, np.zeros(n))), (length, 1)).tocsc()


def host_item_sim_row(B, cnt, item):
    seq = B.getcol(item).nonzero()[0]
    overlap = B.T.dot(get_sparse_vector(seq, B.shape[0])).toarray().ravel()
    overlap[overlap != 0] /= np.sqrt(cnt[overlap != 0])
    return overlap.astype(np.float32)


def host_user_scores(B, cu, user, k):
    seq = B.getrow(user).nonzero()[1]
    sim = B.dot(get_sparse_vector(seq, B.shape[1])).toarray().ravel()
    sim[sim != 0] /= np.sqrt(cu[sim != 0])
    nn = list(np.argpartition(-sim, range(k))[:k])
    scores = B.T.dot(get_sparse_vector(nn, B.shape[0], values=sim[nn])).toarray().ravel()
    scores[seq] = -np.inf
    return scores, seq


def host_item_scores(B, S, user):
    seq = B.getrow(user).nonzero()[1]
    acc = None
    for item in seq:
        acc = S[item] if acc is None else np.add(acc, S[item])
    return (np.zeros(B.shape[1], dtype=np.float32) if acc is None else acc), seq


def host_top(scores, seen, k):
    s = scores.copy()
    s[seen] = -np.inf
    return np.argpartition(-s, range(k))[:k]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=48)
    ap.add_argument("--hip-only", action="store_true", help="skip the host side (for a kernel-trace run)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 *_kernel_stats.csv of a --hip-only run: its knn "
                    "kernels' calls and mean time are added to the result")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_knn.py measures on the GPU; no GPU found and there is no CPU timing path")
    import scipy.sparse as ssp

    import __graft_entry__
    import beta_recsys_amd as hp

    dev = torch.device("cuda:0")
    users, items = synthetic_log()
    users_d, items_d = torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev)
    rng = np.random.default_rng(6)
    query = rng.choice(N_USERS, N_QUERY, replace=False)
    query_d = torch.from_numpy(query).to(dev)
    cfg = dict(n_users=N_USERS, n_items=N_ITEMS, neighbourhood_size=K_NEIGH, device_str="cuda:0")
    result = {"tool": "tools/bench_knn.py", "device": torch.cuda.get_device_name(0),
              "source_hash": __graft_entry__.source_hash(), "n_users": N_USERS, "n_items": N_ITEMS,
              "n_pairs": int(users.size), "neighbourhood_size": K_NEIGH, "n_query": N_QUERY, "top": TOP,
              "iters_per_window": args.iters, "repeats": args.repeats}

    def windows(fn):
        for _ in range(args.warmup):
            fn()
        out = []
        torch.cuda.reset_peak_memory_stats(dev)
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / args.iters * 1e3)
        return {"ms": [round(x, 4) for x in out], "ms_median": round(float(np.median(out)), 4),
                "ms_spread": round(max(out) - min(out), 4),
                "peak_device_bytes": int(torch.cuda.max_memory_allocated(dev))}

    models = {}
    for name, cls in (("itemknn", hp.ItemKNN), ("userknn", hp.UserKNN)):
        model = cls(cfg)
        result[f"{name}_prepare_model"] = windows(lambda: model.prepare_model((users_d, items_d)))
        seen = model.seen_csr()
        result[f"{name}_recommend"] = windows(lambda: model.recommend(query_d, TOP, seen))
        models[name] = model
        print(json.dumps({k: v for k, v in result.items() if k.startswith(name)}), flush=True)

    if not args.hip_only:
        B = ssp.coo_matrix((np.ones(users.size), (users, items)), shape=(N_USERS, N_ITEMS)).tocsr()
        cnt, cu = np.asarray(B.sum(axis=0)).ravel(), np.asarray(B.sum(axis=1)).ravel()
        n = args.host_sample
        S_dev = models["itemknn"].item_sim_matrix.cpu().numpy()
        sample_items = rng.choice(N_ITEMS, n, replace=False)
        t0 = time.perf_counter()
        rows = [host_item_sim_row(B, cnt, int(i)) for i in sample_items]
        t_sim = time.perf_counter() - t0
        sim_equal = sum(int(r.tobytes() == S_dev[i].tobytes()) for r, i in zip(rows, sample_items))
        sample_q = np.arange(n)                      # positions in the query list
        rec = {k: m.recommend(query_d[:n], TOP, m.seen_csr())[0].cpu().numpy() for k, m in models.items()}
        t0 = time.perf_counter()
        host_user = [host_top(*host_user_scores(B, cu, int(query[q]), K_NEIGH), TOP) for q in sample_q]
        t_user = time.perf_counter() - t0
        t0 = time.perf_counter()
        host_item = [host_top(*host_item_scores(B, S_dev, int(query[q])), TOP) for q in sample_q]
        t_item = time.perf_counter() - t0
        same = lambda got, want: float(np.mean([len(set(a) & set(b)) / TOP for a, b in zip(got, want)]))  # noqa: E731
        result["host"] = {
            "what": "the reference's op sequence on scipy, restated in this tool, timed on a sample and scaled",
            "sample_rows": n,
            "item_sim_sample_s": round(t_sim, 4), "item_sim_extrapolated_s": round(t_sim / n * N_ITEMS, 2),
            "userknn_recommend_sample_s": round(t_user, 4),
            "userknn_recommend_extrapolated_s": round(t_user / n * N_QUERY, 2),
            "itemknn_recommend_sample_s": round(t_item, 4),
            "itemknn_recommend_extrapolated_s": round(t_item / n * N_QUERY, 2),
            "item_sim_rows_bit_equal": f"{sim_equal}/{n}",
            "userknn_list_overlap_with_host": round(same(rec["userknn"], host_user), 4),
            "itemknn_list_overlap_with_host": round(same(rec["itemknn"], host_item), 4)}
        h = result["host"]
        result["ratio_host_extrapolated_over_device"] = {
            "itemknn_prepare_model": round(h["item_sim_extrapolated_s"] * 1e3 / result["itemknn_prepare_model"]["ms_median"], 1),
            "userknn_recommend": round(h["userknn_recommend_extrapolated_s"] * 1e3 / result["userknn_recommend"]["ms_median"], 1),
            "itemknn_recommend": round(h["itemknn_recommend_extrapolated_s"] * 1e3 / result["itemknn_recommend"]["ms_median"], 1)}
        print(json.dumps(result["host"]), flush=True)
        print(json.dumps(result["ratio_host_extrapolated_over_device"]), flush=True)
    if args.kernel_stats:
        import csv

        with open(args.kernel_stats) as f:
            result["kernel_trace"] = {
                "what": "rocprofv3 --kernel-trace --stats of a separate --hip-only run of this tool",
                "kernels": {re.search(r"knn_\w+(<\w+>)?", row["Name"]).group(0): {
                    "calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 1)}
                    for row in csv.DictReader(f) if "knn_" in row["Name"]}}
        print(json.dumps(result["kernel_trace"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
