"""Edge cases of the MixGCF sampler / loss / scatter kernel (csrc/mixgcf.hip) and the two rules they are held to.  No
goldens: the fp64 restatement (tests/mixgcf_numpy.py) is the yardstick, on the smallest shapes at which the kernel can go
wrong -- every row width at which the columns-per-lane or tail-lane handling changes (1, 7, 64, 65, 128, 200, 256), one
hop, the register forms' seam (L = 3 | 4 tables) and the limit (L = 6), one and two candidates and one more than a wave's
worth (64, 65), K = 1 and 4, batches that four waves per block do not divide (1, 5, 257).

Every graph has a hub item (item 0, linked to every user) and items without edges (the last three: their hop rows beyond
hop 0 are their own row scaled down); wherever a row has two or more candidates, its first two are the hub and an
edgeless item.

Rule for the choice (nothing is left out): for every (row, k, hop) the candidate j* the implementation chose must have an
fp64 score within 2 * bound of the fp64 maximum, bound = (D + L + 6) * 2^-24 * sum_d |s_d| (|seed p_d| + |(1 - seed) n_d|)
-- the worst case of an fp32 mix, of a pooled s of L + 1 terms and of a D-term dot product in any order -- taken at the
larger of the two candidates compared.  Where two candidates are one item, either index passes.
Gradients and loss are then held to ``mix_grads(..., choice=that choice)`` in fp64 at REL of scale.
"""
import numpy as np

import mixgcf_numpy as mx
from helpers import REL, assert_scalar_close, assert_tensor_close, float64_oracle, to64

MAX_L = 6

#        name            D   L  n_negs K  B    pool      extras
CASES = [
    ("d1",               1,  1, 1,  1, 1,   "concat", {}),
    ("d7_k4",            7,  3, 2,  4, 5,   "mean",   {}),
    ("d64_n64",          64, 3, 64, 1, 5,   "concat", {}),
    ("d65_n65",          65, 1, 65, 1, 5,   "sum",    {}),
    ("d128_lmax_final",  128, MAX_L, 2, 4, 5, "final", {}),
    ("d200_b257",        200, 3, 2,  1, 257, "concat", {}),
    ("d256_lmax_k4",     256, MAX_L, 2, 4, 5, "concat", {}),
    ("d256_l1_mean",     256, 1, 2,  1, 5,   "mean",   {}),
    ("one_user_b257",    64, 3, 2,  1, 257, "sum",    {"one_user": True}),
    ("same_item_row",    20, 3, 5,  2, 5,   "concat", {"same_item": True}),
    ("cand_is_pos",      20, 4, 3,  1, 5,   "mean",   {"cand_is_pos": True}),
    ("dropout_b257",     65, 3, 2,  4, 257, "concat", {"edge_rate": 0.5, "mess_rate": 0.1}),
    ("rns_lmax",         7,  MAX_L, 1, 4, 5, "final", {"ns": "rns"}),
]
CASE_NAMES = [c[0] for c in CASES]


def make_case(name):
    """dict(w, graph, hp, batch, seeds, masks, U, I) of one edge case, seeded by its position in CASES."""
    idx = CASE_NAMES.index(name)
    _, D, L, n_negs, K, B, pool, extra = CASES[idx]
    rng = np.random.default_rng(100 + idx)
    U, I = 23, 19
    N, H = U + I, L + 1
    pairs = {(u, 0) for u in range(U)}                                  # the hub
    for u in range(U):
        for i in rng.choice(np.arange(1, I - 3), size=3, replace=False):  # items I-3 .. I-1 keep no edges
            pairs.add((u, int(i)))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    eu, ei = pairs[:, 0], pairs[:, 1]
    rows = np.concatenate([eu, U + ei, np.arange(N)])
    cols = np.concatenate([U + ei, eu, np.arange(N)])
    vals = (1.0 / np.bincount(rows, minlength=N)[rows]).astype(np.float32)
    perm = rng.permutation(rows.size)
    graph = (rows[perm], cols[perm], vals[perm], N)
    scale = 1.6 / D ** 0.25                                             # |x_k| of a few units at every width
    w = {"user_embedding.weight": (rng.standard_normal((U, D)) * scale).astype(np.float32),
         "item_embedding.weight": (rng.standard_normal((I, D)) * scale).astype(np.float32)}
    ns = extra.get("ns", "mixgcf")
    M = K if ns == "rns" else K * n_negs
    users = rng.integers(0, U, B)
    if extra.get("one_user"):
        users[:] = 7
    pos = rng.integers(0, I, B)
    neg = rng.integers(0, I, (B, M))
    if ns != "rns" and n_negs >= 2:
        neg[:, 0::n_negs] = 0                                           # the hub
        neg[:, 1::n_negs] = I - 1 - (np.arange(B) % 3)[:, None]         # an item without edges
    if extra.get("same_item"):
        neg[B // 2, :] = 5
    if extra.get("cand_is_pos"):
        neg[:, -1] = pos
    seeds = rng.random((B, K, H)).astype(np.float32)
    hp = dict(pool=pool, L=L, n_negs=n_negs, K=K, ns=ns, l2=1e-3, edge_rate=extra.get("edge_rate"),
              mess_rate=extra.get("mess_rate"))
    # whatever the pool and the depth do to the size of a score: the batch's largest |s_pos| is 6, so that no softplus
    # saturates and every row's gradient shows
    f = np.float32(np.sqrt(6.0 / np.abs(mx.mix_predict(w, graph, hp, users, pos)).max()))
    w = {k: v * f for k, v in w.items()}
    edge = [(rng.random(rows.size) < hp["edge_rate"]).astype(np.uint8) for _ in range(L)] if hp["edge_rate"] else None
    mess = [(rng.random((N, D)) >= hp["mess_rate"]).astype(np.uint8) for _ in range(L)] if hp["mess_rate"] else None
    return dict(name=name, w=w, graph=graph, hp=hp, batch=(users, pos, neg), seeds=seeds, masks=(edge, mess), U=U, I=I, D=D,
                L=L, B=B, K=K)


def exact_scores(case):
    """fp64: ``(scores [B, K, n, H], bound [B, K, n, H], cand [B, K, n])`` of the choice rule."""
    hp, (users, pos, neg) = case["hp"], case["batch"]
    D, L = case["D"], case["L"]
    with float64_oracle(mx):
        E, _, _ = mx.propagate(to64(case["w"]), case["graph"], hp, case["masks"])
        cand = mx.candidates(neg, hp)
        sd = None if hp["ns"] == "rns" else case["seeds"].astype(np.float64)
        sc = mx.sampler_scores(E, case["U"], users, pos, cand, sd, hp["pool"])
        Et = np.transpose(E, (1, 0, 2))
        s_e = Et[users]
        if hp["pool"] != "concat":
            s_e = np.repeat(mx.pooling(s_e, hp["pool"])[:, None, :], L + 1, axis=1)
        p_e, n_e = Et[case["U"] + pos], Et[case["U"] + cand]              # [B, H, D], [B, K, n, H, D]
        sdx = np.zeros(cand.shape[:2] + (1, L + 1, 1)) if sd is None else sd[:, :, None, :, None]
        mag = np.abs(sdx * p_e[:, None, None]) + np.abs((1 - sdx) * n_e)
        bound = (D + L + 6) * 2.0 ** -24 * (np.abs(s_e)[:, None, None] * mag).sum(axis=-1)
    return sc, bound, cand


def check_choice(case, choice, what=""):
    """The rule for the choice; returns how many (row, k, hop) differ from the fp64 argmax (all of them near ties)."""
    sc, bound, cand = exact_scores(case)
    choice = np.asarray(choice, dtype=np.int64)
    B, K, n, H = sc.shape
    assert choice.shape == (B, K, H), f"{what}: choice is {choice.shape}"
    assert choice.min() >= 0 and choice.max() < n, f"{what}: a choice outside its candidates"
    best_j = sc.argmax(axis=2)
    pick = lambda a, j: np.take_along_axis(a, j[:, :, None, :], axis=2)[:, :, 0, :]   # noqa: E731
    short = pick(sc, best_j) - pick(sc, choice)
    room = 2 * np.maximum(pick(bound, best_j), pick(bound, choice))
    same_item = pick(np.broadcast_to(cand[..., None], sc.shape), best_j) == pick(np.broadcast_to(cand[..., None], sc.shape), choice)
    bad = (short > room) & ~same_item
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} choices are not the maximum; worst falls short by "
                           f"{short[bad].max():.3e} with room {room[bad][np.argmax(short[bad])]:.3e}")
    return int(((best_j != choice) & ~same_item).sum())


def check_step(case, loss, grads, choice, what=""):
    """Loss and gradients against the fp64 restatement under the implementation's own choice, at REL of scale."""
    with float64_oracle(mx):
        l64, g64, _ = mx.mix_grads(to64(case["w"]), case["graph"], case["hp"], case["batch"],
                                   case["seeds"].astype(np.float64), case["masks"], choice=choice)
    assert_scalar_close(loss, l64, REL, f"{what} loss")
    for k in mx.KEYS:
        assert_tensor_close(np.asarray(grads[k]).reshape(g64[k].shape), g64[k], REL, f"{what} grad {k}")
