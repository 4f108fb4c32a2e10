"""The synthetic VBCAR inputs the GPU edge tests run against the fp64 restatement (tests/vbcar_numpy.py), the recipe that
keeps the KL term well conditioned, and the inputs the host-side visibility checks reuse.  Each shape is
``(U, I, D, L, Fu, Fi, B, n_neg, activator, alpha, config batch_size)``.

Which constant of csrc/vbcar.hip / csrc/ncf.hip each value straddles:

* the loss stage's two columns per lane (``kVbNpl``, D <= 64 / D > 64) and its limit D = 128; D = 3 and 17 leave most
  lanes idle, D = 64 fills exactly one column per lane;
* the grouped GEMM's 64 x 64 tiles with a K tile of 32: rows 30 / 60 (inside a tile), 33 / 66 (one past 32 and 64),
  99 / 198 (several tiles); L = 33 and F = 65 one past a tile in every width; L = 512 the limit;
* the gather's float4 path (F a multiple of 4) and its scalar path (F = 1, 2, 5, 7, 65, 1030), F = 1030 also more than
  one trip of a wave over a row;
* one wave per triple, four per block: B = 2 (half a block), 5, 11, 33 (nine blocks, the last with one wave);
* a short batch (B = 3 with config batch_size 8): ``scale`` comes from the config;
* U = 1: every user gradient lands in one table row (32 adders on one row).

Every batch leaves the last user and the last item out (their gradient rows stay exactly zero) and (B >= 2) holds a user
twice as ``pos_u``, a triple with ``pos_i_1 == pos_i_2``, a negative equal to its own triple's positive and a repeated
negative within one row.
"""
import numpy as np

import vbcar_numpy as vn

SHAPES = [
    (2, 2, 3, 2, 1, 2, 2, 1, "none", 0.3, 2),
    (12, 15, 64, 256, 512, 512, 5, 5, "tanh", 0.001, 256),
    (9, 11, 17, 33, 65, 65, 11, 2, "lrelu", 0.3, 11),
    (6, 6, 128, 512, 64, 64, 33, 2, "sigmoid", 0.3, 33),
    (9, 11, 8, 16, 16, 16, 3, 4, "relu", 0.5, 8),
    (1, 3, 4, 4, 4, 4, 4, 3, "tanh", 0.3, 4),
    # each limit on its own
    (5, 7, 128, 8, 4, 4, 3, 2, "tanh", 0.3, 3),
    (5, 7, 4, 512, 4, 4, 3, 2, "relu", 0.3, 3),
    (5, 7, 4, 8, 1030, 3, 3, 2, "lrelu", 0.3, 3),
]
MIN_ABS_S = 0.25


def shape_id(shape):
    U, I, D, L, Fu, Fi, B, n_neg, activator, alpha, bs = shape
    return f"U{U}-I{I}-D{D}-L{L}-F{Fu}x{Fi}-B{B}of{bs}-n{n_neg}-{activator}"


def condition(w):
    """The conditioning recipe, in place: the KL term is ``-log(s^2 + 1e-10)`` of a raw linear output, so ``s`` is kept
    away from 0 -- the second half of both ``fc_*_2_mu.bias`` becomes +-0.5 (alternating by column) and every
    second-half row of both ``fc_*_2_mu.weight`` is scaled to an absolute row sum of at most 0.25."""
    for side in ("u", "i"):
        W, b = w[f"fc_{side}_2_mu.weight"], w[f"fc_{side}_2_mu.bias"]
        D = b.shape[0] // 2
        b[D:] = np.where(np.arange(D) % 2 == 0, 0.5, -0.5).astype(b.dtype)
        rows = np.abs(W[D:]).sum(1, keepdims=True)
        W[D:] *= np.minimum(1.0, 0.25 / np.maximum(rows, 1e-30)).astype(W.dtype)
    return w


def make_batch(rng, U, I, B, n_neg):
    """Ids with every collision a kernel can get wrong (see the module docstring).  The last user and the last item
    (where there are two or more) are never drawn: their gradient rows must stay exactly zero."""
    nu, ni = max(1, U - 1), max(1, I - 1)
    pos_u, pos_1, pos_2 = rng.integers(0, nu, B), rng.integers(0, ni, B), rng.integers(0, ni, B)
    neg_u, neg_1, neg_2 = (rng.integers(0, n, (B, n_neg)) for n in (nu, ni, ni))
    if B >= 2:
        pos_u[1] = pos_u[0]
        pos_2[0] = pos_1[0]
        neg_1[1, 0] = pos_1[1]
        neg_u[0, 0] = pos_u[0]
        if n_neg >= 2:
            neg_2[B - 1, 1] = neg_2[B - 1, 0]
    return pos_u, pos_1, pos_2, neg_u, neg_1, neg_2


def check_batch(batch):
    pos_u, pos_1, pos_2, neg_u, neg_1, neg_2 = batch
    B, n_neg = neg_u.shape
    assert len(set(pos_u.tolist())) < B, "no user occurs twice as pos_u"
    assert (pos_1 == pos_2).any(), "no triple with pos_i_1 == pos_i_2"
    assert (neg_1 == pos_1[:, None]).any() or (neg_2 == pos_2[:, None]).any() or (neg_u == pos_u[:, None]).any(), \
        "no negative equals its own triple's positive"
    assert set(np.concatenate([pos_u, neg_u.ravel()]).tolist()) & set(
        np.concatenate([pos_1, pos_2, neg_1.ravel(), neg_2.ravel()]).tolist()), "no id is both a user and an item row"
    if n_neg >= 2:
        assert any(len(set(r.tolist())) < n_neg for a in (neg_u, neg_1, neg_2) for r in a), "no repeated negative in a row"


def draw_eps(rng, B, n_neg, D):
    return [rng.standard_normal((n, D)).astype(np.float32) for n in (B, B, B, B * n_neg, B * n_neg, B * n_neg)]


def synthetic(shape, seed=0):
    """``(weights, (user_fea, item_fea), batch, eps)`` for a shape; the same seed gives the same inputs everywhere.
    The weights follow the reference's constructor (N(0, 1) users, uniform items, ``nn.Linear``'s uniform bounds) and
    then :func:`condition`."""
    U, I, D, L, Fu, Fi, B, n_neg, activator, alpha, bs = shape
    rng = np.random.default_rng(seed + 1000 * U + 10 * L + D + Fu)
    w = {}
    for k, s in vn.shapes(U, I, D, L, Fu, Fi).items():
        if k == "user_emb.weight":
            w[k] = rng.standard_normal(s).astype(np.float32)
        elif k == "item_emb.weight":
            w[k] = rng.uniform(-0.1 * D ** -0.5, 0.1 * D ** -0.5, s).astype(np.float32)
        else:
            fan_in = {"fc_u_1_mu": Fu, "fc_i_1_mu": Fi}.get(k.split(".")[0], L)
            w[k] = rng.uniform(-fan_in ** -0.5, fan_in ** -0.5, s).astype(np.float32)
    condition(w)
    fea = (rng.standard_normal((U, Fu)).astype(np.float32), rng.standard_normal((I, Fi)).astype(np.float32))
    batch = make_batch(rng, U, I, B, n_neg)
    return w, fea, batch, draw_eps(rng, B, n_neg, D)


def hyper(shape):
    """``(activator, alpha, scale)``."""
    return shape[8], shape[9], 1.0 / (3 * shape[10])
