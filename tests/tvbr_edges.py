"""The synthetic TVBR inputs the GPU edge tests run against the fp64 restatement (tests/tvbr_numpy.py), the recipe that
keeps the piecewise activators away from their kinks, and the inputs the host-side visibility checks reuse.  Each shape
is ``(U, I, D, T, Fu, Fi, B, n_neg, activator, alpha, config batch_size)`` and runs in two forms: ``mixed`` (every row
its own ``t``) and one ``t`` for the whole batch (what the epoch loop feeds).

Which constant of csrc/tvbr.hip / csrc/ncf.hip each shape straddles:

* ``(2, 2, 3, 1, 1, 2, ...)``: the smallest of everything -- ``T = 1`` (two time rows, both used by every row), ``F = 1``,
  ``K = D + T + 1 + F = 6`` inside one K tile of 32, ``B = 2`` half a block of the loss stage (one wave per triple, four
  per block);
* ``(12, 15, 64, 10, 512, 512, 5, 5, ...)``: the default config's widths -- ``D = 64`` fills exactly one column per lane
  (``kTvNpl`` = 2 columns at most), ``K = 587`` is no multiple of the K tile, 5 of 256 triples is a short batch;
* ``(9, 11, 17, 3, 65, 65, 11, 2, lrelu)``: ``D = 17`` leaves most lanes idle, 33 / 66 rows are one past 32 and 64 (the
  grouped GEMM's 64 x 64 tiles), ``K = 86`` one tile and a rest;
* ``(6, 6, 128, 4, 64, 64, 33, 2, sigmoid)``: ``D = 128`` the limit, two columns per lane; 99 / 198 rows are several GEMM
  tiles, four and seven blocks of the activation backward (``kTvBwdRows`` = 8 rows per wave at least, here 7 in groups
  of ``kTvBwdUnroll`` = 4 and a rest of 3): its wave seams, runs of equal ``t`` that end inside a wave, and the LDS merge
  of four waves that hold different ``t``;
* ``(9, 11, 8, 7, 16, 16, 3, 4, relu)``: a short batch (3 of 8: ``scale`` comes from the config) with an unused time row;
* ``(1, 3, 4, 2, 4, 4, 4, 3, hardtanh)``: ``U = 1``, every user-side table gradient lands in one row (16 adders);
* ``(5, 7, 4, 255, 4, 4, 3, 2, logsigmoid)``: ``time_step = 255`` the limit -- 256 time rows are four row tiles of the
  ``Tb`` GEMM and 256 x 4 blocks of the time-gradient kernel, of which only the rows the batch uses pass its zero-row
  test;
* ``(5, 7, 4, 2, 1030, 3, 3, 2, prelu)``: ``F = 1030`` more than one trip of a wave over a row in the gather and 33 K
  tiles; prelu's saved pre-activation and slope gradients.

Every batch leaves the last user and the last item out (their gradient rows stay exactly zero) and (B >= 2) holds a user
twice as ``pos_u``, a triple with ``pos_i_1 == pos_i_2``, a negative equal to its own triple's positive and a repeated
negative within one row.  A mixed batch also holds ``t = 0`` and ``t = time_step - 1`` and a negative whose ``t`` differs
from its triple's (where ``time_step >= 2``), and with ``time_step >= 4`` never uses time row 2 (no ``t`` is 1 or 2), whose
gradient row must stay exactly zero; with fewer time steps the two ends already use every row.  A one-``t`` batch sits at
``t = time_step - 1`` and leaves every time row below it unused.
"""
import numpy as np

import tvbr_numpy as tn

SHAPES = [
    (2, 2, 3, 1, 1, 2, 2, 1, "tanh", 0.3, 2),
    (12, 15, 64, 10, 512, 512, 5, 5, "tanh", 0.001, 256),
    (9, 11, 17, 3, 65, 65, 11, 2, "lrelu", 0.3, 11),
    (6, 6, 128, 4, 64, 64, 33, 2, "sigmoid", 0.3, 33),
    (9, 11, 8, 7, 16, 16, 3, 4, "relu", 0.5, 8),
    (1, 3, 4, 2, 4, 4, 4, 3, "hardtanh", 0.3, 4),
    (5, 7, 4, 255, 4, 4, 3, 2, "logsigmoid", 0.3, 3),
    (5, 7, 4, 2, 1030, 3, 3, 2, "prelu", 0.3, 3),
]
MIN_KINK_GAP = 0.2      # asserted in fp64 at every step; the recipe gives 0.25, the slack is for three optimizer steps


def shape_id(shape):
    U, I, D, T, Fu, Fi, B, n_neg, activator, alpha, bs = shape
    return f"U{U}-I{I}-D{D}-T{T}-F{Fu}x{Fi}-B{B}of{bs}-n{n_neg}-{activator}"


def perturb_time(w, rng):
    """Move ``time_embdding.weight`` off the identity it is constructed as, in place: an implementation that takes the
    time rows as one-hot is then wrong from the first step."""
    te = w["time_embdding.weight"]
    te += rng.uniform(-0.2, 0.2, te.shape).astype(te.dtype)
    return w


def condition(w, fea, activator):
    """The conditioning recipe, in place, for the piecewise activators only (relu, lrelu, prelu, hardtanh): features,
    the four Gaussian tables and the time table are clipped to [-1, 1], every encoder ``Linear`` row is scaled to an
    absolute row sum of at most 0.25, and its bias becomes the column pattern +0.5, -0.5 (hardtanh: +0.5, -0.5, +1.5,
    -1.5).  Every pre-activation is then at least 0.25 away from a kink by the triangle inequality.  The smooth
    activators get no recipe: the reference's fp32 gradients are within 5e-7 of their scale of the exact ones there."""
    if activator not in tn.PIECEWISE:
        return w, fea
    fea = tuple(np.clip(f, -1.0, 1.0) for f in fea)
    for k in list(tn.TABLES.values()) + ["time_embdding.weight"]:
        np.clip(w[k], -1.0, 1.0, out=w[k])
    pattern = np.array([0.5, -0.5, 1.5, -1.5] if activator == "hardtanh" else [0.5, -0.5])
    for enc in tn.ENCODERS:
        W, b = w[enc + ".0.weight"], w[enc + ".0.bias"]
        b[:] = np.resize(pattern, b.shape[0]).astype(b.dtype)
        rows = np.abs(W).sum(1, keepdims=True)
        W *= np.minimum(1.0, 0.25 / np.maximum(rows, 1e-30)).astype(W.dtype)
    return w, fea


def make_batch(rng, U, I, T, B, n_neg, mixed=True):
    """The eight-tuple with every collision a kernel can get wrong (see the module docstring)."""
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
    if mixed:
        allowed = np.array([t for t in range(T) if T < 4 or t not in (1, 2)])
        pos_t = rng.choice(allowed, B)
        neg_t = np.repeat(pos_t, n_neg).reshape(B, n_neg)
        pos_t[0], pos_t[B - 1] = 0, T - 1
        neg_t[0], neg_t[B - 1] = 0, T - 1
        if T >= 2:
            neg_t[0, 0] = T - 1
            neg_t[B - 1, n_neg - 1] = 0
        if B >= 3:
            neg_t[1:B - 1] = rng.choice(allowed, (B - 2, n_neg))
    else:
        pos_t, neg_t = np.full(B, T - 1), np.full((B, n_neg), T - 1)
    return pos_u, pos_1, pos_2, neg_u, neg_1, neg_2, pos_t.astype(np.int64), neg_t.reshape(-1).astype(np.int64)


def unused_time_rows(batch, T):
    t = np.concatenate([batch[6], batch[7]])
    return sorted(set(range(T + 1)) - set(t.tolist()) - set((t + 1).tolist()))


def check_batch(batch, U, I, T, mixed=True):
    pos_u, pos_1, pos_2, neg_u, neg_1, neg_2, pos_t, neg_t = batch
    B, n_neg = neg_u.shape
    neg_t = neg_t.reshape(B, n_neg)
    assert len(set(pos_u.tolist())) < B, "no user occurs twice as pos_u"
    assert (pos_1 == pos_2).any(), "no triple with pos_i_1 == pos_i_2"
    assert (neg_1 == pos_1[:, None]).any() or (neg_2 == pos_2[:, None]).any() or (neg_u == pos_u[:, None]).any(), \
        "no negative equals its own triple's positive"
    if n_neg >= 2:
        assert any(len(set(r.tolist())) < n_neg for a in (neg_u, neg_1, neg_2) for r in a), "no repeated negative in a row"
    users, items = np.concatenate([pos_u, neg_u.ravel()]), np.concatenate([pos_1, pos_2, neg_1.ravel(), neg_2.ravel()])
    assert U == 1 or U - 1 not in users, "the last user is drawn"
    assert I == 1 or I - 1 not in items, "the last item is drawn"
    every = np.concatenate([pos_t, neg_t.ravel()])
    assert every.min() >= 0 and every.max() <= T - 1
    if mixed:
        assert 0 in every and T - 1 in every, "t = 0 or t = time_step - 1 is missing"
        if T >= 2:
            assert (neg_t != pos_t[:, None]).any(), "no negative whose t differs from its triple's"
        if T >= 4:
            assert 2 in unused_time_rows(batch, T), "every time row is used"
    else:
        assert len(set(every.tolist())) == 1
        if T >= 2:
            assert unused_time_rows(batch, T), "every time row is used"


def draw_eps(rng, B, n_neg, D):
    return [rng.standard_normal((n, D)).astype(np.float32) for n in (B, B, B, B * n_neg, B * n_neg, B * n_neg)]


def synthetic(shape, mixed=True, seed=0):
    """``(weights, (user_fea, item_fea), batch, eps)`` for a shape; the same seed gives the same inputs everywhere.
    The weights follow the reference's constructor (uniform tables, ``nn.Linear``'s uniform bounds, slopes 0.25), with
    the user-side Gaussian tables spread around their constants and the time table off the identity, and then
    :func:`condition`."""
    U, I, D, T, Fu, Fi, B, n_neg, activator, alpha, bs = shape
    rng = np.random.default_rng(seed + 1000 * U + 10 * T + D + Fu)
    r = 0.1 * D ** -0.5
    w = {}
    for k, s in tn.shapes(U, I, D, T, Fu, Fi, activator == "prelu").items():
        if k == "time_embdding.weight":
            w[k] = np.eye(T + 1, dtype=np.float32)
        elif k == "user_mean.weight":
            w[k] = (1.0 + 0.1 * rng.standard_normal(s)).astype(np.float32)
        elif k == "user_std.weight":
            w[k] = (0.1 * rng.standard_normal(s)).astype(np.float32)
        elif k.endswith(".1.weight"):
            w[k] = np.full(s, 0.25, dtype=np.float32)
        elif k.endswith((".0.weight", ".0.bias")):
            fan_in = D + T + 1 + (Fu if k.split(".")[0].endswith("_u") else Fi)
            w[k] = rng.uniform(-fan_in ** -0.5, fan_in ** -0.5, s).astype(np.float32)
        else:
            w[k] = rng.uniform(-r, r, s).astype(np.float32)
    perturb_time(w, rng)
    fea = (rng.standard_normal((U, Fu)).astype(np.float32), rng.standard_normal((I, Fi)).astype(np.float32))
    w, fea = condition(w, fea, activator)
    batch = make_batch(rng, U, I, T, B, n_neg, mixed)
    return w, fea, batch, draw_eps(rng, B, n_neg, D)


def hyper(shape):
    """``(activator, alpha, scale)``."""
    return shape[8], shape[9], 1.0 / (3 * shape[10])
