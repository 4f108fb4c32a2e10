"""The synthetic VAECF inputs the GPU edge tests run against the fp64 restatement (tests/vaecf_numpy.py), the recipe that
keeps every activation and the KL term well conditioned, and the batch layout the fixtures share.  Each shape is
``(n_items, hidden, z_dim, B, activation, likelihood, valued)``; ``valued``: the nonzeros are 0.5 / 1 / 1.5, not all 1.

Which constant of csrc/vaecf.hip (or of the grouped GEMM in csrc/ncf.hip) each value straddles:

* the fused last layer's 64 x 64 tiles (``kVcTile``; 64 is the wave width as well): n_items = 1, 63, 64, 65, and 130 /
  150 / 200 / 300 (3 .. 5 tiles, as many item splits, the last tile partly empty); B = 1, 63, 65 (one row block, one
  row short of it, one row into the second) and 130 (three row blocks);
* the 64 nonzeros a wave takes at once (the first layer's gather and scatter, the sparse pass): the full rows of
  n_items = 130 .. 300 hold more, those of n_items = 65 and 64 (which leaves no item out) hold exactly 64, the one of
  n_items = 63 holds 62;
* the K chunk of 32 (``kVcKc``) and the GEMM's 64 x 64 tiles with a K tile of 32: H1 = 1, 20 (the default), 33 and 40
  (one past, and no multiple of, 32), 512 (the limit: every column slot of a lane in use); z_dim = 1, 10, 256;
* one, two and three hidden layers (the enc_mu / enc_logvar addend of the first layer's backward exists only with one);
* every activation and every likelihood.

Every batch of two or more rows holds an empty row, a full row, an item that several rows share and an item no row
touches: "full" therefore means every item but that last one (its W0 gradient column must stay exactly zero).  The
shape with n_items = 64 and the one-row shapes have a row with EVERY item instead.
"""
import numpy as np

import vaecf_numpy as vn

SHAPES = [
    (1, [1], 1, 1, "tanh", "mult", False),
    (63, [20], 10, 63, "tanh", "mult", False),
    (64, [20], 10, 6, "relu", "bern", False),
    (65, [33], 10, 65, "sigmoid", "gaus", True),
    (150, [20], 10, 5, "relu6", "pois", True),
    (200, [33, 17], 1, 7, "tanh", "mult", True),
    (130, [40, 20, 9], 10, 4, "relu", "mult", False),
    (70, [512], 256, 3, "tanh", "bern", False),
    (300, [20], 10, 130, "tanh", "mult", False),
]
EVERY_ITEM = {64}          # n_items of the shapes whose full row leaves no item out
MIN_PRE = 0.1              # |pre-activation| and |pre-activation - 6| stay above this
MAX_LOGVAR = 1.0
BETA = 0.2


def shape_id(shape):
    I, hidden, Z, B, activation, likelihood, valued = shape
    return f"I{I}-H{'x'.join(map(str, hidden))}-Z{Z}-B{B}-{activation}-{likelihood}{'-valued' if valued else ''}"


def _rows_to(W, limit):
    W *= np.minimum(1.0, limit / np.maximum(np.abs(W).sum(1, keepdims=True), 1e-30)).astype(W.dtype)


def condition(w):
    """The conditioning recipe, in place.  relu and relu6 have kinks at 0 and 6, where a rounding error flips a whole
    gradient column, so every pre-activation is kept at 0.5 +- 0.4: each hidden layer's bias becomes +-0.5 (alternating
    by column) and its weight rows are scaled to an absolute row sum of at most 0.15 (the first layer: its input is at
    most 1.5 per item), 0.05 (the decoder's first layer: ``z`` is unbounded; 0.4 allows |z| <= 8) or 0.25 (the others:
    their input is an activation in [-1, 1]).  ``enc_logvar`` is treated like a hidden layer, which keeps |logvar| below
    0.75.  ``enc_mu`` and the decoder's last layer stay as constructed."""
    n = vn.n_hidden_of(w)
    for l in range(n):
        for side, limit in (("encoder", 0.15 if l == 0 else 0.25), ("decoder", 0.05 if l == 0 else 0.25)):
            b = w[f"{side}.fc{l}.bias"]
            b[:] = np.where(np.arange(b.shape[0]) % 2 == 0, 0.5, -0.5)
            _rows_to(w[f"{side}.fc{l}.weight"], limit)
    b = w["enc_logvar.bias"]
    b[:] = np.where(np.arange(b.shape[0]) % 2 == 0, 0.5, -0.5)
    _rows_to(w["enc_logvar.weight"], 0.25)
    return w


def make_x(rng, B, I, valued=False, every_item=False):
    """A dense batch with the rows a kernel can get wrong (see the module docstring)."""
    x = (rng.random((B, I)) < 0.3).astype(np.float32)
    if B >= 2:
        x[0] = 0.0
        x[1] = 1.0
        if B >= 3:
            x[2:, 0] = 1.0               # item 0 is in every row but the empty one
        if not every_item:
            x[:, I - 1] = 0.0
    else:
        x[0] = 1.0
    if valued:
        x *= rng.choice(np.array([0.5, 1.0, 1.5], dtype=np.float32), size=x.shape)
    return x


def check_batch(x, every_item=False):
    B, I = x.shape
    nz = x != 0
    assert (~nz).all(1).any(), "no empty row"
    assert (nz.sum(0) >= 2).any(), "no item in several rows"
    if every_item:
        assert nz.all(1).any(), "no row with every item"
    else:
        assert not nz[:, I - 1].any(), "the last item is in some row"
        assert nz[:, :I - 1].all(1).any(), "no full row"


def synthetic(shape, seed=0):
    """``(weights, x, eps)`` for a shape; the same seed gives the same inputs everywhere.  The weights follow
    ``nn.Linear``'s uniform bounds and then :func:`condition`."""
    I, hidden, Z, B, activation, likelihood, valued = shape
    rng = np.random.default_rng(seed + 1000 * I + 10 * B + Z + sum(hidden))
    w = {}
    for k, s in vn.shapes(I, hidden, Z).items():
        fan_in = vn.shapes(I, hidden, Z)[k.rsplit(".", 1)[0] + ".weight"][1]
        w[k] = rng.uniform(-fan_in ** -0.5, fan_in ** -0.5, s).astype(np.float32)
    condition(w)
    x = make_x(rng, B, I, valued, I in EVERY_ITEM)
    return w, x, rng.standard_normal((B, Z)).astype(np.float32)


def margins_ok(info, activation):
    """The kinks matter to relu and relu6 only; tanh and sigmoid are smooth everywhere."""
    kinks = activation not in ("relu", "relu6") or (info["min_abs_pre"] >= MIN_PRE
                                                    and info["min_abs_pre_minus_6"] >= MIN_PRE)
    return kinks and info["max_abs_logvar"] <= MAX_LOGVAR
