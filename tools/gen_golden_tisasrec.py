"""ORACLE tooling (test infrastructure): capture the TiSASRec golden vectors from the REAL reference.

Runs only where the reference tree exists (REFERENCE_ROOT, default: where oracle/gen_golden.py looks); the reference
itself never travels -- only the small .npz fixtures written to tests/golden/tisasrec_*.npz do.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_tisasrec.py

Follows ``tools/gen_golden_sasrec.py`` (same shims, same batch maker and batch conditions, same ReLU-margin screen, same
``F.dropout`` capture with the replayed draw) and drives the reference's own ``TiSASRecEngine`` on the CPU.  The
reference hard-codes ``paddings.to("cuda")`` (models/tisasrec.py:135); for the duration of the run ``torch.Tensor.to``
is wrapped so that the device string ``"cuda"`` resolves to the CPU.  The module itself is not modified.

A fixture is ``tisasrec_<name>.npz`` (shapes, hyper-parameters, the initial weights, the batches of every step with their
time sequences and time matrices, the losses, and for the dropout fixture the ``5 + 3 * blocks`` keep masks of every
step) plus one ``tisasrec_<name>_s<k>.npz`` per step k = 1 .. 3.  Before step 1 every LayerNorm weight and bias and every
bias get non-trivial random values (the embeddings, the two position tables and the two time tables are N(0, 1) as
constructed).

Asserted here, with the figures printed: the SASRec batch conditions; the ReLU-margin screen; and for every batch that
its time matrix contains 0, contains the clamped value ``time_span`` and leaves at least one row of the time tables
never indexed (those rows' gradients must be exactly zero).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_sasrec as gs  # noqa: E402
import gen_golden_ultragcn as gu  # noqa: E402  (the shims and REF)

N_STEPS = gs.N_STEPS
N_USERS = gs.N_USERS


def import_reference():
    gu.import_reference()                                    # shims + sys.path
    from beta_rec.models import tisasrec as ref

    return ref


class cuda_means_cpu:
    """``tensor.to("cuda")`` resolves to the CPU while this is active (tisasrec.py:135 hard-codes the string)."""

    def __enter__(self):
        self.orig = orig = torch.Tensor.to

        def to(tensor, *a, **k):
            a = tuple("cpu" if isinstance(x, str) and x == "cuda" else x for x in a)
            if k.get("device") == "cuda":
                k["device"] = "cpu"
            return orig(tensor, *a, **k)

        torch.Tensor.to = to
        return self

    def __exit__(self, *exc):
        torch.Tensor.to = self.orig


def config_for(I, D, H, T, B, nb, p, l2, optimizer, lr, span):
    cfg = gs.config_for(I, D, H, T, B, nb, p, l2, optimizer, lr)
    cfg["model"]["time_span"] = span
    cfg["model"]["device"] = "cpu"          # the reference's model reads it in its constructor (tisasrec.py:191)
    return cfg


def make_times(rng, seq, span):
    """``time_seq [B, T]`` (0 at padded positions, as the reference's sampler leaves them) and its relation matrix.
    Row 0 moves in steps of 0 / 1, the other rows in multiples of 3 from a late start, so that small intervals, a few
    larger ones and the clamp occur while some table rows are never indexed."""
    import tisasrec_numpy as tn

    B, T = seq.shape
    ts = np.zeros((B, T), dtype=np.int64)
    for b in range(B):
        real = np.flatnonzero(seq[b])
        gaps = rng.integers(0, 2, real.size) if b == 0 else 3 * rng.integers(0, 3, real.size)
        ts[b, real] = (1 if b == 0 else 3 * (span // 3 + 1)) + np.cumsum(gaps)
    tm = np.stack([tn.time_relation(ts[b], span) for b in range(B)]).astype(np.int32)
    return ts, tm


def check_times(tm, span):
    used = np.unique(tm)
    assert used.min() == 0 and used.max() == span, "the matrix must hold 0 and the clamped value"
    unused = sorted(set(range(span + 1)) - set(used.tolist()))
    assert unused, "every row of the time tables is indexed"
    return unused


def relu_margins(w, batch, H, l2, keep, p):
    import tisasrec_numpy as tn
    from helpers import float64_oracle, to64

    with float64_oracle(tn):
        _, _, cache = tn.tisasrec_grads(to64(w), batch, H, l2, keep, p, with_cache=True)
    return [(float((c["pre1"] <= 0).mean()), float(np.abs(c["pre1"]).min() / np.abs(c["pre1"]).max()))
            for c in cache["blocks"]]


def nontrivial(rng, w):
    out = {k: v.copy() for k, v in w.items()}
    for k, v in out.items():
        if "layernorm" in k and k.endswith("weight"):
            out[k] = (1.0 + 0.3 * rng.standard_normal(v.shape)).astype(np.float32)
        elif k.endswith("bias"):
            out[k] = (0.2 * rng.standard_normal(v.shape)).astype(np.float32)
    return out


def mask_shapes(B, T, D, H, nb):
    """(shape the reference draws, is it an FFN mask) of the 5 + 3 * blocks dropout calls."""
    out = [((B, T, D), False)] * 3 + [((B, T, T, D), False)] * 2
    for _ in range(nb):
        out += [((H * B, T, T), False), ((B, D, T), True), ((B, D, T), True)]
    return out


def fixture(ref, name, I, D, H, T, B, nb, p, l2, optimizer, lr, span, seed, screen_only=False):
    import tisasrec_numpy as tn

    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    cfg = config_for(I, D, H, T, B, nb, p, l2, optimizer, lr, span)
    eng = gu.quiet(ref.TiSASRecEngine, cfg)
    keys = tn.keys(nb)
    assert tuple(eng.model.state_dict()) == keys == tuple(n for n, _ in eng.model.named_parameters())
    w0 = nontrivial(rng, {k: v.detach().numpy().copy() for k, v in eng.model.state_dict().items()})
    with torch.no_grad():
        for k, prm in eng.model.named_parameters():
            prm.copy_(torch.from_numpy(w0[k]))
    assert float(np.abs(w0["item_emb.weight"][0]).max()) == 0.0
    assert all(float(np.abs(w0[k]).max()) > 0 for k in keys if k.endswith("bias") or "pos" in k or "time" in k)
    assert {k: tuple(v.shape) for k, v in w0.items()} == tn.shapes(I, T, span, D, nb)
    base = {"meta": np.array([I, T, D, H, nb, B, N_STEPS, seed, span], dtype=np.int64), "optimizer": np.array(optimizer),
            "lr": np.array(lr), "l2_emb": np.array(l2), "dropout_rate": np.array(p)}
    for k in keys:
        base[f"w0/{k}"] = w0[k]
    seen = []
    orig_step = eng.optimizer.step

    def capturing_step(*a, **k):
        seen.append({n: prm.grad.detach().numpy().copy() for n, prm in eng.model.named_parameters()})
        return orig_step(*a, **k)

    eng.optimizer.step = capturing_step
    F = torch.nn.functional
    orig_dropout = F.dropout
    calls = []

    def capturing_dropout(input, p=0.5, training=True, inplace=False):   # noqa: A002
        if not training or p == 0.0:
            return orig_dropout(input, p, training, inplace)
        before = torch.get_rng_state()
        x = input.detach().clone()
        out = orig_dropout(input, p, training, inplace)
        after = torch.get_rng_state()
        torch.set_rng_state(before)
        replay = torch.empty_like(x).bernoulli_(1 - p).to(torch.bool)
        torch.set_rng_state(after)
        applied = out.detach() != 0
        known = x != 0
        calls.append((torch.where(known, applied, replay).numpy().copy(), bool((applied == replay)[known].all()),
                      tuple(x.shape)))
        return out

    seqs, tss, tms, poss, negs, losses, sizes, replay_ok, unused_rows = [], [], [], [], [], [], [], [], []
    F.dropout = capturing_dropout
    try:
        with cuda_means_cpu():
            for s in range(N_STEPS):
                seq, pos, neg = gs.make_batch(rng, I, T, B)
                shared = gs.check_batch(seq, pos, neg, T)
                ts, tm = make_times(rng, seq, span)
                try:
                    unused = check_times(tm, span)
                except AssertionError:
                    if screen_only:
                        return False
                    raise
                batch = (seq, tm, pos, neg)
                w_now = {k: v.detach().numpy().copy() for k, v in eng.model.state_dict().items()}
                del calls[:]
                eng.model.train()
                loss = eng.train_single_batch((np.arange(B), seq, ts, tm, pos, neg))
                keep = None
                if p > 0:
                    want = mask_shapes(B, T, D, H, nb)
                    assert len(calls) == len(want), f"{len(calls)} dropout calls"
                    keep = []
                    for i, ((mask, ok, shape), (shape_ref, ffn)) in enumerate(zip(calls, want)):
                        assert shape == shape_ref, (i, shape, shape_ref)
                        keep.append((mask.transpose(0, 2, 1) if ffn else mask).astype(np.uint8).reshape(-1))
                        base[f"keep{s}/{i}"] = keep[-1]
                        replay_ok.append(ok)
                margins = relu_margins(w_now, batch, H, l2, keep, p)
                for b, (inactive, margin) in enumerate(margins):
                    print(f"{name} step {s} block {b}: {inactive:.1%} of the ReLU units inactive, smallest |pre| / "
                          f"largest {margin:.2e}; {shared} items in seq, pos and neg at once; time-table rows never "
                          f"indexed: {unused}")
                    if screen_only and (margin < 2e-4 or not 0.25 <= inactive <= 0.75):
                        return False
                    assert margin >= 1e-4, f"{name}: a ReLU unit sits {margin:.1e} of its layer's scale from zero"
                    assert 0.25 <= inactive <= 0.75, f"{name}: {inactive:.1%} inactive"
                assert float(eng.model.item_emb.weight.detach()[0].abs().max()) == 0.0
                losses.append(loss)
                step = {}
                for k, v in eng.model.state_dict().items():
                    step[f"w/{k}"] = v.detach().numpy().copy()
                for k, v in seen[-1].items():
                    step[f"g/{k}"] = v
                for pname, prm in eng.model.named_parameters():
                    pst = eng.optimizer.state.get(prm, {})
                    for sk, tag in (("exp_avg", "m"), ("exp_avg_sq", "v"), ("square_avg", "v")):
                        if sk in pst:
                            step[f"{tag}/{pname}"] = pst[sk].detach().numpy().copy()
                if not screen_only:
                    path = os.path.join(OUT, f"{name}_s{s + 1}.npz")
                    np.savez_compressed(path, **step)
                    sizes.append(os.path.getsize(path))
                seqs.append(seq), tss.append(ts), tms.append(tm), poss.append(pos), negs.append(neg)
                unused_rows.append(unused)
    finally:
        F.dropout = orig_dropout
    if screen_only:
        return True
    base.update(seq=np.stack(seqs), time_seq=np.stack(tss), time_matrix=np.stack(tms), pos=np.stack(poss),
                neg=np.stack(negs), losses=np.array(losses, dtype=np.float64))
    if p > 0:
        base["replay_ok"] = np.array(replay_ok)
        print(f"{name}: drawing F.dropout's mask again from the same RNG state reproduces the mask in "
              f"{sum(replay_ok)} of {len(replay_ok)} calls")
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **base)
    print(f"{name}: optimizer {optimizer}, losses {losses}")
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB + steps {[f'{s / 1024:.0f} KiB' for s in sizes]}")
    assert max(sizes + [os.path.getsize(path)]) < 500_000
    return True


def init_fixture(ref):
    """Seeded construction: the weights TiSASRecEngine builds for torch seed 2020."""
    I, D, H, T, nb, span = 50, 64, 2, 20, 2, 24
    torch.manual_seed(2020)
    eng = gu.quiet(ref.TiSASRecEngine, config_for(I, D, H, T, 8, nb, 0.2, 0.0, "adam", 1e-3, span))
    out = {"meta": np.array([I, T, D, H, nb, 2020, span], dtype=np.int64)}
    for k, v in eng.model.state_dict().items():
        out[f"w/{k}"] = v.detach().numpy().copy()
    path = os.path.join(OUT, "tisasrec_init.npz")
    np.savez_compressed(path, **out)
    print(f"tisasrec_init: {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    ref = import_reference()
    cases = [("tisasrec_adam", dict(I=40, D=32, H=2, T=12, B=5, nb=2, p=0.0, l2=0.1, optimizer="adam", lr=1e-3,
                                    span=16), 100),
             ("tisasrec_sgd_h1", dict(I=40, D=16, H=1, T=7, B=3, nb=1, p=0.0, l2=0.0, optimizer="sgd", lr=0.05,
                                      span=8), 1000),
             ("tisasrec_rmsprop_drop", dict(I=40, D=32, H=2, T=12, B=4, nb=2, p=0.25, l2=0.01, optimizer="rmsprop",
                                            lr=1e-3, span=16), 2000)]
    for name, kw, first in cases:
        seed = next(sd for sd in range(first, first + 1000)
                    if gu.quiet(fixture, ref, name, seed=sd, screen_only=True, **kw))
        print(f"{name}: seed {seed}")
        fixture(ref, name, seed=seed, **kw)
    init_fixture(ref)


if __name__ == "__main__":
    main()
