"""ORACLE tooling (test infrastructure): capture the NARM golden vectors from the REAL reference.

Runs only where the reference tree exists (REFERENCE_ROOT, default: where oracle/gen_golden.py looks); the reference
itself never travels -- only the small .npz fixtures written to tests/golden/narm_*.npz do.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_narm.py

Imports ``beta_rec.models.narm`` with the in-process shims of ``tools/gen_golden_ultragcn.py`` plus two empty stand-in
modules (``py7zr``, ``aiofiles``: ``beta_rec.datasets`` imports them, nothing here calls them) and drives the reference's
own ``NARMEngine`` on the CPU.  Every step is one epoch of ONE batch through ``train_an_epoch(loader, epoch)`` with
``epoch = 0, 1, 2``, so the StepLR rule is on the path: ``narm_adam`` has ``lr_dc_step = 2``, ``lr_dc = 0.1`` (its third
step runs at ``lr / 10``); the other cases never reach their decay step.

A fixture is ``narm_<name>.npz`` (shapes, hyper-parameters, the constructed weights ``winit`` for the fixture's torch
seed, the initial weights ``w0`` = ``winit`` with non-trivial GRU biases, every step's batch, the losses, the keep masks)
plus one ``narm_<name>_s<k>.npz`` per step k = 1 .. 3 (that step's gradients, the weights and the optimizer state after
it).  The dropout masks are captured by wrapping ``torch.nn.functional.dropout`` as ``tools/gen_golden_sasrec.py`` does;
``replay_ok`` records whether a draw from the same RNG state reproduces each mask.

Asserted here, with the figures printed: every batch holds a session of full length, a session of length 1, a session
with a 0 inside its length, an item that occurs twice in one session and in two sessions, a target that also sits in its
own session, two rows with the same target; in the fp64 evaluation no sigmoid input of alpha exceeds 6 in magnitude.
Also writes ``narm_loader.npz``: a dozen ragged sequences, ``dataset_to_seq_target_format`` of them and the batches the
reference's ``DataLoader(SeqDataset, 5, shuffle=False, collate_fn=collate_fn)`` makes.
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_golden_ultragcn as gu  # noqa: E402  (the shims and REF)

N_STEPS = 3


def import_reference():
    for name in ("py7zr", "aiofiles"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    # dataset_base.py registers the name as an unpack format at import; nothing here calls it
    sys.modules["py7zr"].unpack_7zarchive = lambda *a, **k: None
    gu.import_reference()                                    # shims + sys.path
    from beta_rec.datasets import seq_data_utils as sdu
    from beta_rec.models import narm as ref

    return ref, sdu


def config_for(I, D, H, L, B, p_in, p_hid, optimizer, lr, lr_dc_step, lr_dc):
    return {"dataset": {"n_items": I},
            "model": {"hidden_size": H, "n_layers": L, "embedding_dim": D, "dropout_input": p_in,
                      "dropout_hidden": p_hid, "batch_size": B, "optimizer": optimizer, "lr": lr,
                      "lr_dc_step": lr_dc_step, "lr_dc": lr_dc, "device_str": "cpu"},
            "system": {"run_dir": "/tmp/hiprec_golden_runs"}}


def make_batch(rng, I, T, B):
    """Lengths T, ..., 1 (sorted, with a tie); a 0 inside session 0; one item twice in session 0 and again in session
    1; target 1 sits in its own session; targets 2 and 3 are the same item."""
    lens = np.sort(np.concatenate([[T, 1], rng.integers(2, T, B - 2)]))[::-1].copy()
    lens[2] = lens[1]
    seq = np.zeros((T, B), dtype=np.int64)
    for b, n in enumerate(lens):
        seq[:n, b] = rng.integers(1, I, n)
    x = int(rng.integers(1, I))
    seq[0, 0] = seq[3, 0] = seq[1, 1] = x
    seq[2, 0] = 0
    target = rng.integers(1, I, B)
    target[1] = seq[0, 1]
    target[3] = target[2]
    return seq, target, lens


def check_batch(seq, target, lens, T):
    B = len(lens)
    assert (lens == T).any() and (lens == 1).any() and (np.diff(lens) <= 0).all()
    inside = [(seq[:lens[b], b] == 0).any() for b in range(B)]
    assert any(inside), "no 0 inside a session's length"
    twice = [i for b in range(B) for i in set(seq[:lens[b], b].tolist()) - {0}
             if (seq[:lens[b], b] == i).sum() >= 2 and sum(i in seq[:lens[c], c] for c in range(B)) >= 2]
    assert twice, "no item twice in one session and in two sessions"
    own = [b for b in range(B) if target[b] in seq[:lens[b], b]]
    assert own, "no target sits in its own session"
    assert len(set(target.tolist())) < B, "no two rows share a target"
    return sum(inside), len(set(twice)), len(own), B - len(set(target.tolist()))


def alpha_inputs(w, batch, keep, p):
    """Largest |q1 + mask q2| of the fp64 evaluation over the positions inside a length."""
    import narm_numpy as nn_
    from helpers import float64_oracle, to64

    seq, _, lens = batch
    with float64_oracle(nn_):
        _, c = nn_.narm_forward(to64(w), seq, lens, keep, p)
    s = np.clip(c["s"], 1e-300, 1 - 1e-16)
    pre = np.log(s) - np.log1p(-s)
    live = np.arange(seq.shape[0])[:, None] < np.asarray(lens)[None, :]
    return float(np.abs(pre[live]).max())


def fixture(ref, name, I, D, H, L, T, B, p_in, p_hid, optimizer, lr, lr_dc_step, lr_dc, seed):
    import narm_numpy as nn_

    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    cfg = config_for(I, D, H, L, B, p_in, p_hid, optimizer, lr, lr_dc_step, lr_dc)
    eng = gu.quiet(ref.NARMEngine, cfg)
    keys = nn_.keys(L)
    assert tuple(eng.model.state_dict()) == keys == tuple(n for n, _ in eng.model.named_parameters())
    winit = {k: v.detach().numpy().copy() for k, v in eng.model.state_dict().items()}
    w0 = {k: v.copy() for k, v in winit.items()}
    for k in keys:
        if "bias" in k:
            w0[k] = (0.2 * rng.standard_normal(w0[k].shape)).astype(np.float32)
    with torch.no_grad():
        for k, prm in eng.model.named_parameters():
            prm.copy_(torch.from_numpy(w0[k]))
    assert float(np.abs(w0["emb.weight"][0]).max()) == 0.0
    base = {"meta": np.array([I, T, D, H, L, B, N_STEPS, seed], dtype=np.int64), "optimizer": np.array(optimizer),
            "lr": np.array(lr), "lr_dc_step": np.array(lr_dc_step), "lr_dc": np.array(lr_dc),
            "dropout_input": np.array(p_in), "dropout_hidden": np.array(p_hid)}
    for k in keys:
        base[f"w0/{k}"] = w0[k]
        base[f"winit/{k}"] = winit[k]
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

    p = (p_in, p_hid)
    seqs, targets, lenss, losses, sizes, replay_ok, lrs = [], [], [], [], [], [], []
    F.dropout = capturing_dropout
    try:
        for s in range(N_STEPS):
            batch = make_batch(rng, I, T, B)
            figures = check_batch(*batch, T)
            w_now = {k: v.detach().numpy().copy() for k, v in eng.model.state_dict().items()}
            del calls[:]
            loader = [(torch.from_numpy(batch[0]), torch.from_numpy(batch[1]), batch[2].tolist())]
            loss = gu.quiet(eng.train_an_epoch, loader, s)
            lrs.append(eng.optimizer.param_groups[0]["lr"])
            assert abs(lrs[-1] - nn_.step_lr(lr, lr_dc, lr_dc_step, s)) <= 1e-12 * lr, (lrs, s)
            keep = None
            if any(p):
                assert len(calls) == 2, f"{len(calls)} dropout calls"
                keep = []
                for i, (mask, ok, shape) in enumerate(calls):
                    assert shape == ((T, B, D), (B, 2 * H))[i], shape
                    keep.append(mask.astype(np.uint8).reshape(-1))
                    base[f"keep{s}/{i}"] = keep[-1]
                    replay_ok.append(ok)
            big = alpha_inputs(w_now, batch, keep, p)
            print(f"{name} step {s}: lr {lrs[-1]:g}; {figures[0]} sessions with a 0 inside, {figures[1]} items twice in "
                  f"one session and in two, {figures[2]} targets in their own session, {figures[3]} repeated targets; "
                  f"largest |sigmoid input| of alpha {big:.2f}")
            assert big <= 6.0
            assert float(eng.model.emb.weight.detach()[0].abs().max()) == 0.0
            losses.append(float(loss))
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
            path = os.path.join(OUT, f"{name}_s{s + 1}.npz")
            np.savez_compressed(path, **step)
            sizes.append(os.path.getsize(path))
            seqs.append(batch[0]), targets.append(batch[1]), lenss.append(batch[2])
    finally:
        F.dropout = orig_dropout
    base.update(seq=np.stack(seqs), target=np.stack(targets), lens=np.stack(lenss),
                losses=np.array(losses, dtype=np.float64), lrs=np.array(lrs, dtype=np.float64))
    if any(p):
        base["replay_ok"] = np.array(replay_ok)
        print(f"{name}: drawing F.dropout's mask again from the same RNG state reproduces the mask in "
              f"{sum(replay_ok)} of {len(replay_ok)} calls")
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **base)
    print(f"{name}: optimizer {optimizer}, losses {losses}")
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB + steps {[f'{s / 1024:.0f} KiB' for s in sizes]}")
    assert max(sizes + [os.path.getsize(path)]) < 500_000


def loader_fixture(sdu):
    from torch.utils.data import DataLoader

    rng = np.random.default_rng(7)
    lengths = [2, 5, 3, 3, 6, 2, 4, 3, 7, 2, 5, 4]
    sequences = [rng.integers(1, 30, n).tolist() for n in lengths]
    out_seqs, labs = sdu.dataset_to_seq_target_format({"col_sequence": sequences})
    loader = DataLoader(sdu.SeqDataset((out_seqs, labs), print_info=False), batch_size=5, shuffle=False,
                        collate_fn=sdu.collate_fn)
    out = {"seq_flat": np.concatenate(sequences).astype(np.int64), "seq_lens": np.array(lengths, dtype=np.int64),
           "out_flat": np.concatenate(out_seqs).astype(np.int64),
           "out_lens": np.array([len(s) for s in out_seqs], dtype=np.int64), "labels": np.array(labs, dtype=np.int64),
           "batch_size": np.array(5)}
    n = 0
    tie = False
    for seq, target, lens in loader:
        out[f"b{n}/seq"], out[f"b{n}/target"], out[f"b{n}/lens"] = seq.numpy().copy(), target.numpy(), np.array(lens)
        tie = tie or len(set(lens)) < len(lens)
        n += 1
    out["n_batches"] = np.array(n)
    assert len(out_seqs) % 5 != 0 and tie, "the last batch must be partial and some lengths must tie"
    path = os.path.join(OUT, "narm_loader.npz")
    np.savez_compressed(path, **out)
    print(f"narm_loader: {len(out_seqs)} pairs in {n} batches, {os.path.getsize(path) / 1024:.0f} KiB")


def main():
    ref, sdu = import_reference()
    cases = [("narm_adam", dict(I=40, D=12, H=20, L=1, T=7, B=6, p_in=0.0, p_hid=0.0, optimizer="adam", lr=1e-2,
                                lr_dc_step=2, lr_dc=0.1), 100),
             ("narm_sgd_l2", dict(I=40, D=16, H=16, L=2, T=7, B=6, p_in=0.0, p_hid=0.0, optimizer="sgd", lr=0.05,
                                  lr_dc_step=80, lr_dc=0.1), 1000),
             ("narm_rmsprop_drop", dict(I=40, D=12, H=20, L=1, T=7, B=6, p_in=0.25, p_hid=0.5, optimizer="rmsprop",
                                        lr=1e-3, lr_dc_step=80, lr_dc=0.1), 2000)]
    for name, kw, seed in cases:
        fixture(ref, name, seed=seed, **kw)
    loader_fixture(sdu)


if __name__ == "__main__":
    main()
