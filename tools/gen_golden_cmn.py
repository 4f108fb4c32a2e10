"""ORACLE tooling (test infrastructure): capture the CMN golden vectors from the REAL reference.

Runs only where the reference tree exists (REFERENCE_ROOT, default: where oracle/gen_golden.py looks); the reference
itself never travels -- only the small .npz fixtures written to tests/golden/cmn_*.npz do.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_cmn.py

Imports ``beta_rec.models.cmn`` with the same two in-process shims ``tools/gen_golden_ultragcn.py`` uses and drives the
reference's own ``cmnEngine`` on seeded synthetic neighbourhoods.  A fixture is ``cmn_<name>.npz`` (shapes, the
item -> users lists as a CSR, the triples of every step, the initial weights, losses and pre-clip gradient norms) plus
one ``cmn_<name>_s<k>.npz`` per step k = 1 .. 3 (weights, clipped gradient and optimizer state AFTER that step), which
keeps every file a fraction of a megabyte.  The batches are stored as triples: the seven arrays of a batch are what
``cmn_train_loader`` makes of them (``cmn_numpy.padded_batch``).

Asserted here, with the figures printed: every fixture holds lists of 1, 2, 63, 64, 65 and 300 ids (the 300-id list
visits each of the 100 users three times), an item that is positive and negative in one batch, a user present in every
list of two or more, u in N(i+), and a short last batch; no ReLU pre-activation of the fp64 evaluation lies within 1e-4
of its layer's largest magnitude from zero; in cmn_sgd_hot_clip between 25 % and 75 % of each ReLU layer's units are
inactive and the clip is active; in cmn_adam the clip is inactive.
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

import gen_golden_ultragcn as gu  # noqa: E402  (the shims and REF)

LENGTHS = [1, 2, 63, 64, 65, 300, 7, 30, 12, 5, 90, 3]     # one list per item
U, I = 100, len(LENGTHS)
BATCHES = [14, 14, 5]                                        # batch_size 14, a short last batch


def import_reference():
    gu.import_reference()                                    # shims + sys.path
    from beta_rec.models import cmn as ref_cmn

    return ref_cmn


def neighbourhoods(rng):
    """item -> list of users: distinct users per list (the 300-id list: three permutations of all users); user 0 sits
    in every list of two or more."""
    out = {}
    for i, n in enumerate(LENGTHS):
        if n <= U:
            lst = rng.choice(U, size=n, replace=False)
        else:
            lst = np.concatenate([rng.permutation(U) for _ in range(n // U)])
        if n >= 2 and 0 not in lst:
            lst[rng.integers(0, n)] = 0
        out[i] = [int(x) for x in lst]
    return out


def csr_of(lists):
    rowptr = np.zeros(I + 1, dtype=np.int64)
    np.cumsum([len(lists[i]) for i in range(I)], out=rowptr[1:])
    return rowptr, np.concatenate([np.asarray(lists[i], dtype=np.int64) for i in range(I)])


def triples(rng, lists, B, first):
    """B samples.  The first batch walks every item as a positive and as a negative; half the users come from N(i+)."""
    pos = rng.integers(0, I, B)
    neg = rng.integers(0, I, B)
    if first:
        pos[:I] = np.arange(I)
        neg[:I] = np.roll(np.arange(I), 5)
    neg = np.where(neg == pos, (neg + 1) % I, neg)
    users = rng.integers(0, U, B)
    for b in range(0, B, 2):
        users[b] = lists[int(pos[b])][int(rng.integers(0, len(lists[int(pos[b])])))]
    return users, pos, neg


def config_for(D, optimizer, lr, grad_clip):
    return {"emb_dim": D, "device_str": "cpu", "regs": [1e-5], "batch_size": BATCHES[0], "lr": lr, "momentum": 0.9,
            "training_l2_lambda": 0.001, "grad_clip": grad_clip, "neg_count": 4,
            "model": {"optimizer": optimizer, "lr": lr, "device_str": "cpu"},
            "system": {"run_dir": "/tmp/hiprec_golden_runs"}}


def relu_margins(w, batch, lam):
    """(share of inactive units per ReLU layer, smallest |pre-activation| relative to the layer's largest) in fp64."""
    import cmn_numpy as cn
    from helpers import float64_oracle, to64

    with float64_oracle(cn):
        _, _, caches = cn.cmn_grads(to64(w), batch, lam, with_cache=True)
    out = {}
    for name in ("pre1", "preh"):
        pre = np.concatenate([c[name].reshape(-1) for c in caches])
        out[name] = (float((pre <= 0).mean()), float(np.abs(pre).min() / np.abs(pre).max()))
    return out


def hot_weights(rng, D):
    """Every weight N(0, 0.5), every bias zero."""
    import cmn_numpy as cn

    shapes = {"user_memory.weight": (U, D), "item_memory.weight": (I, D), "user_output.weight": (U, D),
              "mem_layer.hop_mapping.1.weight": (D, D), "mem_layer.hop_mapping.1.bias": (D,),
              "dense.weight": (D, 2 * D), "dense.bias": (D,), "out.weight": (1, D)}
    return {k: (np.zeros(shapes[k]) if k.endswith("bias") else rng.standard_normal(shapes[k]) * 0.5).astype(np.float32)
            for k in cn.KEYS}


def hot_seed_passes(seed, D, lr, grad_clip, lam=0.001):
    """The hot fixture's ReLU-margin condition, tried on the restatement's own trajectory (same draws as fixture()):
    with ~13 000 pre-activations per fixture only about one seed in a hundred leaves none within 1e-4 of its layer's
    scale from zero, so seeds are screened here and the reference then confirms the one that passes."""
    import cmn_numpy as cn

    rng = np.random.default_rng(seed)
    lists = neighbourhoods(rng)
    rowptr, col = csr_of(lists)
    rng.standard_normal((U, D)), rng.standard_normal((I, D))
    w = hot_weights(rng, D)
    st = cn.new_opt_state(w, "sgd")
    for s, B in enumerate(BATCHES):
        batch = cn.padded_batch(rowptr, col, *triples(rng, lists, B, s == 0))
        if any(m < 2e-4 for _, m in relu_margins(w, batch, lam).values()):
            return False
        cn.cmn_train_step(w, st, batch, lam, grad_clip, "sgd", lr)
    return True


def fixture(ref_cmn, name, D, optimizer, lr, seed, grad_clip=5.0, hot=False):
    import cmn_numpy as cn

    rng = np.random.default_rng(seed)
    lists = neighbourhoods(rng)
    rowptr, col = csr_of(lists)
    ue = (rng.standard_normal((U, D)) * 0.01).astype(np.float32)
    ie = (rng.standard_normal((I, D)) * 0.01).astype(np.float32)
    torch.manual_seed(seed)
    cfg = config_for(D, optimizer, lr, grad_clip)
    eng = gu.quiet(ref_cmn.cmnEngine, cfg, ue, ie, lists)
    assert cfg["max_neighbors"] == 300
    assert list(dict(eng.model.named_parameters())) == list(cn.KEYS) == list(eng.model.state_dict())
    if hot:
        w_hot = hot_weights(rng, D)
        with torch.no_grad():
            for k, p in eng.model.named_parameters():
                p.copy_(torch.from_numpy(w_hot[k]))
    kind = type(eng.optimizer).__name__
    mom = eng.optimizer.defaults.get("momentum", 0)
    opt_name = {"Adam": "adam", "SGD": "sgd", "RMSprop": "rmsprop_momentum" if mom else "rmsprop"}[kind]
    lam = cfg["training_l2_lambda"]
    base = {"meta": np.array([U, I, D, BATCHES[0], len(BATCHES), seed], dtype=np.int64), "optimizer": np.array(opt_name),
            "lr": np.array(lr), "momentum": np.array(float(mom)), "l2_lambda": np.array(lam),
            "grad_clip": np.array(grad_clip), "rowptr": rowptr, "col": col}
    for k, v in eng.model.state_dict().items():
        base[f"w0/{k}"] = v.detach().numpy().copy()
    seen, norms = [], []
    orig_step = eng.optimizer.step

    def capturing_step(*a, **k):
        seen.append({n: p.grad.detach().numpy().copy() for n, p in eng.model.named_parameters()})
        return orig_step(*a, **k)

    eng.optimizer.step = capturing_step
    orig_clip = ref_cmn.nn.utils.clip_grad_norm_

    def capturing_clip(*a, **k):
        norms.append(float(orig_clip(*a, **k)))
        return norms[-1]

    ref_cmn.nn.utils.clip_grad_norm_ = capturing_clip
    users, pos, neg, ptr, losses, sizes = [], [], [], [0], [], []
    try:
        for s, B in enumerate(BATCHES):
            u, p, n = triples(rng, lists, B, s == 0)
            batch = cn.padded_batch(rowptr, col, u, p, n)
            w_now = {k: v.detach().numpy().copy() for k, v in eng.model.state_dict().items()}
            margins = relu_margins(w_now, batch, lam)
            for layer, (inactive, margin) in margins.items():
                print(f"{name} step {s} {layer}: {inactive:.1%} inactive, smallest |pre| / largest {margin:.2e}")
                assert margin >= 1e-4, f"{name}: a {layer} unit sits {margin:.1e} of the layer's scale from zero; change the seed"
                if hot:
                    assert 0.25 <= inactive <= 0.75, f"{name}: {inactive:.1%} of {layer} inactive"
            losses.append(eng.train_single_batch(tuple(torch.from_numpy(a) for a in batch)))
            step = {}
            for k, v in eng.model.state_dict().items():
                step[f"w/{k}"] = v.detach().numpy().copy()
            for k, v in seen[-1].items():
                step[f"g/{k}"] = v
            for pname, prm in eng.model.named_parameters():
                pst = eng.optimizer.state.get(prm, {})
                for sk, tag in (("exp_avg", "m"), ("momentum_buffer", "m"), ("exp_avg_sq", "v"), ("square_avg", "v")):
                    if sk in pst:
                        step[f"{tag}/{pname}"] = pst[sk].detach().numpy().copy()
            path = os.path.join(OUT, f"{name}_s{s + 1}.npz")
            np.savez_compressed(path, **step)
            sizes.append(os.path.getsize(path))
            users.append(u), pos.append(p), neg.append(n), ptr.append(ptr[-1] + B)
    finally:
        ref_cmn.nn.utils.clip_grad_norm_ = orig_clip
    base.update(users=np.concatenate(users), pos=np.concatenate(pos), neg=np.concatenate(neg),
                batch_ptr=np.array(ptr, dtype=np.int64), losses=np.array(losses, dtype=np.float64),
                total_norms=np.array(norms, dtype=np.float64))
    # what every fixture must hold
    lens = np.diff(rowptr)
    used = set(np.concatenate(pos + neg).tolist())
    assert all(int(np.nonzero(lens == n)[0][0]) in used for n in (1, 2, 63, 64, 65, 300))
    assert set(pos[0].tolist()) & set(neg[0].tolist())
    assert all(0 in lists[i] for i in range(I) if len(lists[i]) >= 2)
    assert any(int(u) in lists[int(p)] for u, p in zip(users[0], pos[0]))
    assert BATCHES[-1] < BATCHES[0]
    print(f"{name}: optimizer {opt_name}, losses {losses}, total norms {norms} (grad_clip {grad_clip})")
    if hot:
        assert all(t > grad_clip for t in norms), f"{name}: the clip is not active"
    if name == "cmn_adam":
        assert all(t < grad_clip for t in norms), f"{name}: the clip is active"
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **base)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB + steps {[f'{s / 1024:.0f} KiB' for s in sizes]}")


def init_fixture(ref_cmn):
    """Seeded construction: the weights cmnEngine builds for a torch seed from given pre-trained tables."""
    out = {}
    for tag, (D, seed) in {"a": (8, 5), "b": (64, 2021)}.items():
        rng = np.random.default_rng(seed)
        lists = neighbourhoods(rng)
        ue = (rng.standard_normal((U, D)) * 0.01).astype(np.float32)
        ie = (rng.standard_normal((I, D)) * 0.01).astype(np.float32)
        torch.manual_seed(seed)
        eng = gu.quiet(ref_cmn.cmnEngine, config_for(D, "adam", 1e-4, 5.0), ue, ie, lists)
        rowptr, col = csr_of(lists)
        out[f"{tag}/meta"] = np.array([U, I, D, seed], dtype=np.int64)
        out[f"{tag}/rowptr"], out[f"{tag}/col"] = rowptr, col
        out[f"{tag}/user_embeddings"], out[f"{tag}/item_embeddings"] = ue, ie
        for k, v in eng.model.state_dict().items():
            if k not in ("user_memory.weight", "item_memory.weight"):     # those are the two inputs
                out[f"{tag}/w/{k}"] = v.detach().numpy().copy()
    np.savez_compressed(os.path.join(OUT, "cmn_init.npz"), **out)


def main():
    ref_cmn = import_reference()
    # cmn_default.json: D 64, Adam, lr 1e-4, weights as constructed (every ReLU unit active: the biases are 1.0)
    fixture(ref_cmn, "cmn_adam", 64, "adam", 1e-4, 31)
    # no optimizer name the base class knows: the constructor's RMSprop(lr, momentum 0.9) stays
    fixture(ref_cmn, "cmn_rmsprop_mom", 20, "default", 1e-4, 32)
    # width that is not a multiple of 64; weights of std 0.5 and zero biases: about half of every ReLU layer inactive,
    # gradients large enough for the clip to bite
    seed = next(sd for sd in range(33, 5000) if hot_seed_passes(sd, 100, 0.01, 5.0))
    print(f"cmn_sgd_hot_clip: seed {seed}")
    fixture(ref_cmn, "cmn_sgd_hot_clip", 100, "sgd", 0.01, seed, hot=True)
    init_fixture(ref_cmn)


if __name__ == "__main__":
    main()
