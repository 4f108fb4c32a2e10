"""ORACLE tooling (test infrastructure): capture the VAECF golden vectors from the REAL reference.

Runs only where the reference tree exists (REFERENCE_ROOT, default: where oracle/gen_golden.py looks); the reference
itself never travels -- only the small .npz fixtures written to tests/golden/vaecf_*.npz do.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_vaecf.py

Imports ``beta_rec.models.vaecf`` with the in-process shims of ``tools/gen_golden_ultragcn.py`` and drives the reference's
own ``VAECFEngine.train_single_batch`` on the CPU, three steps per case.  The two-hidden-layer case swaps a
``VAE(z_dim, ae_structure, config)`` built directly (and an Adam over its parameters) into the engine, which hard-codes
``z_dim = 10`` and one hidden layer of 20.

The reference's base class replaces the engine's ``Adam(lr, weight_decay)`` by ``config["model"]["optimizer"]`` at ``lr``
alone when that string is sgd / adam / rmsprop (torch_engine.py:16, 23-39).  The cases with a weight decay therefore carry
an optimizer string outside those three, which leaves vaecf.py:128-130's optimizer in place; the fixture records the
string.

The scipy installed here has no ``.A`` on sparse matrices, which the reference's ``train_an_epoch`` and ``predict`` use:
for those two calls an ``A`` property that returns ``toarray()`` is added in process, and the fixture records that
(``patched_A``).

A fixture is ``vaecf_<case>.npz`` (shapes, hyper-parameters, the constructed weights ``winit`` for the fixture's torch
seed, the initial weights ``w0`` = ``winit`` after ``vaecf_edges.condition``, every step's dense batch, its ``eps`` as
captured from ``torch.randn_like``, the RNG state in front of it, the losses and their two parts, one ``predict`` call
with a duplicate pair and pairs of other users) plus one ``vaecf_<case>_s<k>.npz`` per step (its gradients as they stand
at ``optimizer.step``, the weights and Adam's moments after it).  ``vaecf_mult_tanh`` also holds one epoch over a 9-user
matrix at batch size 6 (a short last batch): the printed line and the logged scalar.

Asserted here at every step, with the figures printed: the batch layout of ``vaecf_edges.check_batch``; in the fp64
evaluation every pre-activation at least ``MIN_PRE`` away from 0 and 6 and ``|logvar| <= MAX_LOGVAR``; the reference's
gradients within ``helpers.REL`` of their scale of the fp64 ones.
"""
import contextlib
import io
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

N_STEPS = 3
U, I = 9, 11
CASES = [  # name, likelihood, activation, weight_decay, config optimizer, batch, config batch_size, (z, hidden), lr, beta, seed
    ("vaecf_mult_tanh", "mult", "tanh", 0.0, "adam", 6, 6, None, 0.05, 1.0, 100),
    ("vaecf_bern_relu_wd", "bern", "relu", 0.01, "vaecf", 6, 6, None, 0.001, 0.5, 200),
    ("vaecf_gaus_sigmoid_short", "gaus", "sigmoid", 0.0, "adam", 4, 6, None, 0.01, 0.2, 300),
    ("vaecf_pois_relu6", "pois", "relu6", 0.001, "vaecf", 6, 6, None, 0.001, 0.2, 400),
    ("vaecf_mult_two_layers", "mult", "tanh", 0.0, "adam", 6, 6, (5, [12, 7]), 0.02, 0.2, 500),
]
PREDICT_PAIRS = (np.array([0, 0, 2, 0, 5]), np.array([3, 3, 7, 1, 4]))      # (0, 3) twice; users 2 and 5


def import_reference():
    gu.import_reference()                                    # shims + sys.path
    from beta_rec.models import vaecf as ref

    return ref


@contextlib.contextmanager
def sparse_A():
    """``.A`` on scipy's csr_matrix for the duration of a reference call that needs it."""
    from scipy.sparse import csr_matrix

    had = hasattr(csr_matrix, "A")
    if not had:
        csr_matrix.A = property(lambda self: self.toarray())
    try:
        yield not had
    finally:
        if not had:
            del csr_matrix.A


def config_for(likelihood, activation, wd, optimizer, batch_size, lr, beta):
    return {"model": {"n_users": U, "n_items": I, "activation": activation, "likelihood": likelihood,
                      "batch_size": batch_size, "lr": lr, "beta": beta, "weight_decay": wd, "optimizer": optimizer,
                      "device_str": "cpu"},
            "system": {"run_dir": "/tmp/hiprec_golden_runs"}}


def build_engine(ref, cfg, arch, seed):
    torch.manual_seed(seed)
    if arch is None:
        return gu.quiet(ref.VAECFEngine, cfg)
    model = ref.VAE(arch[0], [I] + arch[1], cfg["model"])   # first: the seed's draws go to this model
    eng = gu.quiet(ref.VAECFEngine, cfg)
    eng.model = model
    eng.model.device = eng.device
    eng.optimizer = torch.optim.Adam(model.parameters(), lr=eng.lr, weight_decay=eng.wd)
    return eng


def fixture(ref, name, likelihood, activation, wd, optimizer, B, batch_size, arch, lr, beta, seed):
    import vaecf_edges as ve
    import vaecf_numpy as vn
    from helpers import REL, float64_oracle, to64

    rng = np.random.default_rng(seed)
    cfg = config_for(likelihood, activation, wd, optimizer, batch_size, lr, beta)
    eng = build_engine(ref, cfg, arch, seed)
    assert isinstance(eng.optimizer, torch.optim.Adam) and eng.optimizer.defaults["weight_decay"] == wd
    z_dim, hidden = (10, [20]) if arch is None else arch
    KEYS = vn.keys(len(hidden))
    assert tuple(eng.model.state_dict()) == KEYS == tuple(n for n, _ in eng.model.named_parameters())
    winit = {k: v.detach().numpy().copy() for k, v in eng.model.state_dict().items()}
    w0 = ve.condition({k: v.copy() for k, v in winit.items()})
    with torch.no_grad():
        for k, prm in eng.model.named_parameters():
            prm.copy_(torch.from_numpy(w0[k]))
    base = {"meta": np.array([U, I, z_dim, B, batch_size, N_STEPS, seed] + hidden, dtype=np.int64),
            "likelihood": np.array(likelihood), "activation": np.array(activation), "optimizer": np.array(optimizer),
            "weight_decay": np.array(wd), "lr": np.array(lr), "beta": np.array(beta)}
    for k in KEYS:
        base[f"w0/{k}"] = w0[k]
        base[f"winit/{k}"] = winit[k]

    # predict, from w0 (vaecf.py:89-108)
    with sparse_A() as patched:
        pred = eng.model.predict(PREDICT_PAIRS[0], PREDICT_PAIRS[1])
    base.update(predict_users=PREDICT_PAIRS[0], predict_items=PREDICT_PAIRS[1], predict_out=pred.numpy().copy(),
                patched_A=np.array(patched))

    if name == "vaecf_mult_tanh":                          # one epoch from w0, then back to w0
        matrix_dense = ve.make_x(rng, U, I)
        from scipy.sparse import csr_matrix

        state = torch.get_rng_state()
        out = io.StringIO()
        n_before = len(eng.writer.scalars)
        with sparse_A(), contextlib.redirect_stdout(out):
            eng.train_an_epoch((np.arange(U), csr_matrix(matrix_dense * 3.0)), 7)    # the loop binarises the 3s
        logged = eng.writer.scalars[n_before:]
        assert len(logged) == 1 and logged[0][0] == "model/loss" and logged[0][2] == 7
        base.update(epoch_matrix=matrix_dense, epoch_rng_state=state.numpy().copy(), epoch_loss=np.array(logged[0][1]),
                    epoch_printed=np.array(out.getvalue().strip()))
        for k, v in eng.model.state_dict().items():
            base[f"epoch_w/{k}"] = v.detach().numpy().copy()
        print(f"{name}: epoch prints {out.getvalue().strip()!r}")
        eng = build_engine(ref, cfg, arch, seed)
        with torch.no_grad():
            for k, prm in eng.model.named_parameters():
                prm.copy_(torch.from_numpy(w0[k]))

    seen, drawn, latent = [], [], []
    orig_step = eng.optimizer.step

    def capturing_step(*a, **k):
        seen.append({n: prm.grad.detach().numpy().copy() for n, prm in eng.model.named_parameters()})
        return orig_step(*a, **k)

    eng.optimizer.step = capturing_step
    orig_randn_like = torch.randn_like

    def capturing_randn_like(x, *a, **k):
        out = orig_randn_like(x, *a, **k)
        drawn.append(out.detach().numpy().copy())
        return out

    orig_loss = eng.model.loss

    def capturing_loss(x, x_, mu, logvar, beta_):
        latent.append((mu.detach().clone(), logvar.detach().clone()))
        return orig_loss(x, x_, mu, logvar, beta_)

    eng.model.loss = capturing_loss
    losses, lls, klds, replay_ok, sizes, xs = [], [], [], [], [], []
    torch.randn_like = capturing_randn_like
    try:
        for s in range(N_STEPS):
            x = ve.make_x(rng, B, I)
            ve.check_batch(x)
            w_now = {k: v.detach().numpy().copy() for k, v in eng.model.state_dict().items()}
            del drawn[:], latent[:]
            state = torch.get_rng_state()
            loss = eng.train_single_batch(torch.from_numpy(x))
            assert len(drawn) == 1 and drawn[0].shape == (B, z_dim)
            after = torch.get_rng_state()
            torch.set_rng_state(state)
            replay_ok.append(np.array_equal(torch.randn(B, z_dim).numpy(), drawn[0]))
            torch.set_rng_state(after)
            base[f"rng_state{s}"] = state.numpy().copy()
            base[f"eps{s}"] = drawn[0]
            mu, logvar = latent[0]
            std = torch.exp(0.5 * logvar)
            kld = float((-0.5 * (1 + 2.0 * torch.log(std) - mu.pow(2) - std.pow(2))).sum(1).mean())
            ll = beta * kld - loss
            with float64_oracle(vn):
                l64, ll64, kld64, g64, info = vn.vaecf_grads(to64(w_now), x, drawn[0], beta, activation, likelihood)
            worst = max(float(np.abs(seen[-1][k] - g64[k]).max() / np.abs(g64[k]).max()) for k in KEYS)
            print(f"{name} step {s}: loss {loss:.6f} (fp64 restatement {l64:.6f}), ll {ll:.6f} ({ll64:.6f}), kld "
                  f"{kld:.6f} ({kld64:.6f}); min |pre| {info['min_abs_pre']:.3f}, min |pre - 6| "
                  f"{info['min_abs_pre_minus_6']:.3f}, max |logvar| {info['max_abs_logvar']:.3f}, max |z| "
                  f"{info['max_abs_z']:.2f}; the reference's gradients are within {worst:.2e} of their scale of the "
                  f"exact ones")
            assert ve.margins_ok(info, activation)
            assert worst <= REL
            assert abs(loss - l64) <= REL * abs(l64)
            losses.append(float(loss)), lls.append(ll), klds.append(kld)
            step = {}
            for k, v in eng.model.state_dict().items():
                step[f"w/{k}"] = v.detach().numpy().copy()
            for k, v in seen[-1].items():
                step[f"g/{k}"] = v
            for pname, prm in eng.model.named_parameters():
                pst = eng.optimizer.state.get(prm, {})
                for sk, tag in (("exp_avg", "m"), ("exp_avg_sq", "v")):
                    step[f"{tag}/{pname}"] = pst[sk].detach().numpy().copy()
            path = os.path.join(OUT, f"{name}_s{s + 1}.npz")
            np.savez_compressed(path, **step)
            sizes.append(os.path.getsize(path))
            xs.append(x)
    finally:
        torch.randn_like = orig_randn_like
    base.update(x=np.stack(xs), losses=np.array(losses), lls=np.array(lls), klds=np.array(klds),
                replay_ok=np.array(replay_ok))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **base)
    print(f"{name}: losses {losses}; one torch.randn from the step's RNG state reproduces eps in {sum(replay_ok)} of "
          f"{len(replay_ok)} steps; predict -> {pred.numpy()}")
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB + steps {[f'{s / 1024:.0f} KiB' for s in sizes]}")
    assert max(sizes + [os.path.getsize(path)]) < 500_000


def main():
    ref = import_reference()
    for case in CASES:
        fixture(ref, *case)


if __name__ == "__main__":
    main()
