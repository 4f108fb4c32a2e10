"""csrc/lcfn.hip at its tile edges (tests/lcfn_edges.py) against the fp64 restatement, on the GPU."""
import numpy as np
import pytest
import torch

import lcfn_edges as le
import lcfn_numpy as lx
from helpers import assert_sgd_exact, assert_tensor_close, float64_oracle, to64
from test_lcfn_host import edge_engine

pytestmark = pytest.mark.gpu
NAMES = list(le.cases())


@pytest.mark.parametrize("name", NAMES)
def test_kernels_meet_the_fp64_restatement(hip_device, name):
    """One forward + backward: loss and parts at REL, every gradient as accurate as the fp32 restatement, nothing NaN;
    the all-embeddings tables against the fp64 propagation.  With all-zero tables the regulariser's gradient is 0."""
    case = le.make_case(name)
    eng = edge_engine(case, device_str="cuda:0")
    eng.model.train()
    loss, grads = eng.backward_only(case["batch"])
    g64 = le.check_step(case, loss, eng.last_losses(), grads, name)
    if not case["train_filters"]:
        for k in lx.tail_keys(case["L"]):
            assert float(grads[k].abs().max()) == 0.0, k
    with float64_oracle(lx):
        ua, ia = lx.lcfn_all_embeddings(to64(case["w"]), (case["P"], case["Q"]), case["hp"])
    U_f, I_f, _, _ = eng.model.ranking_factors()
    for got, ref, what in ((U_f, ua, "users"), (I_f, ia, "items")):
        print(f"  all-embeddings {what}: err {np.abs(got.cpu().numpy() - ref).max():.3e}")
        assert_tensor_close(got.cpu().numpy(), ref, what=f"{name} all-embeddings of {what}")
    if case.get("zero_tables"):
        assert float(np.abs(g64[lx.KEYS[0]]).max()) == 0.0 and float(grads[lx.KEYS[0]].abs().max()) == 0.0
        assert torch.isfinite(eng.model.flat).all()


@pytest.mark.parametrize("name", [n for n in NAMES if le.cases()[n].get("train_filters")])
def test_trained_filters_move_along_the_restatement(hip_device, name):
    """train_filters: two chained SGD steps; tables, filters and transformers every element within REL of the largest
    update of the fp32 restatement's trajectory, and the tail has moved."""
    case = le.make_case(name)
    lr = 0.05
    eng = edge_engine(case, optimizer="sgd", lr=lr, device_str="cuda:0")
    w = {k: v.copy() for k, v in case["w"].items()}
    st = lx.new_opt_state(w, "sgd")
    for _ in range(2):
        eng.train_single_batch(case["batch"])
        lx.lcfn_train_step(w, st, (case["P"], case["Q"]), case["hp"], case["batch"], "sgd", lr, train_filters=True)
    got = {**{k: v.detach().cpu().numpy() for k, v in eng.model.state_dict().items()},
           **{k: v.numpy() for k, v in eng.model.filter_state().items()}}
    assert_sgd_exact(got, w, case["w"], name)
    for k in lx.tail_keys(case["L"]):
        assert np.abs(got[k] - case["w"][k]).max() > 0, f"{k} did not move"
