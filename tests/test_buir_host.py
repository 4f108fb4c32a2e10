"""CPU: planted defects.  Each entry of buir_numpy.DEFECTS is a deliberately wrong BUIR step; the checks the golden and
edge tests apply to the product -- loss to REL, gradients to REL of scale, zero gradient into the target, predict to REL of
scale, everything finite -- must reject every one of them on the inputs those tests use, and pass the step without a
defect."""
import numpy as np
import pytest

import buir_edges as edges
import buir_numpy as bx
from helpers import REL, float64_oracle, load_golden, to64
from test_oracle_golden_buir import bu_batch, bu_graph, bu_meta, bu_params


def violations(defect):
    """What the checks find wrong with a step that carries ``defect`` (None: the step as the reference has it)."""
    found = []
    g = load_golden("buir_adam")
    m, graph = bu_meta(g), bu_graph(g)
    w0 = bu_params(g, "w0")
    loss, grads = bx.buir_grads(w0, graph, m["L"], bu_batch(g, 0), defect=defect)
    if abs(loss - g["losses"][0]) > REL * abs(g["losses"][0]):
        found.append("loss")
    for k in bx.TRAINABLE:
        ref = g[f"g1/{k}"]
        if np.abs(grads[k] - ref).max() > REL * np.abs(ref).max():
            found.append(f"grad {k}")
    if any(grads[k].any() for k in bx.TARGET):
        found.append("a gradient reached the target")
    w3 = bu_params(g, f"w{m['n_steps']}")
    got = bx.buir_predict(w3, graph, m["L"], g["predict_users"], g["predict_items"], defect=defect)
    if np.abs(got - g["predict_scores"]).max() > REL * np.abs(g["predict_scores"]).max():
        found.append("predict")
    # the edge case with all-zero target rows, against the step as the reference has it in fp64
    c = edges.build("d100_l1_zero_target")
    with float64_oracle(bx):
        l64, g64 = bx.buir_grads(to64(c["w"]), c["graph"], c["L"], c["batch"])
    loss, grads = bx.buir_grads(c["w"], c["graph"], c["L"], c["batch"], defect=defect)
    if not (np.isfinite(loss) and all(np.isfinite(v).all() for v in grads.values())):
        found.append("not finite on a zero target row")
    elif abs(loss - l64) > REL * abs(l64):
        found.append("edge loss")
    return found


def test_the_step_without_a_defect_passes_every_check():
    assert violations(None) == []


@pytest.mark.parametrize("defect", bx.DEFECTS)
def test_planted_defect_is_caught(defect):
    found = violations(defect)
    print(defect, "->", found)
    assert found, f"{defect}: no check noticed"
    expect = {"no_layer0": "loss", "divide_by_l": "grad", "two_predictors": "loss", "targets_swapped": "loss",
              "target_gradient": "a gradient reached the target", "predict_from_target": "predict",
              "no_clamp": "not finite on a zero target row"}[defect]
    assert any(f.startswith(expect) for f in found), (defect, found)


def test_the_edge_builder_holds_what_it_promises():
    assert {c[2] for c in edges.CASES.values()} >= {1, edges.TB - 1, edges.TB, edges.TB + 1, 2 * edges.TB + 3}
    assert {c[0] for c in edges.CASES.values()} >= {1, 3, 4, 5, 16, 64, 100, 256}
    assert {c[1] for c in edges.CASES.values()} == {1, 2, 3, 4}
    c = edges.build("d100_l1_zero_target")
    users, pos, _ = c["batch"]
    lu, li = c["U"] - c["n_iso"], c["I"] - c["n_iso"]
    rows, cols, _, _ = c["graph"]
    touched = set(rows.tolist()) | set(cols.tolist())
    assert all(n not in touched for n in list(range(lu, c["U"])) + [c["U"] + i for i in range(li, c["I"])])
    assert set(range(lu, c["U"])) <= set(users.tolist()) and set(range(li, c["I"])) <= set(pos.tolist())
    assert not c["w"][bx.TARGET[0]][lu:].any() and not c["w"][bx.TARGET[1]][li:].any()
    assert ((users == c["U"] - 1) & (pos == c["I"] - 1)).any(), "one pair has both target rows zero"
    r = edges.build("d64_l2_repeated_pair")["batch"]
    assert len(set(r[0])) == 1 and len(set(r[1])) == 1 and r[0].size == edges.TB + 1
