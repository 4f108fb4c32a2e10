"""CPU companion of tests/test_mixgcf_edges_gpu.py: the fp32 restatement itself meets both rules of tests/mixgcf_edges.py
on every case, and every case can see the defects it is there for."""
import numpy as np
import pytest

import mixgcf_edges as me
import mixgcf_numpy as mx


def fp32_step(case, seeds=None, choice=None, defect=None):
    return mx.mix_grads(case["w"], case["graph"], case["hp"], case["batch"], case["seeds"] if seeds is None else seeds,
                        case["masks"], choice=choice, defect=defect)


@pytest.mark.parametrize("name", me.CASE_NAMES)
def test_fp32_restatement_meets_both_rules(name):
    case = me.make_case(name)
    loss, grads, choice = fp32_step(case)
    me.check_choice(case, choice, name)
    me.check_step(case, loss, grads, choice, name)
    x_spread = np.abs(mx.mix_predict(case["w"], case["graph"], case["hp"], case["batch"][0], case["batch"][1])).max()
    assert 0.05 < x_spread < 20, f"{name}: scores of size {x_spread}"


def test_cases_cover_the_shapes():
    cols = list(zip(*me.CASES))
    assert set(cols[1]) == {1, 7, 20, 64, 65, 128, 200, 256} and {1, 3, me.MAX_L} <= set(cols[2])
    assert {1, 2, 64, 65} <= set(cols[3]) and set(cols[4]) == {1, 2, 4} and {1, 5, 257} == set(cols[5])
    assert set(cols[6]) == set(mx.POOLS)
    for name in me.CASE_NAMES:
        case = me.make_case(name)
        U, I = case["U"], case["I"]
        rows, cols_, _, N = case["graph"]
        deg = np.bincount(rows, minlength=N)
        assert deg[U] == U + 1 and (deg[U + I - 3:] == 1).all()            # the hub; items with their self loop only
        cand = mx.candidates(case["batch"][2], case["hp"])
        if cand.shape[2] >= 2 and name != "same_item_row":
            assert (cand[:, :, 0] == 0).all() and (cand[:, :, 1] >= I - 3).all()
    assert len(set(me.make_case("one_user_b257")["batch"][0])) == 1
    c = me.make_case("same_item_row")
    assert len(set(c["batch"][2][c["B"] // 2])) == 1
    c = me.make_case("cand_is_pos")
    assert (c["batch"][2][:, -1] == c["batch"][1]).all()


@pytest.mark.parametrize("name", [n for n in me.CASE_NAMES if n != "rns_lmax"])
def test_a_seed_on_the_wrong_hop_is_seen(name):
    case = me.make_case(name)
    _, _, choice = fp32_step(case)
    loss, grads, _ = fp32_step(case, seeds=np.roll(case["seeds"], 1, axis=2), choice=choice)
    with pytest.raises(AssertionError):
        me.check_step(case, loss, grads, choice, name)


@pytest.mark.parametrize("name", [n for n in me.CASE_NAMES if n != "rns_lmax"])   # (rns mixes nothing: the forms coincide)
@pytest.mark.parametrize("defect", ["drop_pos_seed_term", "reg_unmixed"])
def test_planted_gradient_defects_are_seen(name, defect):
    case = me.make_case(name)
    _, _, choice = fp32_step(case)
    loss, grads, _ = fp32_step(case, choice=choice, defect=defect)
    with pytest.raises(AssertionError):
        me.check_step(case, loss, grads, choice, name)


@pytest.mark.parametrize("name", me.CASE_NAMES)
def test_a_lost_tail_column_and_a_lost_row_are_seen(name):
    """What a wrong tail-lane mask or a dropped last batch row would do to the gradient."""
    case = me.make_case(name)
    loss, grads, choice = fp32_step(case)
    g2 = {k: v.copy() for k, v in grads.items()}
    g2["item_embedding.weight"][:, -1] = 0
    with pytest.raises(AssertionError):
        me.check_step(case, loss, g2, choice, name)
    if case["B"] > 1:
        short = dict(case, batch=tuple(a[:-1] for a in case["batch"]), seeds=case["seeds"][:-1])
        l3, g3, _ = fp32_step(short, choice=choice[:-1])
        g3 = {k: v * np.float32((case["B"] - 1) / case["B"]) for k, v in g3.items()}   # the other rows, weighted as in B
        with pytest.raises(AssertionError):
            me.check_step(case, loss, g3, choice, name)


def test_choice_rule_takes_either_copy_and_refuses_another_item():
    case = me.make_case("same_item_row")
    _, _, choice = fp32_step(case)
    b = case["B"] // 2
    other_copy = choice.copy()
    other_copy[b] = case["hp"]["n_negs"] - 1
    assert me.check_choice(case, other_copy) == 0
    sc, _, cand = me.exact_scores(case)
    wrong = choice.copy()
    wrong[0, 0, 0] = int(sc[0, 0, :, 0].argmin())
    assert cand[0, 0, wrong[0, 0, 0]] != cand[0, 0, choice[0, 0, 0]]
    with pytest.raises(AssertionError, match="not the maximum"):
        me.check_choice(case, wrong)
    # the lowest index wins an exact tie
    assert (choice[b] == 0).all()
