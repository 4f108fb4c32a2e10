"""Host-side logic of the MixGCF mirror (no GPU): config validation, the COO-order permutation of the edge masks, the
ctypes plan layout, and the recorded deviation from the reference's train step."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

import mixgcf_numpy as mx
from helpers import load_golden
from test_oracle_golden_mixgcf import CASES, KEYS, mix_batch, mix_graph, mix_hp, mix_masks, mix_meta, mix_params


def adj_tensor(g):
    rows, cols, vals, N = mix_graph(g)
    return torch.sparse_coo_tensor(torch.from_numpy(np.vstack([rows, cols])), torch.from_numpy(vals), (N, N))


def model_config(g, **over):
    m, hp = mix_meta(g), mix_hp(g)
    cfg = dict(n_users=m["U"], n_items=m["I"], emb_dim=m["D"], pool=hp["pool"], context_hops=m["L"],
               mess_dropout=hp["mess_rate"] is not None, mess_dropout_rate=hp["mess_rate"] or 0.1,
               edge_dropout=hp["edge_rate"] is not None, edge_dropout_rate=hp["edge_rate"] or 0.5,
               norm_adj=adj_tensor(g), l2=hp["l2"], n_negs=hp["n_negs"], ns=hp["ns"], K=hp["K"],
               optimizer=str(g["optimizer"]), lr=float(g["lr"]), device_str="cpu", batch_size=m["B"])
    cfg.update(over)
    return cfg


def make_engine(g, **over):
    import beta_recsys_amd as hp

    with contextlib.redirect_stdout(io.StringIO()):
        return hp.MixGCFEngine({"model": model_config(g, **over), "system": {"run_dir": "/tmp/hiprec_test_runs"}})


def test_config_is_validated():
    g = load_golden("mix_concat_adam")
    eng = make_engine(g)
    assert list(eng.model.state_dict()) == list(KEYS)
    for over, text in (({"pool": "max"}, "pool"), ({"ns": "dns"}, "ns"), ({"K": 0}, "K"), ({"n_negs": 0}, "n_negs"),
                       ({"context_hops": 7}, "context_hops"), ({"emb_dim": 257}, "emb_dim"),
                       ({"K": 17}, "K * (context_hops + 1)"), ({"dropout_rng": "numpy"}, "dropout_rng"),
                       ({"seed_rng": "numpy"}, "seed_rng"), ({"edge_dropout": True, "edge_dropout_rate": 1.0}, "edge_dropout_rate")):
        with pytest.raises(ValueError, match=text.replace("*", r"\*").replace("(", r"\(").replace(")", r"\)").replace("+", r"\+")):
            make_engine(g, **over)
    m = mix_meta(g)
    users, pos, neg = mix_batch(g, 0)
    with pytest.raises(ValueError, match="K \\* n_negs"):
        eng._batch((users, pos, neg[:, : m["K"] * m["n_negs"] - 1]))
    with pytest.raises(ValueError, match="empty batch"):
        eng._batch((users[:0], pos[:0], neg[:0]))
    with pytest.raises(ValueError, match="differ in length"):
        eng._batch((users, pos[:-1], neg))
    rns = make_engine(load_golden("mix_rns_sgd"))
    with pytest.raises(ValueError, match="n >= 2 \\(K\\)"):
        rns._batch((users, pos, neg[:, :1]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.train_single_batch((users, pos, neg))


def test_same_seed_gives_the_references_initial_weights():
    g = load_golden("mix_mean_sgd_drop")
    m = mix_meta(g)
    torch.manual_seed(5)
    a = make_engine(g).model.state_dict()
    torch.manual_seed(5)
    u, i = torch.nn.Embedding(m["U"], m["D"]), torch.nn.Embedding(m["I"], m["D"])
    torch.nn.init.xavier_uniform_(u.weight)
    torch.nn.init.xavier_uniform_(i.weight)
    assert torch.equal(a["user_embedding.weight"], u.weight.data) and torch.equal(a["item_embedding.weight"], i.weight.data)


@pytest.mark.parametrize("case", ["mix_mean_sgd_drop", "mix_final_adam_hot"])
def test_edge_masks_follow_the_coo_order_as_passed(case):
    """The fixtures' norm_adj is a deliberately unsorted COO and their edge masks are in that order.  The mirror's CSR
    edge e is COO entry order[e]; the transposed CSR's edge t is forward edge eid_t[t]."""
    g = load_golden(case)
    rows, cols, vals, N = mix_graph(g)
    assert np.any(np.diff(rows * N + cols) < 0), "the fixture's COO order is sorted"
    model = make_engine(g).model
    gr = model.graph()
    order = gr["order"].numpy()
    rp, col, val = gr["rowptr"].numpy(), gr["col"].numpy(), gr["val"].numpy()
    csr_row = np.repeat(np.arange(N), np.diff(rp))
    assert np.array_equal(csr_row, rows[order]) and np.array_equal(col, cols[order]) and np.array_equal(val, vals[order])
    rpt, colt, eid_t = gr["rowptr_t"].numpy(), gr["col_t"].numpy(), gr["eid_t"].numpy()
    t_row = np.repeat(np.arange(N), np.diff(rpt))
    assert np.array_equal(csr_row[eid_t], colt) and np.array_equal(col[eid_t], t_row)
    # a hop built from the CSR with keep bytes permuted this way is the restatement's hop under the COO-order mask
    keep_coo = g["edge_keep"][0][0]
    keep_csr = keep_coo[order]
    A = np.zeros((N, N), dtype=np.float32)
    scale = np.float32(1.0 / (1 - mix_hp(g)["edge_rate"]))
    A[csr_row, col] = np.where(keep_csr != 0, val * scale, 0)
    assert np.array_equal(A, mx.hop_matrix((rows, cols, vals, N), keep_coo, mix_hp(g)["edge_rate"]))
    At = np.zeros((N, N), dtype=np.float32)
    At[t_row, colt] = np.where(keep_csr[eid_t] != 0, gr["val_t"].numpy() * scale, 0)
    assert np.array_equal(At, A.T)


def test_repeated_coordinates_are_rejected():
    g = load_golden("mix_rns_sgd")
    rows, cols, vals, N = mix_graph(g)
    idx = torch.from_numpy(np.vstack([np.append(rows, rows[3]), np.append(cols, cols[3])]))
    adj = torch.sparse_coo_tensor(idx, torch.from_numpy(np.append(vals, vals[3])), (N, N))
    model = make_engine(g, norm_adj=adj).model
    with pytest.raises(ValueError, match="repeated coordinates"):
        model.graph()
    with pytest.raises(ValueError, match="expected"):
        make_engine(g, norm_adj=torch.sparse_coo_tensor(idx[:, :2], torch.ones(2), (N + 1, N + 1))).model.graph()


def test_plan_struct_matches_the_library():
    from beta_recsys_amd import _lib

    lib = _lib.load()
    assert lib.hiprec_mixgcf_plan_bytes() == ctypes.sizeof(_lib.MixGcfPlan)
    assert _lib.MIXGCF_MAX_HOPS == 6 and _lib.MIXGCF_POOLS == {"concat": 0, "mean": 1, "sum": 2, "final": 3}
    p = _lib.MixGcfPlan()
    rc = lib.hiprec_mixgcf_propagate(ctypes.byref(p), 0, None)      # validated before any HIP call
    assert rc == -1 and lib.hiprec_last_error()
    assert lib.hiprec_mixgcf_grad(None, None, None, None, 0, 0, None, None, 0.0, None, None, 0, None) == -1


@pytest.mark.parametrize("case", CASES)
def test_the_references_step_moves_nothing_and_the_mirrors_does(case):
    """The deviation the mirror records: after the reference's own train_single_batch the weights are bit for bit what
    they were (it returns the loss tensor and never steps); the step of the restatement -- the gradient of that loss,
    then the optimizer -- moves them to where autograd and torch.optim on the reference's loss moved them."""
    g = load_golden(case)
    hp, graph = mix_hp(g), mix_graph(g)
    w0 = mix_params(g, "w0")
    for k in KEYS:
        assert np.array_equal(g[f"ref_after_step/{k}"], w0[k])
    w = {k: v.copy() for k, v in w0.items()}
    st = mx.new_opt_state(w, str(g["optimizer"]))
    mx.mix_train_step(w, st, graph, hp, mix_batch(g, 0), g["seeds"][0], mix_masks(g, 0), str(g["optimizer"]), float(g["lr"]))
    for k in KEYS:
        moved = np.abs(w[k] - w0[k]).max()
        assert moved > 0 and np.abs(w[k] - g[f"w1/{k}"]).max() <= 0.02 * moved + 1e-7
