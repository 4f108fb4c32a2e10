"""ETA without a GPU: the entry points are declared, prototyped and exported and refuse bad arguments before any HIP call, the
limits hold through ``hiprec_eta_param_floats``, the evidence group exists."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("hiprec_eta_param_floats", "hiprec_eta_workspace_bytes", "hiprec_eta_tiles", "hiprec_eta_grad",
           "hiprec_eta_retrieve", "hiprec_eta_attention")


def shape(**kw):
    from beta_recsys_amd import _lib

    s = dict(n_items=60, dim=64, maxlen=1024, hash_bits=64, top_k=48, num_heads=4, dnn_act=0, n_dnn=2, dnn=(200, 80, 0))
    s.update(kw)
    return ctypes.byref(_lib.EtaShape(*(s[n] for n in ("n_items", "dim", "maxlen", "hash_bits", "top_k", "num_heads", "dnn_act",
                                                        "n_dnn")), (ctypes.c_int32 * 3)(*s["dnn"])))


def test_entry_points_are_declared_prototyped_exported_and_validate():
    from beta_recsys_amd import _lib

    header = open(os.path.join(ROOT, "include", "hiprec.h")).read()
    lib = _lib.load()
    for name in ENTRIES:
        assert name + "(" in header and name in _lib.SIGNATURES and callable(getattr(lib, name)), name
    D, s, one = 64, shape(), ctypes.c_void_p(1)
    assert lib.hiprec_eta_param_floats(s) == 61 * D + 4 * (D * D + D) + 200 * 3 * D + 400 + 80 * 200 + 160 + 81
    out = (ctypes.c_int32 * 6)()
    assert lib.hiprec_eta_tiles(s, 4, out) == 0 and list(out) == [64, 2, 1, 192, 4, 6]
    assert lib.hiprec_eta_tiles(shape(dim=128, maxlen=4096, hash_bits=128), 100, out) == 0 and list(out)[2:4] == [0, 4096]
    assert lib.hiprec_eta_tiles(s, 4, None) == -1
    assert lib.hiprec_eta_workspace_bytes(s, (1 << 24) // 1024 + 1, 1, 0) == 0      # batch x maxlen
    assert lib.hiprec_eta_workspace_bytes(s, 1 << 10, (1 << 14) // 48 + 1, 0) == 0      # batch x n_cand x top_k
    assert 0 < lib.hiprec_eta_workspace_bytes(s, 2, 3, 0) < lib.hiprec_eta_workspace_bytes(s, 2, 3, 1)
    grad = lambda sh, w, b, ws: lib.hiprec_eta_grad(sh, w, one, None, one, 0, one, one, None, b, 1, one, one, None, 0, one, ws,  # noqa: E731
                                                    None)
    assert grad(shape(top_k=0), one, 1, 1 << 30) == -1 and b"top_k" in lib.hiprec_last_error()
    assert grad(s, None, 1, 1 << 30) == -1 and grad(s, one, 0, 1 << 30) == -1
    assert grad(s, one, 1, 16) == -1 and b"workspace" in lib.hiprec_last_error()
    assert lib.hiprec_eta_retrieve(s, one, one, one, None, 1, 1, one, one, one, one, 1 << 30, None) == -1
    assert lib.hiprec_eta_retrieve(s, one, one, one, one, 1, 1, one, one, one, one, 16, None) == -1
    assert lib.hiprec_eta_attention(s, one, one, one, None, 1, 1, one, None, None, None, None, one, 1 << 30, None) == -1
    assert lib.hiprec_eta_attention(s, one, one, one, one, 1, 1, one, one, None, None, None, one, 1 << 30, None) == -1
    assert b"backward" in lib.hiprec_last_error()


@pytest.mark.parametrize("bad", [dict(dim=24), dict(dim=144), dict(maxlen=0), dict(maxlen=4097), dict(hash_bits=0),
                                 dict(hash_bits=48), dict(hash_bits=160), dict(top_k=0), dict(top_k=129), dict(num_heads=0),
                                 dict(num_heads=3), dict(num_heads=32), dict(n_dnn=0), dict(n_dnn=4), dict(dnn=(513, 80, 0)),
                                 dict(dnn_act=2), dict(n_items=0)])
def test_limits_hold_through_param_floats(bad):
    from beta_recsys_amd import _lib

    lib = _lib.load()
    assert lib.hiprec_eta_param_floats(shape(**bad)) == -1 and lib.hiprec_last_error()
    assert lib.hiprec_eta_workspace_bytes(shape(**bad), 4, 4, 1) == 0


def test_evidence_group_and_model():
    import __graft_entry__ as ge
    import beta_recsys_amd as hp

    group = ge.EVIDENCE_GROUPS["eta"]
    assert {"eta.hip", "din.hip", "din.hpp", "ncf.hip", "gemm.hpp"} <= set(group)
    assert all(os.path.exists(os.path.join(ge.CSRC, n)) for n in group)
    assert ge.evidence_group("eta_step") == "eta" and ge.evidence_group("dien_step") == "dien"
    with pytest.raises(ValueError, match="hash_bits"):
        hp.ETA(dict(n_items=10, emb_dim=16, maxlen=8, hash_bits=40))
    assert hp.ETAEngine.__mro__[1].__name__ == "_RankingEngine"
    sd = hp.ETA(dict(n_items=10, emb_dim=16, maxlen=300)).state_dict()
    assert tuple(sd["hash.weight"].shape) == (64, 16) and float(sd["item_emb.weight"][0].abs().max()) == 0.0
