"""GPU: the CMN end-to-end example (PairwiseGMF pre-training -> tables handed to cmnEngine -> resident epochs on the
item -> users CSR -> full-catalogue evaluation -> recommendations) runs at a small shape."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cmn_example_runs_both_halves(hip_device):
    """Both stages report finite, falling losses, the evaluation and the recommendations come back well-formed.  No
    ranking bar: as in the reference, ``predict`` is the plain dot product M[u] . E[i], which neither stage's loss
    trains directly (PairwiseGMF scores v . (M[u] * E[i]), CMN scores through the memory network)."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import cmn_end_to_end
    finally:
        sys.path.pop(0)
    hist, rec = cmn_end_to_end.main(["--users", "400", "--items", "300", "--interactions", "20000", "--emb-dim", "32",
                                     "--batch-size", "512", "--pretrain-epochs", "3", "--epochs", "3", "--lr", "0.005",
                                     "--top", "5"])
    print(hist)
    gmf = [h for h in hist if h["stage"] == "pairwise_gmf"]
    cmn = [h for h in hist if h["stage"] == "cmn"]
    assert len(gmf) == 3 and len(cmn) == 3
    assert all(np.isfinite(h["loss"]) for h in hist)
    assert gmf[-1]["loss"] < gmf[0]["loss"] and cmn[-1]["loss"] < cmn[0]["loss"]
    assert cmn[0]["max_neighbors"] > 64                   # lists beyond one wave's worth of rows
    assert all(0.0 <= h["recall@20"] <= 1.0 and 0.0 <= h["ndcg@10"] <= 1.0 for h in cmn)
    assert rec.shape == (3, 5) and (rec >= 0).all() and (rec < 300).all()
