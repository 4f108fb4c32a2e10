"""GPU: the MixGCF end-to-end example (graph -> candidate batches -> training steps in csrc/mixgcf.hip -> full-catalogue
ranking) runs and learns on data with planted structure."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mixgcf_example_learns(hip_device):
    """Full-catalogue NDCG@10 ends above the untrained model's by at least 0.2 and the mean step loss falls.  The numpy
    restatement, trained on the CPU from the same weights, batches and seeds, gains 0.34 (0.045 -> 0.386) with the loss
    going 0.693 -> 0.644: see the example's docstring."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import mixgcf_end_to_end
    finally:
        sys.path.pop(0)
    hist = mixgcf_end_to_end.main(["--users", "300", "--items", "200", "--interactions", "6000", "--emb-dim", "32",
                                   "--epochs", "6"])
    print([(h["epoch"], h["loss"] and round(h["loss"], 4), round(h["ndcg@10"], 3)) for h in hist])
    assert len(hist) == 7 and hist[0]["epoch"] == -1 and hist[0]["loss"] is None
    assert hist[-1]["loss"] < hist[1]["loss"]
    assert hist[-1]["ndcg@10"] >= hist[0]["ndcg@10"] + 0.2, [h["ndcg@10"] for h in hist]
    assert 0.0 <= hist[-1]["recall@10"] <= 1.0
