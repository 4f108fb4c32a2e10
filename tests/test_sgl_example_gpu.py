"""GPU: the SGL end-to-end example (clustered log -> graph -> epochs with a sub-graph refresh each -> full-catalogue
ranking) runs and learns on data with planted structure."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sgl_example_learns(hip_device):
    """Full-catalogue NDCG@10 ends above the untrained model's; every epoch reports finite loss parts, the InfoNCE part
    among them."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import sgl_end_to_end
    finally:
        sys.path.pop(0)
    hist = sgl_end_to_end.main(["--users", "300", "--items", "200", "--interactions", "6000", "--emb-dim", "32",
                                "--epochs", "6"])
    print([(h["epoch"], h["loss"] and round(h["loss"], 4), round(h["ndcg@10"], 3)) for h in hist])
    assert len(hist) == 7 and hist[0]["epoch"] == -1 and hist[0]["loss"] is None
    assert all(np.isfinite(h["loss"]) and np.isfinite(h["last_parts"]).all() and h["last_parts"][2] > 0 for h in hist[1:])
    assert hist[-1]["ndcg@10"] > hist[0]["ndcg@10"], [h["ndcg@10"] for h in hist]
    assert 0.0 <= hist[-1]["recall@10"] <= 1.0
