"""GPU: the SimGCL end-to-end example (clustered log -> graph -> DeviceTripleBatcher epochs with the device draw ->
full-catalogue ranking of the raw tables) runs and learns on data with planted structure."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_simgcl_example_learns(hip_device):
    """On its small default, full-catalogue NDCG@10 after training is above the untrained model's; every epoch reports
    finite loss parts."""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import simgcl_end_to_end
    finally:
        sys.path.pop(0)
    hist = simgcl_end_to_end.main([])
    print([(h["epoch"], h["loss"] and round(h["loss"], 4), round(h["ndcg@10"], 3)) for h in hist], hist[0]["chance_ndcg@10"])
    assert hist[0]["epoch"] == -1 and hist[0]["loss"] is None and len(hist) >= 2
    assert all(np.isfinite(h["loss"]) and np.isfinite(h["last_parts"]).all() for h in hist[1:])
    assert hist[-1]["ndcg@10"] > hist[0]["ndcg@10"], [h["ndcg@10"] for h in hist]
    assert 0.0 <= hist[-1]["recall@10"] <= 1.0
