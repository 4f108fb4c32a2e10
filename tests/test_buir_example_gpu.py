"""GPU: the BUIR end-to-end example (clustered log -> graph -> DeviceTripleBatcher epochs -> top-K over the whole catalogue
through ranking_factors) runs and its loss falls, with the frozen target and with the moving one."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("argv", [[], ["--update-target", "--epochs", "3"]])
def test_buir_example_runs_and_its_loss_falls(hip_device, argv):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import buir_end_to_end
    finally:
        sys.path.pop(0)
    hist, top, (tr_u, tr_i) = buir_end_to_end.main(argv)
    print([(h["epoch"], round(h["loss"], 4)) for h in hist])
    assert len(hist) >= 3 and all(np.isfinite(h["loss"]) for h in hist)
    assert hist[-1]["loss"] < hist[0]["loss"], [h["loss"] for h in hist]
    # ten distinct items per user, none of them a training item of that user
    seen = set(zip(tr_u.tolist(), tr_i.tolist()))
    assert top.shape == (300, 10)
    for u in range(top.shape[0]):
        assert len(set(top[u])) == 10 and not any((u, int(i)) in seen for i in top[u]), f"user {u}"
