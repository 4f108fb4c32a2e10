"""GPU: the VAECF end-to-end example (synthetic frame -> loader -> epochs -> recommend -> hit rate) runs at a reduced
shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_vaecf_example_runs(hip_device):
    """Exit status 0, one JSON line, finite losses that fall over the epochs, held-out items ranked better than chance."""
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "vaecf_end_to_end.py"), "--users", "300", "--items", "200",
         "--groups", "5", "--per-user", "12", "--batch-size", "100", "--epochs", "8"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    print(res)
    losses = res["loss_per_epoch"]
    assert len(losses) == 8 and res["steps_per_epoch"] == 3
    assert all(np.isfinite(x) for x in losses)
    assert losses[-1] < losses[0]
    assert 0.0 < res["chance_hit_rate@10"] < res["hit_rate@10"] <= 1.0
