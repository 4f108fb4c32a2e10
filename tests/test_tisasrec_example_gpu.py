"""GPU: the TiSASRec end-to-end example (synthetic timestamped log -> TimeSequenceSampler -> epochs -> recommend_next -> hit rate) runs at
a reduced shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tisasrec_example_runs(hip_device):
    """Exit status 0, one JSON line, finite losses that fall over the epochs, a hit rate that is a rate."""
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "tisasrec_end_to_end.py"), "--users", "256", "--items", "200",
         "--maxlen", "20", "--time-span", "16", "--emb-dim", "32", "--heads", "2", "--batch-size", "64", "--epochs", "4", "--lr", "0.003"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    print(res)
    losses = res["mean_loss_per_epoch"]
    assert len(losses) == 4 and res["steps_per_epoch"] == 4
    assert all(np.isfinite(x) for x in losses)
    assert losses[-1] < losses[0]
    assert 0.0 <= res["hit_rate@10"] <= 1.0
