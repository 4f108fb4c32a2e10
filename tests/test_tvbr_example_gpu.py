"""GPU: the TVBR end-to-end example (synthetic timestamped baskets -> triples with T -> N(0, 1) features -> alias
samplers -> epochs over the time steps -> recommend -> hit rate) runs at a reduced shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tvbr_example_runs(hip_device):
    """Exit status 0, one JSON line, a step for every full batch of every time step, finite losses that fall over the
    epochs, a hit rate above the untrained model's and above the chance of a random ranking."""
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "tvbr_end_to_end.py"), "--users", "300", "--items", "200",
         "--groups", "8", "--emb-dim", "24", "--fea-dim", "48", "--time-step", "4", "--batch-size", "128", "--epochs", "6"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    print(res)
    losses = res["total_loss_per_epoch"]
    assert len(losses) == 6 and res["time_step"] == 4
    assert res["triples"] // 128 - 4 < res["steps_per_epoch"] <= res["triples"] // 128
    assert all(np.isfinite(x) for x in losses)
    assert losses[-1] < losses[0]
    assert res["random_ranking"] == 10 / 200
    assert res["random_ranking"] < res["hit_rate@10"] <= 1.0
    assert 0.0 <= res["untrained_hit_rate@10"] < res["hit_rate@10"]
