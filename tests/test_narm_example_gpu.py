"""GPU: the NARM end-to-end example (synthetic session log -> session_prefixes -> SessionLoader -> epochs ->
recommend_next -> hit rate) runs at a reduced shape."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_narm_example_runs(hip_device):
    """Exit status 0, one JSON line, finite losses that fall over the epochs, a hit rate above the untrained model's."""
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "narm_end_to_end.py"), "--sessions", "300", "--items", "100",
         "--max-len", "9", "--emb-dim", "24", "--hidden", "36", "--batch-size", "128", "--epochs", "8", "--lr", "0.01"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    print(res)
    losses = res["mean_loss_per_epoch"]
    assert len(losses) == 8 and res["steps_per_epoch"] == -(-res["pairs"] // 128)
    assert all(np.isfinite(x) for x in losses)
    assert losses[-1] < losses[0]
    assert 0.0 <= res["untrained_hit_rate@10"] < res["hit_rate@10"] <= 1.0
