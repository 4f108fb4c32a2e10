"""GPU: the Mamba4Rec end-to-end example (synthetic log -> prefix batches -> epochs -> recommend_next) runs at a toy size
and its loss falls."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mamba4rec_example_runs_and_its_loss_falls(hip_device):
    epochs = 12
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "mamba4rec_end_to_end.py"), "--users", "192", "--items", "60",
         "--group", "10", "--emb-dim", "16", "--maxlen", "12", "--num-blocks", "1", "--batch-size", "64", "--epochs",
         str(epochs), "--lr", "0.005"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    print(res)
    losses = res["loss_per_epoch"]
    assert len(losses) == epochs and res["steps_per_epoch"] == 3
    assert all(np.isfinite(x) for x in losses) and losses[-1] < losses[0]
    assert 0.0 <= res["hit_rate@10"] <= 1.0 and res["random_hit_rate"] == 10 / 60
