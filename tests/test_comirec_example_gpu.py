"""GPU: the ComiRec end-to-end example (synthetic multi-interest users -> session_prefixes -> MultiInterestLoader -> epochs ->
recommend_next) runs at a toy size and its loss falls."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_comirec_example_runs_and_its_loss_falls(hip_device):
    epochs = 6
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "comirec_end_to_end.py"), "--users", "96", "--items", "60",
         "--group", "10", "--length", "10", "--emb-dim", "16", "--maxlen", "8", "--num-interest", "2", "--n-sample", "20",
         "--batch-size", "256", "--epochs", str(epochs), "--lr", "0.005"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    print(res)
    for key in ("loss_per_epoch", "loss_per_epoch_one_interest"):
        losses = res[key]
        assert len(losses) == epochs and all(np.isfinite(x) for x in losses) and losses[-1] < losses[0], key
    assert res["steps_per_epoch"] == 3      # 96 users x 8 prefixes in batches of 256
    assert 0.0 <= res["hit_rate@10"] <= 1.0 and 0.0 <= res["hit_rate@10_one_interest"] <= 1.0
    assert res["random_hit_rate"] == 10 / 60
