"""GPU: the ETA end-to-end example (a telling burst more than 256 positions back -> CandidateLoader -> epochs -> rerank of 1
positive among 99 negatives) runs at a toy size, its loss falls and its hit rate clears chance by the 4-sigma margin."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eta_example_ranks_the_held_out_item_above_chance(hip_device):
    epochs = 30
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "eta_end_to_end.py"), "--users", "192", "--items", "400", "--clusters",
         "16", "--group", "8", "--maxlen", "288", "--emb-dim", "16", "--batch-size", "128", "--epochs", str(epochs)],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    print(res)
    losses = res["loss_per_epoch"]
    assert len(losses) == epochs and all(np.isfinite(x) for x in losses) and losses[-1] < losses[0]
    assert res["steps_per_epoch"] == 11      # 192 users x 7 targets in batches of 128
    assert res["random_hit_rate"] == 0.1 and 0.0 <= res["burst_share_before"] <= 1.0 >= res["burst_share_after"] >= 0.0
    assert res["hit_rate@10"] > res["random_hit_rate"] + res["margin"]
