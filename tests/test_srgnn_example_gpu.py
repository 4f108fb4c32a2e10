"""GPU: the SR-GNN end-to-end example (synthetic sessions with revisits -> session_prefixes -> a shuffled SessionLoader ->
epochs -> recommend_next -> hit rate) at a reduced shape learns: its hit-rate@10 is above chance by the margin the example
itself prints."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_srgnn_example_learns(hip_device):
    """384 sessions, 60 items in groups of 10: chance is 10 / 60, and four binomial standard deviations of it at 384
    queries are 4 * sqrt(1/6 * 5/6 / 384) = 0.076 -- the margin is derived from the spread of chance, not from a run."""
    sessions, items, top, epochs = 384, 60, 10, 6
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "srgnn_end_to_end.py"), "--sessions", str(sessions), "--items",
         str(items), "--group", "10", "--hidden", "32", "--batch-size", "64", "--epochs", str(epochs), "--lr", "0.01",
         "--lr-dc-step", "4"],
        capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    print(res)
    losses = res["mean_loss_per_epoch"]
    assert len(losses) == epochs and res["steps_per_epoch"] >= 2
    assert all(np.isfinite(x) for x in losses) and losses[-1] < losses[0]
    chance = top / items
    margin = 4.0 * np.sqrt(chance * (1.0 - chance) / sessions)
    assert res["random_hit_rate"] == chance and abs(res["margin"] - margin) < 1e-12
    assert res[f"hit_rate@{top}"] > chance + margin, res
