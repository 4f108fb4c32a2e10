"""GPU: the neighbourhood example (ItemKNN and UserKNN on a clustered log -> recommend -> hit-rate@10) runs in a fresh
process and both models beat chance by a wide margin."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_knn_example_beats_chance(hip_device):
    """Chance is 10 / (unseen items) ~ 0.026 at 400 items; 90 % of a user's interactions lie in the user's group (one of
    8), so a neighbourhood model puts the held-out item among its 10 best many times as often."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "knn_end_to_end.py"), "--users", "600",
                          "--items", "400", "--interactions", "30000", "--neighbourhood-size", "50", "--top", "10",
                          "--show-users", "2"], capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    rows = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    summary, lists = [r for r in rows if "chance" in r], [r for r in rows if "user" in r]
    assert [r["model"] for r in summary] == ["ItemKNN", "UserKNN"] and len(lists) == 4
    for r in summary:
        assert r["users"] > 500 and 0.0 < r["chance"] < 0.05
        assert r["hit_rate@10"] > 3 * r["chance"], r
    for r in lists:
        assert len(r["recommended"]) == 10 and len(set(r["recommended"])) == 10
        assert all(0 <= i < 400 for i in r["recommended"])
        assert r["scores"] == sorted(r["scores"], reverse=True)
