"""GPU: the EASE example (clustered log -> prepare_model -> evaluate_full / recommend -> recommend_for for users outside
the frame) runs in a fresh process at a small size; the model finds the held-out item far more often than chance."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ease_example_beats_chance(hip_device):
    """Chance is 10 / (unseen items) ~ 0.026 at 400 items; 90 % of a user's interactions lie in the user's group (one of
    8).  Twice chance is a sanity floor, not a tuned number."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ease_end_to_end.py"), "--users", "600",
                          "--items", "400", "--interactions", "30000", "--reg", "20", "--fold-users", "60", "--top",
                          "10", "--show-users", "2"], capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    rows = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    summary = [r for r in rows if "chance" in r]
    lists = [r for r in rows if "recommended" in r]
    assert len(summary) == 1 and len(lists) == 2
    s = summary[0]
    assert s["users"] > 400 and s["held_out_users"] == 60 and 0.0 < s["chance"] < 0.05
    assert s["hit_rate@10"] > 2 * s["chance"], s
    assert s["held_out_hit_rate@10"] > 2 * s["chance"], s
    assert 0.0 < s["ndcg@10"] <= 1.0
    for r in lists:
        assert len(r["recommended"]) == 10 and len(set(r["recommended"])) == 10
        assert all(0 <= i < 400 for i in r["recommended"])
        assert r["scores"] == sorted(r["scores"], reverse=True)
