"""GPU: the SLIM example (clustered log -> prepare_model -> evaluate_full / recommend -> recommend_for for users outside
the frame) runs in a fresh process at a small size; the model finds the held-out item far more often than chance and
reports its sparsity and sweep counts."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slim_example_beats_chance(hip_device):
    """Chance is 10 / (unseen items) ~ 0.026 at 400 items; 90 % of a user's interactions lie in the user's group (one of
    8).  Twice chance is a sanity floor, not a tuned number.  (The restatement needs at most 192 sweeps on the whole log
    at this l2; the frame of the example, without the held-out pairs, took 155 on an MI355X.)"""
    launcher = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")
    env = {k: v for k, v in os.environ.items() if k not in launcher}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "slim_end_to_end.py"), "--users", "600",
                          "--items", "400", "--interactions", "30000", "--l1", "1", "--l2", "50", "--max-sweeps", "300", "--fold-users", "60",
                          "--top", "10", "--show-users", "2"], capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    rows = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    summary = [r for r in rows if "chance" in r]
    lists = [r for r in rows if "recommended" in r]
    assert len(summary) == 1 and len(lists) == 2
    s = summary[0]
    assert s["model"] == "SLIM" and s["users"] > 400 and s["held_out_users"] == 60 and 0.0 < s["chance"] < 0.05
    assert s["hit_rate@10"] > 2 * s["chance"], s
    assert s["held_out_hit_rate@10"] > 2 * s["chance"], s
    assert 0.0 < s["ndcg@10"] <= 1.0
    assert 0 < s["nnz"] < 400 * 399 and 0.0 < s["density"] < 1.0, "the weights are sparse and not empty"
    assert 1 <= s["sweeps"]["min"] <= s["sweeps"]["median"] <= s["sweeps"]["max"] <= 300 and s["n_unconverged"] == 0
    for r in lists:
        assert len(r["recommended"]) == 10 and len(set(r["recommended"])) == 10
        assert all(0 <= i < 400 for i in r["recommended"])
        assert r["scores"] == sorted(r["scores"], reverse=True)
