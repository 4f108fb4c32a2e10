"""GPU: the recommendation example (train BPR-MF -> evaluate_full over the whole catalogue -> recommend for a few users)
runs in a fresh process, learns on data with planted structure, and prints its metrics and lists."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_recommend_example_learns_and_recommends(hip_device):
    """Full-catalogue ndcg@10 of a random order is about 2 * 10 / 400 / idcg ~ 0.03 here; a model that found the planted
    groups ranks the held-out items (two per user, in the user's group 9 times of 10) far above that."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "recommend_end_to_end.py"), "--users", "600",
                          "--items", "400", "--interactions", "30000", "--emb-dim", "32", "--batch-size", "512",
                          "--epochs", "6", "--top", "10", "--show-users", "3"],
                         capture_output=True, text=True, env=env, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    rows = [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]
    hist, recs = [r for r in rows if "epoch" in r], [r for r in rows if "user" in r]
    assert len(hist) == 6 and len(recs) == 3
    assert hist[-1]["loss"] < hist[0]["loss"]
    assert max(h["ndcg@10"] for h in hist) > 0.1, [h["ndcg@10"] for h in hist]
    assert all(0.0 <= h[f"{m}@{k}"] <= 1.0 for h in hist for m in ("ndcg", "recall", "precision") for k in (5, 10, 20))
    for r in recs:
        assert len(r["recommended"]) == 10 and len(set(r["recommended"])) == 10
        assert all(0 <= i < 400 for i in r["recommended"])
        assert r["scores"] == sorted(r["scores"], reverse=True)
