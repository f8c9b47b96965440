"""examples/policy_search_es.py at a tiny size: it runs, prints finite scores for both nets and the mean policy's return."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_policy_search_es_example_runs():
    r = subprocess.run([sys.executable, "examples/policy_search_es.py", "--envs", "2", "--candidates", "8", "--horizon", "4", "--iters", "2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    rule = re.search(r"rule-based controller, default constants: score ([-\d.e+]+)", r.stdout)
    assert rule and np.isfinite(float(rule.group(1))), r.stdout
    for name in ("linear", "23-32-6 tanh"):
        scores = [float(v) for v in re.findall(rf"{name}\s+iteration \d+: best score ([-\d.e+]+)", r.stdout)]
        assert len(scores) == 2 and np.isfinite(scores).all(), (name, r.stdout)
        mean = re.search(rf"{name}\s+\d+ parameters; the mean policy: score ([-\d.e+]+)", r.stdout)
        assert mean and np.isfinite(float(mean.group(1))), (name, r.stdout)
    assert "nan" not in r.stdout.lower()
