"""examples/collect_rollouts.py at a small size: it runs, collects, and prints finite figures for its three PPO iterations."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_collect_rollouts_example_runs():
    r = subprocess.run([sys.executable, "examples/collect_rollouts.py", "--n-envs", "4096", "--n-steps", "8"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = re.findall(r"iteration (\d): 4096 envs x 8 steps collected in ([\d.]+) ms: ([\d.e+]+) env-steps/s; "
                       r"first minibatch max \|ratio - 1\| = ([\d.e+-]+); loss ([-+\d.]+) -> ([-+\d.]+)", r.stdout)
    assert [int(v[0]) for v in lines] == [0, 1, 2], r.stdout
    vals = np.array([[float(x) for x in v[1:]] for v in lines])
    assert np.isfinite(vals).all() and (vals[:, 1] > 0).all(), r.stdout
    print("max |ratio - 1| of the first minibatch, per iteration:", vals[:, 2])      # recorded only: no bar
    tail = re.search(r"advantage mean ([-+\d.]+), normalised reward mean ([-+\d.]+), episodes finished so far (\d+), ODE failures (\d+)", r.stdout)
    assert tail and np.isfinite([float(tail.group(1)), float(tail.group(2))]).all() and int(tail.group(4)) == 0, r.stdout
    assert "nan" not in r.stdout.lower()
