"""examples/train_recurrent_ppo.py at a small size: it runs, collects, updates, and prints finite figures for its three iterations."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_train_recurrent_ppo_example_runs():
    r = subprocess.run([sys.executable, "examples/train_recurrent_ppo.py", "--n-envs", "4096", "--n-steps", "8", "--seq-len", "4", "--epochs", "2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = re.findall(r"iteration (\d): 4096 envs x 8 steps collected in ([\d.]+) ms: ([\d.e+]+) env-steps/s; update \(2 epochs x 4 minibatches "
                       r"of sequences of 4\) in ([\d.]+) ms; normalised reward mean ([-+\d.]+); loss ([-+\d.]+) -> ([-+\d.]+), "
                       r"approx_kl ([-\d.e+]+), clip_fraction ([\d.]+), first minibatch max ratio ([\d.]+)", r.stdout)
    assert [int(v[0]) for v in lines] == [0, 1, 2], r.stdout
    vals = np.array([[float(x) for x in v[1:]] for v in lines])
    assert np.isfinite(vals).all() and (vals[:, 1] > 0).all() and (vals[:, 2] > 0).all(), r.stdout
    # before the first optimiser step of an iteration the ratio is 1 up to the float32 chains of the collection's and the update's products
    # (different shapes, so not bit for bit): 1e-3, the figure of tests/test_gpu_examples_ppo.py
    assert (np.abs(vals[:, 8] - 1) < 1e-3).all(), r.stdout
    tail = re.search(r"episodes finished so far (\d+), ODE failures (\d+)", r.stdout)
    assert tail and int(tail.group(2)) == 0, r.stdout
    assert "nan" not in r.stdout.lower()
