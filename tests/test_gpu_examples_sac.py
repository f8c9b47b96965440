"""examples/train_sac.py at a small size: it runs in a child process of its own, collects, updates, and prints finite figures."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_train_sac_example_runs():
    r = subprocess.run([sys.executable, "examples/train_sac.py", "--n-envs", "4096", "--n-slots", "6", "--train-freq", "2", "--gradient-steps", "2"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = re.findall(r"iteration (\d): 4096 envs x 2 steps collected in ([\d.]+) ms: ([\d.e+]+) env-steps/s; 2 gradient steps of 4096 rows in ([\d.]+) ms; "
                       r"ring (\d) of 5 slots; normalised reward mean ([-+\d.]+); critic_loss ([\d.]+), actor_loss ([-+\d.]+), "
                       r"ent_coef_loss ([-+\d.]+), alpha ([\d.]+), logp_mean ([-+\d.]+)", r.stdout)
    assert [int(v[0]) for v in lines] == [0, 1, 2], r.stdout
    vals = np.array([[float(x) for x in v[1:]] for v in lines])
    assert np.isfinite(vals).all() and (vals[:, 1] > 0).all() and (vals[:, 2] > 0).all() and (vals[:, 8] > 0).all(), r.stdout
    assert vals[:, 3].tolist() == [4, 5, 5], r.stdout             # 2 warm-up steps, then 2 per iteration into a ring of 5 transition slots
    tail = re.search(r"episodes finished so far (\d+), ODE failures (\d+)", r.stdout)
    assert tail and int(tail.group(2)) == 0, r.stdout
    assert "nan" not in r.stdout.lower()
