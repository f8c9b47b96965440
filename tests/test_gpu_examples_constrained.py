"""examples/mpc_constrained.py at its smallest arguments: it runs and prints finite returns and achieved violations for both runs."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_mpc_constrained_example_runs():
    r = subprocess.run([sys.executable, "examples/mpc_constrained.py", "--season", "0.125", "--candidates", "16", "--horizon", "4", "--iters", "2",
                        "--elites", "4"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    for head in ("unconstrained", "rh budget 0"):
        m = re.search(rf"^{head}: episode return ([-\d.e+]+), achieved RH violation per step ([-\d.e+]+) ", r.stdout, flags=re.M)
        assert m and np.isfinite(float(m.group(1))) and float(m.group(2)) >= 0.0, (head, r.stdout)
    m = re.search(r"decisions whose best candidate was feasible: (\d+) of (\d+)", r.stdout)
    assert m and 0 <= int(m.group(1)) <= int(m.group(2)) and int(m.group(2)) > 0, r.stdout
    assert "nan" not in r.stdout.lower()
