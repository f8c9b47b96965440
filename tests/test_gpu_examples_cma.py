"""examples/tune_rule_based_cma.py at its smallest arguments: it runs and prints finite returns for both searches."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def test_tune_rule_based_cma_example_runs(method="cma"):
    r = subprocess.run([sys.executable, "examples/tune_rule_based_cma.py", "--method", method, "--envs", "2", "--candidates", "8",
                        "--horizon", "4", "--iters", "2"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    default = re.search(r"default controller: return over the horizon ([-\d.e+]+)", r.stdout)
    assert default and np.isfinite(float(default.group(1))), r.stdout
    for name in ("cma", "cem"):
        m = re.search(rf"^{name}: best candidate ([-\d.e+]+) .*mean controller ([-\d.e+]+)", r.stdout, flags=re.M)
        assert m and np.isfinite(float(m.group(1))) and np.isfinite(float(m.group(2))), (name, r.stdout)
    assert "rows updated in the last generation: 2 of 2" in r.stdout and f"tuned by {method}:" in r.stdout
    assert len(re.findall(r"^  \w+\s+default\s+[\d.]+\s+tuned(\s+[\d.]+){2}$", r.stdout, flags=re.M)) == 5, r.stdout
    assert "nan" not in r.stdout.lower()
