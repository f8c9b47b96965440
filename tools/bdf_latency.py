#!/usr/bin/env python3
"""Latency of one glgym_evalF call with the BDF integrator (GLGYM_INTEGRATOR_BDF) beside the explicit ls5 parity preset, on the SAME
inputs, in the same process, alternating call by call.  Host buffers in / out (what GreenLight.evalF pays).  fp64 handles.
Inputs: one-step maps drawn from tests/golden/holdout_gl2010_random.npz (realistic trajectory states of ten frost days: state k,
control k, weather row k); the init_state tuples of tools/evalf_latency.py are reported separately.  Median [p10, p90] of `reps`
calls after a warm-up; beside them the mean right-hand sides, steps and LU factorisations per row (GreenLight.solver_stats()).
        python tools/bdf_latency.py [reps] > profiles/bdf_evalf_latency.txt
        rocprofv3 --kernel-trace --stats -d DIR -o bdf -- python tools/bdf_latency.py trace     (B = 1 BDF calls only: kernel vs copies)"""
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "greenlight-gym2_amd"))
from gl_gym_amd import GreenLight  # noqa: E402
from gl_gym_amd.utils import init_state, synthetic_weather  # noqa: E402

trace = len(sys.argv) > 1 and sys.argv[1] == "trace"
reps = int(sys.argv[1]) if len(sys.argv) > 1 and not trace else 50
g = np.load(ROOT / "tests" / "golden" / "holdout_gl2010_random.npz")
rng = np.random.default_rng(11)
if trace:
    m = GreenLight(28, 6, 10, 208, 900.0, integrator="bdf")
    for k in range(0, 961, 32):                              # 31 calls of one row each
        m.evalF_batch(g["X"][k], g["U"][k], g["weather"][k])
    m.close()
    sys.exit(0)


def holdout_rows(B):
    k = rng.integers(0, 961, B)
    return g["X"][k], g["U"][k], g["weather"][k]


w = synthetic_weather(2000)


def init_rows(B):
    D = w[rng.integers(0, len(w), B)]
    return np.array([init_state(d) for d in D]), rng.uniform(0, 1, (B, 6)), D


def handles():
    hs = {}
    for tol in (1e-6, 1e-8):
        hs[f"bdf {tol:g}"] = GreenLight(28, 6, 10, 208, 900.0, integrator="bdf", rtol=tol, atol=tol)
    for verify in ("auto", "never"):
        m = GreenLight(28, 6, 10, 208, 900.0)                # ls5 parity preset (n_sub 192, window 1)
        m.set_verify(verify)
        hs[f"ls5 parity {verify}"] = m
    return hs


def measure(hs, X, U, D, n):
    t = {k: [] for k in hs}
    for _ in range(3):
        for m in hs.values():
            m.evalF_batch(X, U, D)
    for _ in range(n):
        for k, m in hs.items():                              # alternating: every setting sees the same machine state
            t0 = time.perf_counter()
            m.evalF_batch(X, U, D)
            t[k].append((time.perf_counter() - t0) * 1e3)
    return t


hs = handles()
print("# glgym_evalF latency, fp64, host pointers in / out, MI355X; milliseconds per CALL: median [p10, p90]; BDF rows: mean right-hand")
print("# sides / steps / LU factorisations per row (solver_stats).  ls5 parity = the explicit default of GreenLight (n_sub 192, window 1)")
for label, make in (("holdout_gl2010_random one-step maps", holdout_rows), ("init_state tuples (tools/evalf_latency.py)", init_rows)):
    print(f"# inputs: {label}")
    print("# setting            B      ms/call                     us/row      rhs/row  steps/row  LU/row")
    for B in (1, 8, 64, 1024, 4096):
        X, U, D = make(B)
        n = reps if B <= 64 else max(5, reps // 10)
        t = measure(hs, X, U, D, n)
        for k, m in hs.items():
            v = np.array(t[k])
            extra = ""
            if k.startswith("bdf"):
                st = m.solver_stats()
                extra = f"{st['rhs_evals'].mean():9.0f}  {st['steps'].mean():9.1f}  {st['factorisations'].mean():6.1f}"
            print(f"{k:18s} {B:5d}   {np.median(v):9.3f} [{np.quantile(v, .1):8.3f}, {np.quantile(v, .9):8.3f}]   "
                  f"{1e3 * np.median(v) / B:9.2f}  {extra}", flush=True)
for m in hs.values():
    m.close()
