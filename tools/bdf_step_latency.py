#!/usr/bin/env python3
"""Latency of the BDF env-step (glgym_set_step_integrator) against glgym_evalF's BDF and the explicit env-step, fp64, on the rows of
holdout_gl2010_random: in repetition r environment b of a batch of B takes row k = (b + 31 r) mod 961 (glgym_step with X[k], U[k] as
raw control, w_off = k, timestep = 0; glgym_evalF on the same rows), so that small batches are timed over many rows, not one.  Also a
free-running step_tensor rollout of B identical environments from the reset state, with the fixture's actions and with its raw controls.
ms per launch, median [p10, p90] -> profiles/bdf_env_step_latency.txt (one MI355X run).

    python tools/bdf_step_latency.py [--reps 31] [--out profiles/bdf_env_step_latency.txt]
"""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT / "greenlight-gym2_amd")]

import torch                                                   # noqa: E402

from gl_gym_amd import GreenLight                              # noqa: E402
from gl_gym_amd import _lib as L                               # noqa: E402
from gl_gym_amd.tomato_env import TomatoVecEnv                 # noqa: E402

# bdf_env_kernel, both dtypes: -Rpass-analysis=kernel-resource-usage of csrc/glgym_bdf.hip at the Makefile's flags (hipcc, gfx950)
RESOURCES = "VGPRs 256, AGPRs 223, LDS 20 280 B per workgroup, scratch 0 B per lane, occupancy 1 wave per SIMD"


def q(v):
    v = np.asarray(v)
    return f"{np.median(v):8.3f} [{np.percentile(v, 10):7.3f}, {np.percentile(v, 90):7.3f}]"


class Step:
    """glgym_step on device tensors of B environments of an fp64 handle; once(idx) loads rows idx of the fixture (untimed), then times
    one launch."""

    def __init__(self, m, B, X, U, W, raw):
        dev, t = torch.device("cuda:0"), dict(dtype=torch.float64, device="cuda:0")
        self.m, self.B, self.Xh, self.Uh, self.raw = m, B, X, U, raw
        self.X, self.U = torch.zeros(28, B, **t), torch.zeros(6, B, **t)
        self.ctl = torch.zeros(6, B, **t) if raw else None
        self.act = None if raw else torch.zeros(B, 6, dtype=torch.float32, device=dev)
        self.W = torch.as_tensor(W, **t)
        self.w_off = torch.zeros(B, dtype=torch.int32, device=dev)
        self.ts = torch.zeros(B, dtype=torch.int32, device=dev)
        self.rew, self.info = torch.zeros(B, **t), torch.zeros(11, B, **t)
        self.done = torch.zeros(B, dtype=torch.uint8, device=dev)
        self.met = torch.zeros(L.METRIC_REPLICAS, L.METRIC_STRIDE, dtype=torch.float32, device=dev)
        self.flags = torch.zeros(B, dtype=torch.int32, device=dev)
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def once(self, idx):
        self.X.copy_(torch.as_tensor(self.Xh[idx].T.copy()))
        self.U.copy_(torch.as_tensor(self.Uh[idx].T.copy()))
        if self.raw:
            self.ctl.copy_(self.U)
        self.w_off.copy_(torch.as_tensor(idx, dtype=torch.int32))
        self.ts.zero_()
        a = L.make_step_args(self.B, self.B, self.X.data_ptr(), self.U.data_ptr(), self.act.data_ptr() if self.act is not None else None,
                             self.ctl.data_ptr() if self.ctl is not None else None, self.W.data_ptr(), self.W.shape[0],
                             self.w_off.data_ptr(), self.ts.data_ptr(), None, 10 ** 6, self.rew.data_ptr(), self.info.data_ptr(),
                             self.done.data_ptr(), self.met.data_ptr(), self.flags.data_ptr())
        torch.cuda.synchronize()
        self.ev[0].record()
        L.check(self.m._lib.glgym_step(self.m.handle, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "glgym_step")
        self.ev[1].record()
        torch.cuda.synchronize()
        return self.ev[0].elapsed_time(self.ev[1])


def handle(step_bdf, tol=1e-6):
    m = GreenLight(28, 6, 10, 208, 900.0, integrator="bdf", rtol=tol, atol=tol)     # evalF BDF; fp64, parity preset for explicit steps
    L.check(m._lib.glgym_set_step_integrator(m.handle, 1 if step_bdf else 0))
    if not step_bdf:
        m.set_integrator("explicit")
    return m


def rollout_ms(B, W, seq, raw, reps):
    """Free-running step_tensor of B identical environments from the reset state: seq[k] = the fixture's action (raw False) or raw
    control (raw True) of step k; the first two steps are not timed."""
    env = TomatoVecEnv(B, weather=W, dtype="float64", season_length=1, auto_reset=False, integrator="bdf")
    env.reset_tensor()
    src = torch.as_tensor(seq[:reps + 2], dtype=torch.float64 if raw else torch.float32, device=env.device)
    out = []
    for k in range(reps + 2):
        row = src[k][None].expand(B, 6).contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        env.step_tensor(controls_t=row, want_obs=False) if raw else env.step_tensor(row, want_obs=False)
        torch.cuda.synchronize()
        if k >= 2:
            out.append(1e3 * (time.perf_counter() - t0))
    assert env.metrics()["n_ode_fail"] == 0
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=31)
    ap.add_argument("--batches", default="1,8,64,1024,4096")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bdf_env_step_latency.txt"))
    args = ap.parse_args()
    g = np.load(ROOT / "tests" / "golden" / "holdout_gl2010_random.npz")
    X, U, Wall, acts = g["X"], g["U"], g["weather"], g["actions"]
    n = len(U)
    lines = [f"# BDF env-step latency, MI355X, fp64, holdout_gl2010_random one-step maps: repetition r, env b takes row (b + 31 r) mod {n} "
             f"(state, raw control, w_off = that row, timestep 0); ms per launch, median [p10, p90] of {args.reps} repetitions; "
             f"bdf_env_kernel: {RESOURCES}",
             "# free-running columns: B identical envs from the reset state, the fixture's actions / its raw controls, steps 2..11",
             "# B | step BDF 1e-6 | step BDF 1e-8 | evalF BDF 1e-6 (host copies incl.) | explicit parity raw (verify auto) | explicit "
             "parity action (zero actions) | free-running BDF actions | free-running BDF raw | mean BDF steps, rhs per env-step (1e-6)"]
    for B in [int(b) for b in args.batches.split(",")]:
        rows = [(np.arange(B) + 31 * r) % n for r in range(args.reps)]
        res = {}
        for key, bdf, tol, raw in (("b6", True, 1e-6, True), ("b8", True, 1e-8, True), ("er", False, 1e-6, True), ("ea", False, 1e-6, False)):
            m = handle(bdf, tol)
            s = Step(m, B, X, U, Wall, raw)
            s.once(rows[0])
            s.met.zero_()
            res[key] = [s.once(idx) for idx in rows]
            if key == "b6":
                mv = s.met.double().sum(dim=0).cpu().numpy()
                res["stats"] = (mv[L.METRIC_BDF] / (B * args.reps), mv[L.METRIC_BDF + 1] / (B * args.reps))
                flags = s.flags.cpu().numpy()
                assert np.all(flags & L.SF_BDF) and not np.any(flags & L.SF_FAILED)
            m.close()
        m = handle(True)
        m.evalF_batch(X[rows[0]], U[rows[0]], Wall[rows[0]])
        ev = []
        for idx in rows:
            Xi, Ui, Wi = X[idx], U[idx], Wall[idx]
            t0 = time.perf_counter()
            m.evalF_batch(Xi, Ui, Wi)
            ev.append(1e3 * (time.perf_counter() - t0))
        m.close()
        ra = rollout_ms(B, Wall, acts, False, min(args.reps, 10))
        rr = rollout_ms(B, Wall, U, True, min(args.reps, 10))
        line = (f"B {B:5d} | {q(res['b6'])} | {q(res['b8'])} | {q(ev)} | {q(res['er'])} | {q(res['ea'])} | {q(ra)} | {q(rr)} | "
                f"{res['stats'][0]:.1f}, {res['stats'][1]:.0f}")
        print(line, flush=True)
        lines.append(line)
    Path(args.out).parent.mkdir(exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
