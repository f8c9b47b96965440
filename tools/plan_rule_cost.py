#!/usr/bin/env python3
"""What closed-loop rule-based rollouts cost, measured on the GPU -> profiles/plan_rule_cost.txt.

    python tools/plan_rule_cost.py [--parent-pkg DIR] [--out profiles/plan_rule_cost.txt]

fp32, ls5, (P, K, H) = (64, 1 024, 48): 65 536 children; device events, warmed up, alternating samples.
(a) One RuleSearch.rollout (fork + 48 x (controller, step, accumulate)) against Planner.rollout(controls_t = the controls that rollout
    recorded) of the parent commit's build on the same children with the same verify mode: both sides integrate the same controls; the
    closed-loop side computes them, the open-loop side pays its staging copy.  --parent-pkg DIR: the greenlight-gym2_amd directory of a
    checkout of the PARENT commit with its library built; its rollout runs in a child process on that build.  Without it, it runs on
    this build, the report says so and gives no verdict.  Requirement: ratio <= 1.05.
(b) Recorded, no requirement: glgym_rule_rows on its own at that shape; RuleBasedController.predict with one config on device tensors
    of that shape (the torch-ops version of one candidate's work); one cem(n_iter=4) over the search space of
    examples/tune_rule_based.py, end to end.
No fallback: without a GPU this fails."""
import argparse
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
P0, K0, H0 = 64, 1024, 48
N_SAMPLES, N_INNER, N_WARM = 7, 3, 2
SEASON = 10
TUNE = {"temp_setpoint_day": (17.0, 23.0), "temp_setpoint_night": (14.0, 19.0), "co2_day": (400.0, 1200.0), "rh_max": (75.0, 95.0),
        "lamps_off": (12.0, 22.0)}                           # examples/tune_rule_based.py


def setup(pkg):
    sys.path.insert(0, str(pkg))
    import torch
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    return torch, TomatoVecEnv, synthetic_weather


def parent_env(torch, TomatoVecEnv, w, P):
    """The P parent environments both sides start from: seeded reset, four steps under the default controller."""
    from gl_gym_amd.baseline import RuleBasedController
    env = TomatoVecEnv(P, weather=w, dtype="float32", season_length=SEASON, start_rows=list(range(0, 96 * P, 96)), seed=5, auto_reset=False)
    env.reset_tensor()
    for _ in range(4):
        env.step_tensor(controller=RuleBasedController(), want_obs=False)
    assert (env.scheme, env.n_sub) == ("ls5", 128)
    return env


def timed(torch, fn, n=N_INNER):
    """Device time of fn() in ms, mean of n windows between events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / n


def worker(pkg, P, K, H, controls_file):
    """Planner.rollout(controls_t) on the build under pkg; answers "time" on stdin with one sample."""
    torch, TomatoVecEnv, synthetic_weather = setup(pkg)
    env = parent_env(torch, TomatoVecEnv, synthetic_weather(n_rows=35040), P)
    plan = env.planner(K, H)
    controls = torch.load(controls_file).to(env.device)
    for _ in range(N_WARM):
        timed(torch, lambda: plan.rollout(controls_t=controls), 1)
    print(f"ready {float(plan.ret_t.sum()):.17g}", flush=True)
    for line in sys.stdin:
        if line.strip() != "time":
            break
        print(f"ms {timed(torch, lambda: plan.rollout(controls_t=controls)):.6f}", flush=True)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", default=None, help="built greenlight-gym2_amd directory of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plan_rule_cost.txt"))
    ap.add_argument("--worker", nargs=5, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker[0]), *(int(v) for v in args.worker[1:4]), args.worker[4])
    torch, TomatoVecEnv, synthetic_weather = setup(ROOT / "greenlight-gym2_amd")
    if not torch.cuda.is_available():
        sys.exit("plan_rule_cost.py needs a GPU (no fallback)")
    import ctypes as C
    from gl_gym_amd import _lib as L
    from gl_gym_amd.baseline import RuleBasedController
    P, K, H = P0, K0, H0
    n = P * K
    lines = [f"closed-loop rule-based rollouts on the device: cost on {torch.cuda.get_device_name(0)} (tools/plan_rule_cost.py)",
             f"fp32 ls5-128, verify mode auto (raw-control steps run verified), (P, K, H) = ({P}, {K}, {H}): {n} candidate controllers = children, "
             f"{len(TUNE)} tuned constants; device events, {N_WARM} warm-up windows, {N_SAMPLES} alternating samples of {N_INNER} calls each; "
             "spread = (max - min) / median of a side's samples", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731
    env = parent_env(torch, TomatoVecEnv, synthetic_weather(n_rows=35040), P)
    dev = env.device
    base = RuleBasedController()
    search = env.rule_search(K, H, tune=TUNE, base=base)
    g = torch.Generator().manual_seed(2)
    theta = (search.theta_of(base).cpu() + 0.3 * torch.randn(search.Ht, n, 6, generator=g)).clamp_(-1, 1).to(dev).contiguous()
    search.rollout(theta, record=True)
    closed_sum = float(search.plan.ret_t.sum())
    assert int(search.plan.n_steps_t.min()) == H
    n_failed = int(search.plan.failed_t.sum())
    controls = search.controls.contiguous()                     # [H, C, 6]

    # ---- (a) the closed-loop rollout against the parent commit's open-loop rollout of the recorded controls ----------------------------
    tmp = None
    if args.parent_pkg:
        tmp = tempfile.NamedTemporaryFile(suffix=".pt")
        torch.save(controls.cpu(), tmp.name)
        child = subprocess.Popen([sys.executable, __file__, "--worker", str(Path(args.parent_pkg).resolve()), str(P), str(K), str(H), tmp.name],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        ready = child.stdout.readline().split()
        assert ready and ready[0] == "ready", "the parent-commit worker did not start"
        open_sum = float(ready[1])

        def open_sample():
            child.stdin.write("time\n")
            child.stdin.flush()
            return float(child.stdout.readline().split()[1])
        where = "a child process on the parent commit's build (--parent-pkg)"
    else:
        child, other = None, env.planner(K, H)
        open_sample = lambda: timed(torch, lambda: other.rollout(controls_t=controls))  # noqa: E731
        other.rollout(controls_t=controls)
        open_sum = float(other.ret_t.sum())
        where = "THIS build (no --parent-pkg given; its step kernels are the parent commit's instruction for instruction)"
    for _ in range(N_WARM):
        timed(torch, lambda: search.rollout(theta), 1)
        if not child:
            open_sample()
    cl, op = [], []
    for _ in range(N_SAMPLES):
        cl.append(timed(torch, lambda: search.rollout(theta)))
        op.append(open_sample())
    if child:
        child.stdin.write("quit\n")
        child.stdin.flush()
        child.wait(timeout=60)
    m_cl, m_op = statistics.median(cl), statistics.median(op)
    ratio = m_cl / m_op
    say(f"(a) the open-loop rollout of the recorded controls on the same {n} children runs in {where}")
    say(f"      sum of the {n} returns: closed loop {closed_sum:.17g}, open-loop replay {open_sum:.17g} ({'equal' if closed_sum == open_sum else 'DIFFERENT'}); "
        f"{n_failed} children failed")
    say("      closed-loop rollout (fork + 48 x (controller, step, accumulate)), ms              : " + " ".join(f"{v:.3f}" for v in cl))
    say("      open-loop rollout of the recorded controls (staging copy + fork + 48 x (step, accumulate)), ms: " + " ".join(f"{v:.3f}" for v in op))
    say(f"      medians {m_cl:.3f} / {m_op:.3f} ms; spread of the closed-loop samples {spread(cl) * 100:.1f} %, of the open-loop samples "
        f"{spread(op) * 100:.1f} %")
    say(f"      ratio = {ratio:.4f}" + (f"   (requirement <= 1.05: {'met' if ratio <= 1.05 else 'NOT MET'})" if child else ""))
    say()

    # ---- (b) recorded: the rows kernel, predict with torch ops, one cem() -------------------------------------------------------------
    p = search.plan
    p.fork()
    plane = torch.zeros(6, p.ld, dtype=env.tdtype, device=dev)
    rule = L.RuleArgs(p.C, p.ld, p.x_T.data_ptr(), env.weather_t.data_ptr(), env.weather_rows, p.w_off_t.data_ptr(), p.timestep_t.data_ptr(),
                      p.start_day_t.data_ptr(), None, None, plane.data_ptr())
    ra = L.make_plan_args(L.RuleRowsArgs, p.J, 0, rule, search._space, theta.data_ptr())

    def hip_rows():
        L.check(env._lib.glgym_rule_rows(env._h, C.byref(ra), env._stream()), "glgym_rule_rows")

    x = p.x.contiguous()                                        # [C, 28]
    d = env.weather_t[(p.w_off_t + p.timestep_t).long().clamp_(0, env.weather_rows - 1)]
    hod = (p.timestep_t.double() * (env.dt / 3600)) % 24
    doy = p.start_day_t.double() + p.timestep_t.double() * ((env.dt / 86400) % 365)

    def th_predict():
        return base.predict(x, d, hod.to(x.dtype), doy.to(x.dtype))

    for fn in (hip_rows, th_predict):
        timed(torch, fn, 3)
    rows_t, pred_t = [], []
    for _ in range(N_SAMPLES):
        rows_t.append(timed(torch, hip_rows, 20))
        pred_t.append(timed(torch, th_predict, 20))
    E = 64
    for _ in range(N_WARM):
        timed(torch, lambda: search.cem(4, E, carry=2, seed=1), 1)
    cem_t = [timed(torch, lambda: search.cem(4, E, carry=2, seed=1), 1) for _ in range(N_SAMPLES)]
    say("(b) recorded, no requirement")
    say(f"      glgym_rule_rows ({n} rows, one set of constants each), us per step : " + " ".join(f"{v * 1e3:.1f}" for v in rows_t)
        + f"   median {statistics.median(rows_t) * 1e3:.1f} us = {statistics.median(rows_t) * H / m_cl * 100:.2f} % of the rollout in (a) over its {H} steps")
    say(f"      RuleBasedController.predict, ONE config, torch ops on {n} rows, us    : " + " ".join(f"{v * 1e3:.1f}" for v in pred_t)
        + f"   median {statistics.median(pred_t) * 1e3:.1f} us")
    say(f"      cem(n_iter=4, n_elite={E}, carry=2), end to end, ms                     : " + " ".join(f"{v:.2f}" for v in cem_t)
        + f"   median {statistics.median(cem_t):.2f} ms = {statistics.median(cem_t) / (4 * m_cl):.4f} x four rollouts of (a); "
        f"{4 * n * H / statistics.median(cem_t) * 1e3:.3e} closed-loop env-steps/s")
    say()
    env.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if (ratio <= 1.05 or not args.parent_pkg) else 1


if __name__ == "__main__":
    sys.exit(main())
