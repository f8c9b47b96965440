#!/usr/bin/env python3
"""What weather-forecast scenarios cost, measured on the GPU -> profiles/plan_wscen_cost.txt.

    python tools/plan_wscen_cost.py [--parent-pkg DIR] [--out profiles/plan_wscen_cost.txt]

fp32, ls5, (P, K, S, H) = (64, 128, 8, 48): 65 536 children; device events, warmed up, alternating samples.
(a) One Planner.rollout in scenario mode with weather_sigma = zeros -- the windows hold the parents' own rows, so both sides integrate
    identical weather values and differ only in the window stage and in where the rows are read from -- against the same scenario
    rollout (no weather_sigma) of the parent commit's build on the same children.  --parent-pkg DIR: the greenlight-gym2_amd directory
    of a checkout of the PARENT commit with its library built; its rollout runs in a child process on that build.  Without it, it runs
    on this build, the report says so and gives no verdict.  Requirement: ratio <= 1.05.
(b) Recorded, no requirement: glgym_plan_weather on its own; a rollout at typical sigmas (its env-step cost depends on the weather the
    children meet); the window stage written with torch ops in the same process (rand + cumulative recurrence + gather + where).
No fallback: without a GPU this fails."""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
P0, K0, S0, H0, TAIL, SCALE = 64, 128, 8, 48, 4, 0.2
SIGMA = [0.2, 1.5, 0.1, 0.0, 0.3, 2.0, 0.0]
PHI = 0.9
N_SAMPLES, N_INNER, N_WARM = 7, 5, 2
SEASON = 10


def setup(pkg):
    sys.path.insert(0, str(pkg))
    import torch
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    return torch, TomatoVecEnv, synthetic_weather


def parent_env(torch, TomatoVecEnv, w, P):
    """The P noisy parent environments both sides start from: seeded reset, four seeded steps."""
    env = TomatoVecEnv(P, weather=w, dtype="float32", season_length=SEASON, start_rows=list(range(0, 96 * P, 96)), seed=5, auto_reset=False,
                       uncertainty_scale=SCALE)
    env.reset_tensor()
    g = torch.Generator().manual_seed(1)
    for _ in range(4):
        env.step_tensor((torch.rand(P, 6, generator=g) * 2 - 1).to(env.device))
    assert (env.scheme, env.n_sub) == ("ls5", 128)
    return env


def candidates(torch, H, J, dev):
    return (torch.rand(H, J, 6, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(dev).contiguous()


def timed(torch, fn, n=N_INNER):
    """Device time of fn() in ms, mean of n windows between events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / n


def worker(pkg, P, K, S, H):
    """The scenario rollout (no weather_sigma) on the build under pkg; answers "time" on stdin with one sample."""
    torch, TomatoVecEnv, synthetic_weather = setup(pkg)
    env = parent_env(torch, TomatoVecEnv, synthetic_weather(n_rows=35040), P)
    plan = env.planner(K, H, n_scenarios=S, n_tail=TAIL, scenario_seed=7)
    cand = candidates(torch, H, P * K, env.device)
    for _ in range(N_WARM):
        timed(torch, lambda: plan.rollout(cand), 1)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "time":
            break
        print(f"ms {timed(torch, lambda: plan.rollout(cand)):.6f}", flush=True)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", default=None, help="built greenlight-gym2_amd directory of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plan_wscen_cost.txt"))
    ap.add_argument("--worker", nargs=5, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker[0]), *(int(v) for v in args.worker[1:]))
    torch, TomatoVecEnv, synthetic_weather = setup(ROOT / "greenlight-gym2_amd")
    if not torch.cuda.is_available():
        sys.exit("plan_wscen_cost.py needs a GPU (no fallback)")
    import ctypes as C
    from gl_gym_amd import _lib as L
    P, K, S, H = P0, K0, S0, H0
    J, n = P * K, P * K * S
    lines = [f"weather-forecast scenarios on the device: cost on {torch.cuda.get_device_name(0)} (tools/plan_wscen_cost.py)",
             f"fp32 ls5-128, (P, K, S, H) = ({P}, {K}, {S}, {H}): {J} candidates, {n} children, {P * S * H} window rows; noise=\"step\", scale {SCALE}, "
             f"n_tail {TAIL}; device events, {N_WARM} warm-up windows, {N_SAMPLES} alternating samples of {N_INNER} calls each; spread = (max - min) "
             "/ median of a side's samples", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731
    env = parent_env(torch, TomatoVecEnv, synthetic_weather(n_rows=35040), P)
    dev = env.device
    kw = dict(n_scenarios=S, n_tail=TAIL, scenario_seed=7)
    zeros = env.planner(K, H, weather_sigma=[0.0] * 7, weather_phi=PHI, **kw)
    typical = env.planner(K, H, weather_sigma=SIGMA, weather_phi=PHI, **kw)
    cand = candidates(torch, H, J, dev)

    # ---- (a) zero-sigma weather-scenario rollout against the parent commit's scenario rollout ---------------------------------------
    if args.parent_pkg:
        child = subprocess.Popen([sys.executable, __file__, "--worker", str(Path(args.parent_pkg).resolve()), str(P), str(K), str(S), str(H)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert child.stdout.readline().strip() == "ready", "the parent-commit worker did not start"

        def plain_sample():
            child.stdin.write("time\n")
            child.stdin.flush()
            return float(child.stdout.readline().split()[1])
        where = "a child process on the parent commit's build (--parent-pkg)"
    else:
        child, other = None, env.planner(K, H, **kw)
        plain_sample = lambda: timed(torch, lambda: other.rollout(cand))  # noqa: E731
        where = "THIS build (no --parent-pkg given; its step kernels are the parent commit's instruction for instruction)"
    for _ in range(N_WARM):
        timed(torch, lambda: zeros.rollout(cand), 1)
        if not child:
            plain_sample()
    ws, pl = [], []
    for _ in range(N_SAMPLES):
        ws.append(timed(torch, lambda: zeros.rollout(cand)))
        pl.append(plain_sample())
    if child:
        child.stdin.write("quit\n")
        child.stdin.flush()
        child.wait(timeout=60)
    assert int(zeros.n_steps_t.min()) == H and int(zeros.failed_t.max()) == 0
    m_ws, m_pl = statistics.median(ws), statistics.median(pl)
    ratio = m_ws / m_pl
    say(f"(a) the scenario rollout without weather_sigma on the same {n} children runs in {where}")
    say("      weather-scenario rollout, sigma = 0 (fork + window + 48 x (prologue, step, accumulate) + aggregate), ms: " + " ".join(f"{v:.3f}" for v in ws))
    say("      scenario rollout (fork + 48 x (prologue, step, accumulate) + aggregate), ms                            : " + " ".join(f"{v:.3f}" for v in pl))
    say(f"      medians {m_ws:.3f} / {m_pl:.3f} ms; spread of the weather-scenario samples {spread(ws) * 100:.1f} %, of the scenario samples "
        f"{spread(pl) * 100:.1f} %")
    say(f"      ratio = {ratio:.4f}" + (f"   (requirement <= 1.05: {'met' if ratio <= 1.05 else 'NOT MET'})" if child else ""))
    say()

    # ---- (b) recorded: the window stage on its own, a rollout at typical sigmas, the stage with torch ops ----------------------------
    lib, h, st = env._lib, env._h, env._stream
    wa = L.make_plan_args(L.PlanWeatherArgs, P, K, S, H, env.weather_rows, env.weather_t.data_ptr(), env.w_off_t.data_ptr(), env.timestep_t.data_ptr(),
                          (C.c_double * 7)(*SIGMA), PHI, 7, 0, typical.scenario_base_t.data_ptr(), typical.weather_window_t.data_ptr(),
                          typical.w_off_t.data_ptr())

    def hip_window():
        L.check(lib.glgym_plan_weather(h, C.byref(wa), st()), "glgym_plan_weather")

    nd = env.nd
    additive = torch.tensor([0, 1, 0, 0, 0, 1, 1], dtype=torch.bool, device=dev)
    g_t = torch.tensor(SIGMA, dtype=torch.float64, device=dev) * (1 - PHI * PHI) ** 0.5
    win_th = torch.zeros_like(typical.weather_window_t)
    off_th = torch.zeros_like(typical.w_off_t)
    hs = torch.arange(H, device=dev)

    def th_window():
        eps = (torch.rand(P * S, H, 7, 4, dtype=torch.float64, device=dev) - 0.5).sum(dim=3) * 3 ** 0.5
        e = torch.zeros(P * S, H, 7, dtype=torch.float64, device=dev)
        for k in range(1, H):                                    # the recurrence, one launch group per step
            e[:, k] = PHI * e[:, k - 1] + g_t * eps[:, k]
        rows = ((env.w_off_t + env.timestep_t).long()[:, None] + hs[None, :]).clamp_(0, env.weather_rows - 1)
        src = env.weather_t[rows].repeat_interleave(S, dim=0)     # [P*S, H, nd]
        w = src[..., :7].double()
        v = torch.where(additive, w + e, (w + e * w).clamp_min(0.0))
        out = win_th.view(P * S, H, nd)
        out.copy_(src)
        out[..., :7] = v.float()
        ps = torch.arange(P * S, device=dev).view(P, 1, S)
        off_th.view(P, K, S).copy_((ps * H - env.timestep_t.view(P, 1, 1)).expand(P, K, S))

    for fn in (hip_window, th_window):
        timed(torch, fn, 3)
    hipw, thw = [], []
    for _ in range(N_SAMPLES):
        hipw.append(timed(torch, hip_window))
        thw.append(timed(torch, th_window))
    for _ in range(N_WARM):
        timed(torch, lambda: typical.rollout(cand), 1)
    ty = [timed(torch, lambda: typical.rollout(cand)) for _ in range(N_SAMPLES)]
    n_failed = int(typical.failed_t.sum())
    say("(b) recorded, no requirement")
    say(f"      glgym_plan_weather ({P * S * H} rows x {nd} columns + {n} offsets), us : " + " ".join(f"{v * 1e3:.1f}" for v in hipw)
        + f"   median {statistics.median(hipw) * 1e3:.1f} us = {statistics.median(hipw) / m_ws * 100:.3f} % of the rollout in (a)")
    say("      the same stage with torch ops, us                                      : " + " ".join(f"{v * 1e3:.1f}" for v in thw)
        + f"   median {statistics.median(thw) * 1e3:.1f} us")
    say(f"      weather-scenario rollout at sigma = {SIGMA}, phi = {PHI}, ms: " + " ".join(f"{v:.3f}" for v in ty)
        + f"   median {statistics.median(ty):.3f} ms = {statistics.median(ty) / m_ws:.4f} x the zero-sigma rollout; {n_failed} of {n} children failed")
    say(f"      weather-scenario rollout rate at those sigmas {n * H / statistics.median(ty) * 1e3:.3e} scenario env-steps/s")
    say()
    env.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if (ratio <= 1.05 or not args.parent_pkg) else 1


if __name__ == "__main__":
    sys.exit(main())
