#!/usr/bin/env python3
"""What device-side planning costs, measured on the GPU -> profiles/plan_rollout_cost.txt.

    python tools/plan_cost.py [--parent-pkg DIR] [--out profiles/plan_rollout_cost.txt]

1. Overhead per step.  fp32, ls5, B x K = 64 x 1 024 = 65 536 children, H = 20: the device time of Planner.rollout (fork + 20 x
   (glgym_step + glgym_plan_accumulate)) against 20 x step_tensor(want_obs=False) on a 65 536-environment auto_reset=False
   environment holding the same states and taking the same actions.  --parent-pkg DIR: the greenlight-gym2_amd directory of a
   checkout of the PARENT commit with its library built (make -C DIR/csrc); the loop then runs in a child process on that build.
   Without it the loop runs on this build (whose step kernels are the parent's instruction for instruction) and the report says so.  Both sides are timed with device events around the same work, warmed up, in alternation, N_SAMPLES samples of N_INNER
   horizons each; the report gives every sample, the medians and their ratio.  Requirement: ratio <= 1.05.
2. glgym_plan_fork and glgym_plan_select (with and without the MPPI mean) at (B, K, H) = (64, 1 024, 48) and (8, 8 192, 48), and the
   end-to-end planning rate (fork + rollout + select) in candidate env-steps/s.  Recorded, no bar.
3. The free-running 97-step rollout against the reference environment's fixture (tests/golden/refenv_1day.npz, leg ra), both dtypes.
No fallback: without a GPU this fails."""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
B0, K0, H0 = 64, 1024, 20
N_SAMPLES, N_INNER, N_WARM = 7, 10, 3
SEASON = 10


def setup(pkg):
    sys.path.insert(0, str(pkg))
    import torch
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    return torch, TomatoVecEnv, synthetic_weather


def parent_states(torch, TomatoVecEnv, w):
    """The 64 parent environments both sides start from: seeded reset, four seeded steps."""
    env = TomatoVecEnv(B0, weather=w, dtype="float32", season_length=SEASON, start_rows=list(range(0, 96 * 64, 96)), seed=5, auto_reset=False)
    env.reset_tensor()
    g = torch.Generator().manual_seed(1)
    for _ in range(4):
        env.step_tensor((torch.rand(B0, 6, generator=g) * 2 - 1).to(env.device))
    return env


def horizon_actions(torch, device):
    g = torch.Generator().manual_seed(2)
    return (torch.rand(H0, B0 * K0, 6, generator=g) * 2 - 1).to(device).contiguous()


def timed(torch, fn, prepare=None, n=N_INNER):
    """Device time of fn() in ms, mean of n windows between events; prepare() runs before each window, untimed."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        if prepare:
            prepare()
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / n


class StepLoop:
    """20 x step_tensor(want_obs=False) on 65 536 environments holding the forked states."""

    def __init__(self, pkg):
        torch, TomatoVecEnv, synthetic_weather = setup(pkg)
        self.torch = torch
        w = synthetic_weather(n_rows=35040)
        par = parent_states(torch, TomatoVecEnv, w)
        self.env = env = TomatoVecEnv(B0 * K0, weather=w, dtype="float32", season_length=SEASON, start_rows=[0], seed=5, auto_reset=False)
        env.reset_tensor()
        rep = lambda t: t.repeat_interleave(K0, dim=-1)  # noqa: E731
        C = B0 * K0
        self.keep = [(env.x_T[:, :C], rep(par.x_T[:, :B0]).clone()), (env.u_T[:, :C], rep(par.u_T[:, :B0]).clone()),
                     (env.timestep_t, rep(par.timestep_t).clone()), (env.w_off_t, rep(par.w_off_t).clone()),
                     (env.start_day_t, rep(par.start_day_t).clone())]
        self.acts = horizon_actions(torch, env.device)
        assert (env.scheme, env.n_sub) == ("ls5", 128)
        for _ in range(N_WARM):
            self.sample(1)

    def restore(self):
        for dst, src in self.keep:
            dst.copy_(src)

    def loop(self):
        for h in range(H0):
            self.env.step_tensor(self.acts[h], want_obs=False)

    def sample(self, n=N_INNER):
        return timed(self.torch, self.loop, self.restore, n)


def worker(pkg):
    s = StepLoop(pkg)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() == "time":
            print(f"ms {s.sample():.6f}", flush=True)
        else:
            break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", default=None, help="built greenlight-gym2_amd directory of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plan_rollout_cost.txt"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker))
    torch, TomatoVecEnv, synthetic_weather = setup(ROOT / "greenlight-gym2_amd")
    if not torch.cuda.is_available():
        sys.exit("plan_cost.py needs a GPU (no fallback)")
    import numpy as np
    lines = [f"device-side planning: cost on {torch.cuda.get_device_name(0)} (tools/plan_cost.py)", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731

    # ---- 1. overhead per step ------------------------------------------------------------------------------------------------
    w = synthetic_weather(n_rows=35040)
    par = parent_states(torch, TomatoVecEnv, w)
    plan = par.planner(K0, H0)
    acts = horizon_actions(torch, par.device)
    if args.parent_pkg:
        child = subprocess.Popen([sys.executable, __file__, "--worker", str(Path(args.parent_pkg).resolve())], stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, text=True)
        assert child.stdout.readline().strip() == "ready", "the parent-commit worker did not start"

        def loop_sample():
            child.stdin.write("time\n")
            child.stdin.flush()
            return float(child.stdout.readline().split()[1])
        loop_where = "a child process on the parent commit's build (--parent-pkg)"
    else:
        child, local = None, StepLoop(ROOT / "greenlight-gym2_amd")
        loop_sample = local.sample
        loop_where = "THIS build (no --parent-pkg given; its step kernels are the parent commit's instruction for instruction)"
    for _ in range(N_WARM):
        timed(torch, lambda: plan.rollout(acts), n=1)
    roll, loop = [], []
    for _ in range(N_SAMPLES):                       # alternating
        roll.append(timed(torch, lambda: plan.rollout(acts)))
        loop.append(loop_sample())
    if child:
        child.stdin.write("quit\n")
        child.stdin.flush()
        child.wait(timeout=60)
    ret, alive, steps, _, failed = plan.rollout(acts)
    assert int(steps.min()) == H0 and int(alive.min()) == 1 and int(failed.max()) == 0
    if not args.parent_pkg:                          # same process: the returns are the loop's rewards, a check on "the same work"
        local.restore()
        tot = torch.zeros(B0 * K0, dtype=torch.float64, device=par.device)
        for h in range(H0):
            tot += local.env.step_tensor(local.acts[h], want_obs=False)[1].double()
        assert torch.equal(tot, ret.reshape(-1))
    m_roll, m_loop = statistics.median(roll), statistics.median(loop)
    ratio = m_roll / m_loop
    say(f"1. overhead per step: fp32 ls5-128, B x K = {B0} x {K0} = {B0 * K0} children, H = {H0}; device events, {N_WARM} warm-up windows, "
        f"{N_SAMPLES} alternating samples of {N_INNER} horizons each; ms per horizon")
    say(f"   step loop = {H0} x step_tensor(want_obs=False), {B0 * K0} envs, auto_reset=False, same states and actions, in {loop_where}")
    say("   Planner.rollout (fork + 20 x (step + accumulate)): " + " ".join(f"{v:.3f}" for v in roll))
    say("   step loop                                        : " + " ".join(f"{v:.3f}" for v in loop))
    say(f"   medians {m_roll:.3f} / {m_loop:.3f} ms  ({m_roll / H0:.4f} / {m_loop / H0:.4f} ms per step);  spread of the loop samples "
        f"{(max(loop) - min(loop)) / m_loop * 100:.1f} %, of the rollout samples {(max(roll) - min(roll)) / m_roll * 100:.1f} %")
    say(f"   ratio rollout / loop = {ratio:.4f}   (requirement <= 1.05: {'met' if ratio <= 1.05 else 'NOT MET'})")
    say(f"   rollout rate {B0 * K0 * H0 / m_roll * 1e3:.3e} candidate env-steps/s")
    say()
    del plan
    par.close()

    # ---- 2. fork, select, end to end -----------------------------------------------------------------------------------------
    say("2. glgym_plan_fork / glgym_plan_select / end to end, fp32 ls5-128, H = 48; device events, mean of 20 calls after 3 (fork, select), "
        "median of 5 (end to end)")
    for B, K, H in ((64, 1024, 48), (8, 8192, 48)):
        env = TomatoVecEnv(B, weather=w, dtype="float32", season_length=SEASON, start_rows=list(range(0, 96 * B, 96)), seed=5, auto_reset=False)
        env.reset_tensor()
        plan = env.planner(K, H)
        g = torch.Generator().manual_seed(3)
        a = (torch.rand(H, B * K, 6, generator=g) * 2 - 1).to(env.device).contiguous()
        a[:, ::K] = 0.0

        def whole():
            plan.rollout(a)
            plan.select()
        e2e = statistics.median(timed(torch, whole, n=1) for _ in range(5))
        for _ in range(3):
            plan.fork(); plan.select(); plan.select(temperature=1.0); plan.select(sequence=True)
        plan.rollout(a)
        t_fork = timed(torch, plan.fork, n=20)
        plan.rollout(a)
        t_sel = timed(torch, plan.select, n=20)
        t_seq = timed(torch, lambda: plan.select(sequence=True), n=20)
        t_mppi = timed(torch, lambda: plan.select(temperature=1.0), n=20)
        say(f"   (B, K, H) = ({B}, {K}, {H}): fork {t_fork * 1e3:.1f} us, select {t_sel * 1e3:.1f} us, with best_sequence {t_seq * 1e3:.1f} us, "
            f"with the MPPI mean {t_mppi * 1e3:.1f} us ({H * B * K * 24 / (t_mppi - t_sel) / 1e6:.0f} GB/s on the action block); "
            f"fork + rollout + select {e2e:.2f} ms = {B * K * H / e2e * 1e3:.3e} candidate env-steps/s")
        env.close()
    say()

    # ---- 3. the reference environment's fixture ------------------------------------------------------------------------------
    fx = ROOT / "tests" / "golden" / "refenv_1day.npz"
    if fx.exists():
        g = np.load(fx, allow_pickle=False)
        say("3. free-running H = 97 rollout of the reference TomatoEnv's random-action episode (tests/golden/refenv_1day.npz, leg ra), "
            "bound 97 x 2e-4 = 1.94e-2")
        for dtype in ("float64", "float32"):
            env = TomatoVecEnv(1, weather=g["weather"], params=g["p"], dtype=dtype, season_length=1, pred_horizon=0.5, start_rows=[0],
                               start_days=[0.0], auto_reset=False)
            env.reset_tensor()
            env.x.copy_(torch.as_tensor(g["ra_x"][:1], dtype=env.tdtype, device=env.device))
            a = torch.as_tensor(np.ascontiguousarray(g["ra_actions"][:97], dtype=np.float32), device=env.device).view(97, 1, 6)
            ret, alive, steps, _, _ = env.planner(1, 97).rollout(a)
            ref = float(np.sum(g["ra_reward"].astype(np.float64)))
            say(f"   {dtype}: return {float(ret[0, 0]):.6f}, sum ra_reward {ref:.6f}, |difference| {abs(float(ret[0, 0]) - ref):.3e}, "
                f"steps {int(steps[0, 0])}, alive {int(alive[0, 0])}")
            env.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if ratio <= 1.05 else 1


if __name__ == "__main__":
    sys.exit(main())
