#!/usr/bin/env python3
"""Receding-horizon random-shooting MPC on the device (gl_gym_amd.planner.Planner; include/glgym.h glgym_plan_*).

    python examples/mpc_random_shooting.py [--season 2] [--candidates 1024] [--horizon 48] [--gamma 1.0] [--temperature T]

8 greenhouses; at every step each one simulates K candidate action sequences over H steps on forked copies of itself, and applies the
first action of the best one (with --temperature: of the MPPI-weighted mean sequence).  Candidate 0 is always the all-zero sequence
("hold the controls"), so the plan is never worse, over its horizon and on its model, than doing nothing.

This is PERFECT-FORECAST MPC: the candidates are simulated on the true future rows of the (synthetic) weather table, clamped at its
end.  The episode return is printed beside that of the same greenhouses under the rule-based controller; the script makes no claim
about which is better -- K, H and the sampling distribution are untuned."""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "greenlight-gym2_amd"))

from gl_gym_amd.baseline import RuleBasedController          # noqa: E402
from gl_gym_amd.tomato_env import TomatoVecEnv               # noqa: E402
from gl_gym_amd.utils import synthetic_weather               # noqa: E402

N_ENVS = 8


def make_env(w, season, dtype):
    starts = [96 * 30 * k for k in range(N_ENVS)]            # eight start days, a month apart
    return TomatoVecEnv(N_ENVS, weather=w, dtype=dtype, season_length=season, start_rows=starts, start_days=[s / 96.0 for s in starts],
                        seed=666, auto_reset=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--season", type=float, default=2, help="season length [days]")
    ap.add_argument("--candidates", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=48, help="planning horizon [env-steps of 15 min]")
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--temperature", type=float, default=None, help="apply the MPPI mean's first action instead of the best candidate's")
    ap.add_argument("--dtype", default="float32")
    args = ap.parse_args()
    import torch

    w = synthetic_weather(n_rows=35040)
    K, H = args.candidates, args.horizon
    env = make_env(w, args.season, args.dtype)
    env.reset_tensor()
    plan = env.planner(K, H, gamma=args.gamma)
    gen = torch.Generator(device=env.device).manual_seed(0)
    acts = torch.empty(H, N_ENVS, K, 6, dtype=torch.float32, device=env.device)
    n_steps = env.N + 1
    total = torch.zeros(N_ENVS, dtype=torch.float64, device=env.device)
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(n_steps):
        acts.uniform_(-1.0, 1.0, generator=gen)
        acts[:, :, 0] = 0.0                                   # candidate 0: hold the controls
        plan.rollout(acts)
        sel = plan.select(temperature=args.temperature)
        first = sel["mean_sequence"][0] if args.temperature else sel["best_action"]
        _, r, done, _ = env.step_tensor(first.contiguous(), want_obs=False)
        total += r.double()
    torch.cuda.synchronize()
    el = time.time() - t0
    assert bool(done.all())
    mpc = total.cpu().numpy()

    rb_env = make_env(w, args.season, args.dtype)
    rb_env.reset_tensor()
    ctrl = RuleBasedController()
    total_rb = torch.zeros(N_ENVS, dtype=torch.float64, device=env.device)
    for _ in range(n_steps):
        _, r, done, _ = rb_env.step_tensor(controller=ctrl, want_obs=False)
        total_rb += r.double()
    rb = total_rb.cpu().numpy()

    print(f"{N_ENVS} greenhouses x {n_steps} steps, {K} candidates x {H} steps per decision: {el:.2f} s "
          f"({N_ENVS * K * H * n_steps / el:.3e} candidate env-steps/s incl. sampling and the host loop)")
    print(f"MPC episode return {mpc.mean():.4f} (per greenhouse: {' '.join(f'{v:.3f}' for v in mpc)})")
    print(f"rule-based {rb.mean():.4f} (per greenhouse: {' '.join(f'{v:.3f}' for v in rb)})")
    print(f"ODE failures: MPC env {int(env.metrics()['n_ode_fail'])}, rule-based env {int(rb_env.metrics()['n_ode_fail'])}")
    env.close()
    rb_env.close()


if __name__ == "__main__":
    main()
