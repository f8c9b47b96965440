#!/usr/bin/env python3
"""Receding-horizon MPC by the cross-entropy method on the device (gl_gym_amd.planner.Planner.cem; include/glgym.h glgym_plan_sample,
glgym_plan_elites, glgym_plan_refit).

    python examples/mpc_cem.py [--season 2] [--candidates 1024] [--horizon 48] [--iters 3] [--elites 64] [--beta 0.5] [--carry 4]

8 greenhouses; at every step each one draws K candidate action sequences from a Gaussian per (horizon step, actuator), simulates them
over H steps on forked copies of itself, refits the Gaussian to the best --elites of them, repeats that --iters times, and applies the
first action of the best sequence of the last population.  The distribution is then shifted by one step and warm-starts the next
decision.  Candidate 0 is always the distribution's mean and the first population starts from "hold the controls".

This is PERFECT-FORECAST MPC: the candidates are simulated on the true future rows of the (synthetic) weather table, clamped at its
end.  The episode return is printed beside that of the same greenhouses under the rule-based controller; the script makes no claim
about which is better -- K, H, the number of iterations and the spreads are untuned."""
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
    ap.add_argument("--iters", type=int, default=3, help="CEM iterations per decision")
    ap.add_argument("--elites", type=int, default=64)
    ap.add_argument("--beta", type=float, default=0.5, help="lag-1 correlation of the sampling noise along the horizon")
    ap.add_argument("--carry", type=int, default=4, help="elites kept from one population to the next")
    ap.add_argument("--init-std", type=float, default=0.5)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--dtype", default="float32")
    args = ap.parse_args()
    import torch

    w = synthetic_weather(n_rows=35040)
    K, H = args.candidates, args.horizon
    env = make_env(w, args.season, args.dtype)
    env.reset_tensor()
    plan = env.planner(K, H, gamma=args.gamma)
    n_steps = env.N + 1
    total = torch.zeros(N_ENVS, dtype=torch.float64, device=env.device)
    no_plan = torch.zeros(N_ENVS, dtype=torch.int64, device=env.device)
    torch.cuda.synchronize()
    t0 = time.time()
    mean_t = std_t = None                                     # the first decision starts from zeros
    for _ in range(n_steps):
        out = plan.cem(args.iters, args.elites, init_std=args.init_std, beta=args.beta, carry=min(args.carry, args.elites), seed=666,
                       mean_t=mean_t, std_t=std_t)
        no_plan += (out["best_k"] < 0).long()
        _, r, done, _ = env.step_tensor(out["best_action"].contiguous(), want_obs=False)
        total += r.double()
        mean_t, std_t = plan.shift(args.init_std)
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

    print(f"{N_ENVS} greenhouses x {n_steps} steps, {args.iters} iterations x {K} candidates x {H} steps per decision, {args.elites} elites: "
          f"{el:.2f} s ({N_ENVS * K * H * args.iters * n_steps / el:.3e} candidate env-steps/s incl. sampling, ranking, refit and the host loop)")
    print(f"CEM-MPC episode return {mpc.mean():.4f} (per greenhouse: {' '.join(f'{v:.3f}' for v in mpc)})")
    print(f"rule-based {rb.mean():.4f} (per greenhouse: {' '.join(f'{v:.3f}' for v in rb)})")
    print(f"decisions without an admissible candidate: {int(no_plan.sum())}")
    print(f"ODE failures: MPC env {int(env.metrics()['n_ode_fail'])}, rule-based env {int(rb_env.metrics()['n_ode_fail'])}")
    env.close()
    rb_env.close()


if __name__ == "__main__":
    main()
