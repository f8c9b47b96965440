#!/usr/bin/env python3
"""Robust receding-horizon MPC under crop-parameter noise (gl_gym_amd.planner.Planner with n_scenarios; include/glgym.h
glgym_plan_scenario, glgym_plan_rollout_scenarios, glgym_plan_aggregate).

    python examples/mpc_robust.py [--season 2] [--candidates 256] [--scenarios 8] [--tail 4] [--horizon 24] [--iters 3] [--elites 32]
                                  [--scale 0.2] [--noise step]

8 greenhouses whose 34 crop parameters are multiplied by 1 + U(-scale/2, scale/2) at every env-step (uncertainty_scale, the
reference's noise.py).  Two planners decide for two identically seeded copies of them, by the cross-entropy method:
  * the robust one simulates every candidate sequence under --scenarios sampled futures of the crop block and scores it by the mean
    of its --tail worst returns; all candidates of a greenhouse see the same futures (common random numbers), which stay fixed over
    the iterations of one decision and are redrawn for the next;
  * the nominal one scores every candidate on ONE deterministic future with the handle's crop parameters (examples/mpc_cem.py).
Both apply the first action of their best sequence to the noisy plant; the closed-loop returns are printed side by side.  The
script makes no claim about which is better -- every setting is untuned.  The two plants share seed and draw counter, so both meet
the same sequence of crop blocks."""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "greenlight-gym2_amd"))

from gl_gym_amd.tomato_env import TomatoVecEnv               # noqa: E402
from gl_gym_amd.utils import synthetic_weather               # noqa: E402

N_ENVS = 8


def make_env(w, season, dtype, scale):
    starts = [96 * 30 * k for k in range(N_ENVS)]            # eight start days, a month apart
    return TomatoVecEnv(N_ENVS, weather=w, dtype=dtype, season_length=season, start_rows=starts, start_days=[s / 96.0 for s in starts],
                        seed=666, auto_reset=False, uncertainty_scale=scale)


def closed_loop(env, plan, args, robust):
    import torch
    total = torch.zeros(N_ENVS, dtype=torch.float64, device=env.device)
    no_plan = torch.zeros(N_ENVS, dtype=torch.int64, device=env.device)
    mean_t = std_t = None                                     # the first decision starts from zeros
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(env.N + 1):
        out = plan.cem(args.iters, args.elites, init_std=args.init_std, beta=args.beta, carry=min(args.carry, args.elites), seed=666,
                       mean_t=mean_t, std_t=std_t)
        no_plan += (out["best_k"] < 0).long()
        _, r, done, _ = env.step_tensor(out["best_action"].contiguous(), want_obs=False)
        total += r.double()
        mean_t, std_t = plan.shift(args.init_std)
        if robust:
            plan.new_scenarios()                              # the next decision looks at other futures
    torch.cuda.synchronize()
    assert bool(done.all())
    return total.cpu().numpy(), int(no_plan.sum()), time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--season", type=float, default=2, help="season length [days]")
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=8, help="sampled futures per candidate")
    ap.add_argument("--tail", type=int, default=4, help="score = mean of the worst --tail scenario returns (= --scenarios: the mean)")
    ap.add_argument("--horizon", type=int, default=24, help="planning horizon [env-steps of 15 min]")
    ap.add_argument("--iters", type=int, default=3, help="CEM iterations per decision")
    ap.add_argument("--elites", type=int, default=32)
    ap.add_argument("--beta", type=float, default=0.5, help="lag-1 correlation of the sampling noise along the horizon")
    ap.add_argument("--carry", type=int, default=4, help="elites kept from one population to the next")
    ap.add_argument("--init-std", type=float, default=0.5)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--scale", type=float, default=0.2, help="uncertainty_scale of the plant and of the sampled futures")
    ap.add_argument("--noise", default="step", choices=["step", "hold"], help="a fresh draw at every horizon step, or one held draw")
    ap.add_argument("--dtype", default="float32")
    args = ap.parse_args()
    if not args.scale > 0:
        ap.error("--scale must be > 0: this example is about the noisy plant")

    w = synthetic_weather(n_rows=35040)
    K, S, H = args.candidates, args.scenarios, args.horizon
    env_r, env_n = make_env(w, args.season, args.dtype, args.scale), make_env(w, args.season, args.dtype, args.scale)
    env_r.reset_tensor()
    env_n.reset_tensor()
    robust = env_r.planner(K, H, gamma=args.gamma, n_scenarios=S, n_tail=args.tail, noise=args.noise, scenario_seed=667)
    nominal = env_n.planner(K, H, gamma=args.gamma)
    n_steps = env_r.N + 1
    ret_r, none_r, el_r = closed_loop(env_r, robust, args, True)
    ret_n, none_n, el_n = closed_loop(env_n, nominal, args, False)

    print(f"{N_ENVS} greenhouses x {n_steps} steps at uncertainty_scale {args.scale}, {args.iters} iterations x {K} candidates x {H} steps per "
          f"decision, {args.elites} elites")
    print(f"robust CEM-MPC ({S} scenarios, noise={args.noise}, mean of the worst {args.tail}): closed-loop return {ret_r.mean():.4f} "
          f"(per greenhouse: {' '.join(f'{v:.3f}' for v in ret_r)}), {el_r:.2f} s "
          f"({N_ENVS * K * S * H * args.iters * n_steps / el_r:.3e} scenario env-steps/s incl. every stage and the host loop)")
    print(f"nominal CEM-MPC (one deterministic future): closed-loop return {ret_n.mean():.4f} "
          f"(per greenhouse: {' '.join(f'{v:.3f}' for v in ret_n)}), {el_n:.2f} s")
    print(f"decisions without an admissible candidate: robust {none_r}, nominal {none_n}")
    print(f"ODE failures: robust plant {int(env_r.metrics()['n_ode_fail'])}, nominal plant {int(env_n.metrics()['n_ode_fail'])}")
    env_r.close()
    env_n.close()


if __name__ == "__main__":
    main()
