#!/usr/bin/env python3
"""Receding-horizon MPC under weather-forecast uncertainty (gl_gym_amd.planner.Planner with weather_sigma; include/glgym.h
glgym_plan_weather).

    python examples/mpc_forecast.py [--season 2] [--candidates 256] [--scenarios 8] [--tail 2] [--horizon 24] [--iters 3] [--elites 32]
                                    [--phi 0.9] [--sigma-iglob 0.2] [--sigma-tout 1.5] [--sigma-vpout 0.1] [--sigma-wind 0.3]
                                    [--sigma-tsky 2.0]

Three identical copies of 8 greenhouses on the true weather (no crop noise), each steered by the cross-entropy method with another
view of the coming weather:
  * perfect forecast: every candidate is simulated on the true future rows of the weather table (examples/mpc_cem.py);
  * one wrong forecast: n_scenarios = 1 -- certainty-equivalent MPC on a single forecast whose error grows with the lead time;
  * --scenarios forecast scenarios, scored by the mean of the --tail worst returns; all candidates of a greenhouse see the same
    futures (common random numbers), which stay fixed over the iterations of one decision and are redrawn for the next.
The forecast error is zero at the row being integrated, lag-1 correlated along the horizon (--phi) and saturates at the given
sigmas: relative for iGlob, vpOut and wind, kelvin for tOut and tSky.  All three apply the first action of their best sequence to
the true plant; the realised returns are printed side by side.  The script makes no claim about which is better -- every setting is
untuned."""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "greenlight-gym2_amd"))

from gl_gym_amd.tomato_env import TomatoVecEnv               # noqa: E402
from gl_gym_amd.utils import synthetic_weather               # noqa: E402

N_ENVS = 8


def make_env(w, season, dtype):
    starts = [96 * 30 * k for k in range(N_ENVS)]            # eight start days, a month apart
    return TomatoVecEnv(N_ENVS, weather=w, dtype=dtype, season_length=season, start_rows=starts, start_days=[s / 96.0 for s in starts],
                        seed=666, auto_reset=False)


def closed_loop(env, plan, args):
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
        if plan.S:
            plan.new_scenarios()                              # the next decision gets a fresh forecast
    torch.cuda.synchronize()
    assert bool(done.all())
    return total.cpu().numpy(), int(no_plan.sum()), time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--season", type=float, default=2, help="season length [days]")
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--scenarios", type=int, default=8, help="forecast scenarios per candidate of the third planner")
    ap.add_argument("--tail", type=int, default=2, help="score = mean of the worst --tail scenario returns (= --scenarios: the mean)")
    ap.add_argument("--horizon", type=int, default=24, help="planning horizon [env-steps of 15 min]")
    ap.add_argument("--iters", type=int, default=3, help="CEM iterations per decision")
    ap.add_argument("--elites", type=int, default=32)
    ap.add_argument("--beta", type=float, default=0.5, help="lag-1 correlation of the sampling noise along the horizon")
    ap.add_argument("--carry", type=int, default=4, help="elites kept from one population to the next")
    ap.add_argument("--init-std", type=float, default=0.5)
    ap.add_argument("--gamma", type=float, default=1.0)
    ap.add_argument("--phi", type=float, default=0.9, help="lag-1 correlation of the forecast error along the horizon")
    ap.add_argument("--sigma-iglob", type=float, default=0.2, help="relative")
    ap.add_argument("--sigma-tout", type=float, default=1.5, help="[K]")
    ap.add_argument("--sigma-vpout", type=float, default=0.1, help="relative")
    ap.add_argument("--sigma-wind", type=float, default=0.3, help="relative")
    ap.add_argument("--sigma-tsky", type=float, default=2.0, help="[K]")
    ap.add_argument("--dtype", default="float32")
    args = ap.parse_args()

    w = synthetic_weather(n_rows=35040)
    K, S, H = args.candidates, args.scenarios, args.horizon
    sigma = {"iGlob": args.sigma_iglob, "tOut": args.sigma_tout, "vpOut": args.sigma_vpout, "wind": args.sigma_wind, "tSky": args.sigma_tsky}
    envs = [make_env(w, args.season, args.dtype) for _ in range(3)]
    for env in envs:
        env.reset_tensor()
    forecast = dict(gamma=args.gamma, noise_scale=0.0, weather_sigma=sigma, weather_phi=args.phi, scenario_seed=667)
    planners = [envs[0].planner(K, H, gamma=args.gamma),
                envs[1].planner(K, H, n_scenarios=1, **forecast),
                envs[2].planner(K, H, n_scenarios=S, n_tail=args.tail, **forecast)]
    names = ["perfect forecast (the true future rows)", "one wrong forecast (n_scenarios = 1)",
             f"{S} forecast scenarios (mean of the worst {args.tail})"]
    n_steps = envs[0].N + 1
    results = [closed_loop(env, plan, args) for env, plan in zip(envs, planners)]

    print(f"{N_ENVS} greenhouses x {n_steps} steps, {args.iters} iterations x {K} candidates x {H} steps per decision, {args.elites} elites; "
          f"forecast error phi = {args.phi}, sigma = {sigma}")
    for name, plan, (ret, none, el) in zip(names, planners, results):
        print(f"CEM-MPC, {name}: closed-loop return {ret.mean():.4f} (per greenhouse: {' '.join(f'{v:.3f}' for v in ret)}), {el:.2f} s "
              f"({N_ENVS * K * (plan.S or 1) * H * args.iters * n_steps / el:.3e} env-steps/s incl. every stage and the host loop), "
              f"{none} decisions without an admissible candidate")
    print("ODE failures of the plants: " + " ".join(str(int(env.metrics()["n_ode_fail"])) for env in envs))
    for env in envs:
        env.close()


if __name__ == "__main__":
    main()
