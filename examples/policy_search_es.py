#!/usr/bin/env python3
"""Policy search by an evolution strategy on the device (gl_gym_amd.planner.PolicySearch.es; include/glgym.h glgym_plan_es_sample,
glgym_plan_es_utilities, glgym_plan_es_update).

    python examples/policy_search_es.py [--envs 4] [--candidates 256] [--horizon 96] [--iters 10] [--lr 0.03] [--lr-std 0.1]
                                        [--optimizer adam] [--scenarios 0]

The setting of examples/policy_search.py: a handful of greenhouses a month apart in the (synthetic) weather year, 23 observation
columns, every candidate a set of weights rolled out closed-loop on forked copies of ALL greenhouses (share="all") and scored by its
mean return.  Instead of refitting a Gaussian to the best few, every iteration draws the candidates in mirrored pairs around the mean,
turns the returns of the WHOLE population into centred ranks, and takes one search-gradient step on the mean (Adam or SGD) and one
on the per-parameter spread.  Printed per iteration: the best candidate's score and the smallest and largest spread; at the end the
return of the MEAN policy (evaluate(mean)), which is what the strategy optimises, next to the rule-based controller's.

This is PERFECT-FORECAST search over ONE day from ONE state: it shows the machinery; it trains no policy worth deploying."""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "greenlight-gym2_amd"))

from gl_gym_amd.baseline import RuleBasedController          # noqa: E402
from gl_gym_amd.planner import MLPSpec                       # noqa: E402
from gl_gym_amd.tomato_env import TomatoVecEnv               # noqa: E402
from gl_gym_amd.utils import synthetic_weather               # noqa: E402

RULE_TUNE = {"temp_setpoint_day": (17.0, 23.0)}              # RuleSearch wants a search space; only the default controller is rolled out


def search(env, name, spec, args, scen):
    ps = env.policy_search(args.candidates, args.horizon, spec, share="all", **scen)
    for it in range(args.iters):                             # one iteration per call; resume keeps mean, spread, moments and step count
        out = ps.es(1, lr=args.lr, lr_std=args.lr_std, init_std=args.init_std, min_std=0.01, optimizer=args.optimizer, seed=666,
                    resume=it > 0)
        print(f"{name:14s} iteration {it + 1}: best score {float(out['best_return'][0]):.4f}  "
              f"spread {float(out['std'].min()):.3f} .. {float(out['std'].max()):.3f}")
    per_greenhouse = ps.evaluate(ps.mean_t)[0][:, 0].cpu().numpy()
    print(f"{name:14s} {spec.D} parameters; the mean policy: score {per_greenhouse.mean():.4f} "
          f"(per greenhouse: {' '.join(f'{v:.3f}' for v in per_greenhouse)})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--candidates", type=int, default=256, help="even: the population is drawn in mirrored pairs")
    ap.add_argument("--horizon", type=int, default=96, help="env-steps of 15 min (96: one day)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--lr", type=float, default=0.03)
    ap.add_argument("--lr-std", type=float, default=0.1)
    ap.add_argument("--init-std", type=float, default=0.1)
    ap.add_argument("--optimizer", default="adam", choices=("adam", "sgd"))
    ap.add_argument("--scenarios", type=int, default=0, help="crop-noise scenarios per candidate (0: none)")
    ap.add_argument("--dtype", default="float32")
    args = ap.parse_args()

    B = args.envs
    starts = [96 * 30 * k for k in range(B)]
    env = TomatoVecEnv(B, weather=synthetic_weather(n_rows=35040), dtype=args.dtype, season_length=10, pred_horizon=0.0, start_rows=starts,
                       start_days=[s / 96.0 for s in starts], seed=666, auto_reset=False)
    env.reset_tensor()
    base = RuleBasedController()
    seen = []
    for _ in range(96):                                       # a first day under the default controller: the observations' statistics
        seen.append(env.step_tensor(controller=base, want_obs=True)[0].double().cpu().numpy().copy())
    seen = np.concatenate(seen)
    norm = (seen.mean(axis=0), seen.var(axis=0), 1e-8, 10.0)
    scen = dict(n_scenarios=args.scenarios, noise_scale=0.2) if args.scenarios else {}
    print(f"{B} greenhouses, {args.iters} iterations x {args.candidates} candidate policies x {args.horizon} closed-loop steps"
          + (f" x {args.scenarios} scenarios" if args.scenarios else "") + f", {env.obs_dim} observation columns, {args.optimizer}")
    rules = env.rule_search(1, args.horizon, tune=RULE_TUNE, base=base, **scen)
    rule_ret = rules.rollout(rules.theta_of(base))[0][:, 0].cpu().numpy()
    print(f"rule-based controller, default constants: score {rule_ret.mean():.4f} (per greenhouse: {' '.join(f'{v:.3f}' for v in rule_ret)})")
    search(env, "linear", MLPSpec(env.obs_dim, (), squash="clip", scale=[1.0 / np.sqrt(env.obs_dim), 0.5], obs_norm=norm), args, scen)
    search(env, "23-32-6 tanh", MLPSpec(env.obs_dim, (32,), activation="tanh", squash="clip",
                                        scale=[2.0 / np.sqrt(env.obs_dim), 0.5, 0.5, 0.5], obs_norm=norm), args, scen)
    env.close()


if __name__ == "__main__":
    main()
