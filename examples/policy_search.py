#!/usr/bin/env python3
"""Gradient-free policy search on the device (gl_gym_amd.planner.PolicySearch; include/glgym.h glgym_policy_rows,
glgym_plan_rollout_policy).

    python examples/policy_search.py [--envs 4] [--candidates 256] [--horizon 96] [--iters 6] [--elites 32] [--carry 2] [--scenarios 0]

A handful of greenhouses, a month apart in the (synthetic) weather year, without the forecast in the observation (pred_horizon = 0:
23 columns).  The cross-entropy method searches the weights of a LINEAR policy (23 -> 6) and of a 23 -> 16 -> 6 tanh policy over a
horizon of one day: every candidate is a set of weights, rolled out closed-loop on forked copies of ALL greenhouses (share="all": its
action at step h follows from the child's own observation after step h-1) and scored by its mean return.  Printed per iteration: the
best score, next to the score of the rule-based controller with its default constants from RuleSearch.rollout on the same fork.
--scenarios S > 0 scores every policy under S sampled futures of the crop parameters (mean) instead of one.

The observations are normalised with the statistics of a first day under the rule-based controller.  This is PERFECT-FORECAST search
over ONE day from ONE state with a few thousand rollouts: it shows the machinery; it trains no policy worth deploying."""
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
    E, carry = min(args.elites, args.candidates), min(args.carry, args.elites, args.candidates)
    ps.mean_t.zero_()                                        # theta = 0: the policy that holds the controls
    ps.std_t.fill_(args.init_std)
    for it in range(args.iters):
        pop = ps.sample(ps.mean_t, ps.std_t, seed=666, draw_index=it, carry=carry)
        ps.rollout(pop)
        ps.elites(E)
        ps.refit(ps.mean_t, ps.std_t, 0.1, 0.02)
        best = ps.select()
        print(f"{name:14s} iteration {it + 1}: best score {float(best['best_return'][0]):.4f}")
    per_greenhouse = ps.evaluate(ps.best_theta())[0][:, 0].cpu().numpy()
    print(f"{name:14s} {spec.D} parameters; the best policy per greenhouse: {' '.join(f'{v:.3f}' for v in per_greenhouse)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=96, help="env-steps of 15 min (96: one day)")
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--elites", type=int, default=32)
    ap.add_argument("--carry", type=int, default=2)
    ap.add_argument("--init-std", type=float, default=0.5)
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
          + (f" x {args.scenarios} scenarios" if args.scenarios else "") + f", {env.obs_dim} observation columns")
    rules = env.rule_search(1, args.horizon, tune=RULE_TUNE, base=base, **scen)
    rule_ret = rules.rollout(rules.theta_of(base))[0][:, 0].cpu().numpy()
    print(f"rule-based controller, default constants: score {rule_ret.mean():.4f} (per greenhouse: {' '.join(f'{v:.3f}' for v in rule_ret)})")
    # the scale is the search bound of a parameter: weights 1 / sqrt(fan_in), biases 0.5
    search(env, "linear", MLPSpec(env.obs_dim, (), squash="clip", scale=[1.0 / np.sqrt(env.obs_dim), 0.5], obs_norm=norm), args, scen)
    search(env, "23-16-6 tanh", MLPSpec(env.obs_dim, (16,), activation="tanh", squash="clip",
                                        scale=[2.0 / np.sqrt(env.obs_dim), 0.5, 0.5, 0.5], obs_norm=norm), args, scen)
    env.close()


if __name__ == "__main__":
    main()
