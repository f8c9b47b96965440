#!/usr/bin/env python3
"""Tune the rule-based controller's setpoints on the device (gl_gym_amd.planner.RuleSearch; include/glgym.h glgym_rule_rows,
glgym_plan_rollout_rule).

    python examples/tune_rule_based.py [--envs 4] [--candidates 256] [--horizon 96] [--iters 4] [--elites 32] [--carry 2] [--scenarios 0]

A handful of greenhouses, a month apart in the (synthetic) weather year; for each one the cross-entropy method searches five constants
of the rule-based controller -- day and night temperature setpoint, the CO2 setpoint, the humidity limit and the lamps' switch-off hour
-- over a horizon of one day: every candidate is a CONTROLLER, rolled out closed-loop on a forked copy of the greenhouse (its controls
at step h follow from its own state after step h-1).  Printed: the return of the default controller over that horizon, the tuned one,
and the tuned values.  --scenarios S > 0 tunes against S sampled futures of the crop parameters (mean score) instead of one.

This is PERFECT-FORECAST tuning over ONE day from ONE state: the tuned values fit that day; the script makes no claim beyond it."""
import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "greenlight-gym2_amd"))

from gl_gym_amd.baseline import RuleBasedController          # noqa: E402
from gl_gym_amd.tomato_env import TomatoVecEnv               # noqa: E402
from gl_gym_amd.utils import synthetic_weather               # noqa: E402

TUNE = {"temp_setpoint_day": (17.0, 23.0), "temp_setpoint_night": (14.0, 19.0), "co2_day": (400.0, 1200.0), "rh_max": (75.0, 95.0),
        "lamps_off": (12.0, 22.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--candidates", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=96, help="env-steps of 15 min (96: one day)")
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--elites", type=int, default=32)
    ap.add_argument("--carry", type=int, default=2)
    ap.add_argument("--init-std", type=float, default=0.5)
    ap.add_argument("--scenarios", type=int, default=0, help="crop-noise scenarios per candidate (0: none)")
    ap.add_argument("--dtype", default="float32")
    args = ap.parse_args()

    B = args.envs
    starts = [96 * 30 * k for k in range(B)]
    env = TomatoVecEnv(B, weather=synthetic_weather(n_rows=35040), dtype=args.dtype, season_length=10, start_rows=starts,
                       start_days=[s / 96.0 for s in starts], seed=666, auto_reset=False)
    env.reset_tensor()
    base = RuleBasedController()
    for _ in range(4):                                        # a first hour under the default controller
        env.step_tensor(controller=base, want_obs=False)
    scen = dict(n_scenarios=args.scenarios, noise_scale=0.2) if args.scenarios else {}
    search = env.rule_search(args.candidates, args.horizon, tune=TUNE, base=base, **scen)
    default_ret = search.rollout(search.theta_of(base))[0][:, 0].cpu().numpy()
    out = search.cem(args.iters, min(args.elites, args.candidates), init_std=args.init_std, carry=min(args.carry, args.elites), seed=666)
    tuned_ret = out["best_return"].cpu().numpy()
    print(f"{B} greenhouses, {args.iters} iterations x {args.candidates} candidate controllers x {args.horizon} closed-loop steps"
          + (f" x {args.scenarios} scenarios" if args.scenarios else ""))
    print(f"default controller: return over the horizon {default_ret.mean():.4f} (per greenhouse: {' '.join(f'{v:.3f}' for v in default_ret)})")
    print(f"tuned controller  : return over the horizon {tuned_ret.mean():.4f} (per greenhouse: {' '.join(f'{v:.3f}' for v in tuned_ret)})")
    for name in TUNE:
        vals = out["best_params"][name].cpu().numpy()
        print(f"  {name:20s} default {getattr(base, name):8.2f}   tuned " + " ".join(f"{v:8.2f}" for v in vals))
    best0 = search.best_controller(0)
    assert all(TUNE[n][0] <= getattr(best0, n) <= TUNE[n][1] for n in TUNE)
    print(f"greenhouses without an admissible candidate: {int((out['best_k'] < 0).sum())}")
    env.close()


if __name__ == "__main__":
    main()
