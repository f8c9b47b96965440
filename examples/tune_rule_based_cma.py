#!/usr/bin/env python3
"""Tune the rule-based controller's setpoints by CMA-ES with a full covariance matrix, next to the cross-entropy method
(gl_gym_amd.planner.RuleSearch.cma / .cem; include/glgym.h glgym_plan_cma_sample, glgym_plan_cma_update).

    python examples/tune_rule_based_cma.py [--method cma|cem] [--envs 4] [--candidates 64] [--horizon 96] [--iters 8] [--scenarios 0]

The setting of examples/tune_rule_based.py: a handful of greenhouses, a month apart in the (synthetic) weather year, five constants of
the rule-based controller -- day and night temperature setpoint, the CO2 setpoint, the humidity limit and the lamps' switch-off hour --
searched over a horizon of one day, every candidate a CONTROLLER rolled out closed-loop on a forked copy of the greenhouse.  --method
picks the search whose tuned values are printed; BOTH searches run with the same candidates, iterations and seed, and both returns are
printed: the best candidate of the last population, and the controller at the mean of the final search distribution.  The CEM refits
one spread per constant; CMA-ES adapts a 5 x 5 covariance matrix and a step size per greenhouse, so it can follow constants that
interact (the temperature setpoints against the humidity limit, the CO2 setpoint against the lamp hours).

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
    ap.add_argument("--method", choices=("cma", "cem"), default="cma")
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--candidates", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=96, help="env-steps of 15 min (96: one day)")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--elites", type=int, default=0, help="0: half the candidates (CMA-ES), an eighth of them (CEM)")
    ap.add_argument("--init-sigma", type=float, default=0.3)
    ap.add_argument("--scenarios", type=int, default=0, help="crop-noise scenarios per candidate (0: none)")
    ap.add_argument("--dtype", default="float32")
    args = ap.parse_args()

    B, K = args.envs, args.candidates
    starts = [96 * 30 * k for k in range(B)]
    env = TomatoVecEnv(B, weather=synthetic_weather(n_rows=35040), dtype=args.dtype, season_length=10, start_rows=starts,
                       start_days=[s / 96.0 for s in starts], seed=666, auto_reset=False)
    env.reset_tensor()
    base = RuleBasedController()
    for _ in range(4):                                        # a first hour under the default controller
        env.step_tensor(controller=base, want_obs=False)
    scen = dict(n_scenarios=args.scenarios, noise_scale=0.2) if args.scenarios else {}
    search = env.rule_search(K, args.horizon, tune=TUNE, base=base, **scen)
    default_ret = search.rollout(search.theta_of(base))[0][:, 0].cpu().numpy()
    print(f"{B} greenhouses, {args.iters} iterations x {K} candidate controllers x {args.horizon} closed-loop steps"
          + (f" x {args.scenarios} scenarios" if args.scenarios else ""))
    print(f"default controller: return over the horizon {default_ret.mean():.4f} (per greenhouse: {' '.join(f'{v:.3f}' for v in default_ret)})")

    def mean_return(out):
        """The return of the controller at the mean of the search distribution (every candidate of a rollout is that controller)."""
        theta = out["mean"].clamp(-1.0, 1.0).repeat_interleave(K, dim=1)
        return search.rollout(theta)[0][:, 0].cpu().numpy()

    shown = None
    for method in ("cma", "cem"):
        if method == "cma":
            out = search.cma(args.iters, args.elites or None, init_sigma=args.init_sigma, seed=666)
            extra = f"; sigma {' '.join(f'{v:.3f}' for v in out['sigma'].cpu().numpy())}; rows updated in the last generation: " \
                    f"{int((out['status'] == 0).sum())} of {B}"
        else:
            E = args.elites or max(1, K // 8)
            out = search.cem(args.iters, min(E, K), init_std=args.init_sigma, carry=min(2, E), seed=666)
            extra = ""
        best = out["best_return"].cpu().numpy().copy()
        picked = {n: v.cpu().numpy().copy() for n, v in out["best_params"].items()}
        no_adm = int((out["best_k"] < 0).sum())
        at_mean = mean_return(out)
        print(f"{method}: best candidate {best.mean():.4f} (per greenhouse: {' '.join(f'{v:.3f}' for v in best)}); "
              f"mean controller {at_mean.mean():.4f}{extra}")
        if method == args.method:
            shown = (picked, no_adm)
    picked, no_adm = shown
    print(f"tuned by {args.method}:")
    for name in TUNE:
        print(f"  {name:20s} default {getattr(base, name):8.2f}   tuned " + " ".join(f"{v:8.2f}" for v in picked[name]))
        assert all(TUNE[name][0] <= v <= TUNE[name][1] for v in picked[name])
    print(f"greenhouses without an admissible candidate: {no_adm}")
    env.close()


if __name__ == "__main__":
    main()
