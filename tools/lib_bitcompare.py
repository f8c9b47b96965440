#!/usr/bin/env python3
"""Are two builds of libglgym.so bit-identical on the GPU?  (round 6: the policy refactor sc_policy.hpp must not change a bit.)

    GLGYM_LIB=/path/a.so python tools/lib_bitcompare.py dump /tmp/a.npz
    GLGYM_LIB=/path/b.so python tools/lib_bitcompare.py dump /tmp/b.npz
    python tools/lib_bitcompare.py compare /tmp/a.npz /tmp/b.npz

Workloads: the fused step in every kernel layout (fp32 one lane per environment, one- and two-wave builds; fp32 and fp64 four lanes per
environment), actions and verified raw controls, every scheme; glgym_evalF on raw-control-jump tuples (sequential and two-rungs ladder);
small seeded planner workloads through every rollout and every search stage (dump_planning)."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "greenlight-gym2_amd"))


def dump_planning(out, w):
    """Seeded planner workloads, 4 greenhouses x 16 candidates x 6 steps: Planner.cem with scenarios and weather_sigma, RuleSearch.cem and
    .cma, PolicySearch.es and .cem, a constrained Planner.cem.  Kept: everything the search returns, and the children's own returns,
    violations, step counts and flags of its last rollout."""
    import torch
    from gl_gym_amd.planner import Constraints, MLPSpec
    from gl_gym_amd.tomato_env import TomatoVecEnv
    P, K, H = 4, 16, 6
    env = TomatoVecEnv(P, weather=w, dtype="float32", season_length=1, start_rows=[0, 96, 480, 1000], seed=5, auto_reset=False)
    env.reset_tensor()
    g = torch.Generator().manual_seed(11)
    for _ in range(3):
        env.step_tensor((torch.rand(P, 6, generator=g) * 2 - 1).to(env.device), want_obs=True)
    tune = {"temp_setpoint_day": (16.5, 22.5), "temp_setpoint_night": (13.5, 19.5), "co2_day": (400.0, 1200.0), "rh_max": (75.0, 95.0)}
    spec = MLPSpec(env.obs_dim, (8,), scale=0.1)

    def keep(tag, res, plan):
        def walk(prefix, v):
            if isinstance(v, dict):
                for k, x in v.items():
                    walk(f"{prefix}_{k}", x)
            elif hasattr(v, "cpu"):
                out[prefix] = v.cpu().numpy()
        walk(f"plan_{tag}", res)
        for k in ("ret_t", "viol_T", "n_steps_t", "alive_t", "failed_t"):
            out[f"plan_{tag}_child_{k}"] = getattr(plan, k).cpu().numpy()

    scen = dict(n_scenarios=3, noise_scale=0.2, n_tail=2, scenario_seed=4)
    pl = env.planner(K, H, weather_sigma=[20.0, 1.0, 50.0, 10.0, 0.5, 1.0, 0.5], weather_phi=0.6, **scen)
    keep("cem_wscen", pl.cem(2, 4, carry=2, beta=0.5, seed=3), pl)
    out["plan_cem_wscen_window"] = pl.weather_window_t.cpu().numpy()
    rs = env.rule_search(K, H, tune=tune, **scen)
    keep("rule_cem", rs.cem(2, 4, carry=2, seed=3), rs.plan)
    rs = env.rule_search(K, H, tune=tune)
    keep("rule_cma", rs.cma(3, seed=3), rs.plan)
    ps = env.policy_search(K, H, spec, **scen)
    keep("policy_es", ps.es(2, lr=0.05, seed=3), ps.plan)
    ps = env.policy_search(K, H, spec, share="all")
    keep("policy_cem", ps.cem(2, 4, carry=2, seed=3), ps.plan)
    pl = env.planner(K, H, constraints=Constraints(co2=50.0, temp=0.5, rh=2.0), **scen)
    keep("cem_constrained", pl.cem(2, 4, carry=2, seed=3), pl)
    env.close()


def dump(path):
    import torch
    from gl_gym_amd import GreenLight
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    w = synthetic_weather(n_rows=4000)
    w[:, 4] *= 2.5                                  # windy: refined windows, limiter, the odd flag
    out = {}
    starts = list(range(0, 2000, 37))
    for scheme in ("ls5", "rk4", "rk3", "rk2"):
        for tag, dtype, B, layout, occ in (("f32one", "float32", 20480, "one", 1), ("f32occ2", "float32", 20480, "one", 2),
                                           ("f32quad", "float32", 2048, "quad", 0), ("f64quad", "float64", 512, None, 0)):
            env = TomatoVecEnv(B, weather=w, dtype=dtype, scheme=scheme, season_length=1, start_rows=starts, seed=5, auto_reset=False)
            if layout:
                env.set_layout(layout)
            if occ:
                env.set_occupancy(occ)
            env.reset_tensor()
            g = torch.Generator(device=env.device).manual_seed(3)
            for k in range(4):
                env.step_tensor(torch.rand(B, 6, generator=g, device=env.device) * 2 - 1, want_obs=False)
            env.step_tensor(controls_t=torch.rand(B, 6, generator=g, device=env.device, dtype=env.tdtype), want_obs=False)
            out[f"{scheme}_{tag}_x"] = env.x.cpu().numpy()
            out[f"{scheme}_{tag}_flags"] = env.step_flags_t.cpu().numpy()
            out[f"{scheme}_{tag}_reward"] = env.reward_t[:B].cpu().numpy()
            env.close()
    g = np.load(ROOT / "tests" / "golden" / "step_tight_jump.npz")
    X, U, D = g["X"][:96], g["U"][:96], g["D"][:96]
    for dtype in ("float64", "float32"):
        for par in (True, False):
            m = GreenLight(28, 6, 10, 208, 900.0, dtype=dtype, preset="throughput")
            m.set_ladder_parallel(par)
            try:
                out[f"evalF_{dtype}_{int(par)}"] = m.evalF_batch(X, U, D)
            except Exception as e:                   # a failed row raises: record which
                out[f"evalF_{dtype}_{int(par)}"] = np.array([hash(str(e)) % 1000])
            m.close()
    dump_planning(out, w)
    np.savez(path, **out)
    print("dumped", len(out), "arrays to", path)


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = 0
    for k in A.files:
        same = np.array_equal(A[k], B[k], equal_nan=True)
        if not same:
            bad += 1
            d = np.abs(A[k].astype(np.float64) - B[k].astype(np.float64))
            print(f"DIFFERENT {k}: {int((A[k] != B[k]).sum())} of {A[k].size} entries, max |d| {np.nanmax(d):.3e}")
    print(f"{len(A.files)} arrays compared, {bad} differ")
    return bad


if __name__ == "__main__":
    if sys.argv[1] == "dump":
        dump(sys.argv[2])
    else:
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
