#!/usr/bin/env python3
"""What constrained ranking costs, measured on the GPU -> profiles/plan_constrain_cost.txt.

    python tools/plan_constrain_cost.py [--parent-pkg DIR] [--out profiles/plan_constrain_cost.txt]

Device events, warmed up, alternating samples; spread = (max - min) / median of a side's samples.
(a) glgym_plan_constrain on its own (both kernels, every optional output) at (P, O, K, S) = (64, 1, 1024, 1), (64, 1, 128, 8) and
    (1, 64, 8192, 1) -- share="all" over 64 greenhouses -- on seeded violations with budgets at their median, per step,
    feasibility-first; beside it the same computation written with torch ops in the same process, and the ratio, whichever way it falls.
(b) Planner.cem, RuleSearch.cem and PolicySearch.cem WITHOUT constraints on this build against the parent commit's build on the same inputs: the paths the
    stage must leave alone.  --parent-pkg DIR: the greenlight-gym2_amd directory of a checkout of the PARENT commit with its library
    built; both sides then run in child processes of their own.  Without it the report says so and gives no verdict.
    Requirement: ratio <= 1.05.
No fallback: without a GPU this fails."""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(64, 1, 1024, 1), (64, 1, 128, 8), (1, 64, 8192, 1)]
N_SAMPLES, N_INNER, N_WARM = 7, 20, 2
CEM_P, CEM_K, CEM_H, CEM_ITERS, CEM_ELITES, CEM_INNER = 64, 128, 24, 2, 16, 3
TUNE = {"temp_setpoint_day": (16.5, 22.5), "temp_setpoint_night": (13.5, 19.5), "co2_day": (400.0, 1200.0), "rh_max": (75.0, 95.0)}


def timed(torch, fn, n):
    """Device time of fn() in ms, mean of n windows between events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / n


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def worker(pkg):
    """Planner.cem, RuleSearch.cem and PolicySearch.cem without constraints on the build under pkg; answers "planner" / "rule" / "policy"
    on stdin with one sample."""
    sys.path.insert(0, str(pkg))
    import torch
    from gl_gym_amd.planner import MLPSpec
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    env = TomatoVecEnv(CEM_P, weather=synthetic_weather(n_rows=35040), dtype="float32", season_length=10,
                       start_rows=list(range(0, 96 * CEM_P, 96)), seed=5, auto_reset=False)
    env.reset_tensor()
    g = torch.Generator().manual_seed(1)
    for _ in range(4):
        env.step_tensor((torch.rand(CEM_P, 6, generator=g) * 2 - 1).to(env.device))
    plan, rule = env.planner(CEM_K, CEM_H), env.rule_search(CEM_K, CEM_H, tune=TUNE)
    policy = env.policy_search(CEM_K, CEM_H, MLPSpec(env.obs_dim, (16,), scale=0.1))
    calls = {"planner": lambda: plan.cem(CEM_ITERS, CEM_ELITES, carry=4, beta=0.5, seed=3), "rule": lambda: rule.cem(CEM_ITERS, CEM_ELITES, carry=4, seed=3),
             "policy": lambda: policy.cem(CEM_ITERS, CEM_ELITES, carry=4, seed=3)}
    for fn in calls.values():
        for _ in range(N_WARM):
            timed(torch, fn, 1)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() not in calls:
            break
        print(f"ms {timed(torch, calls[line.strip()], CEM_INNER):.6f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", default=None, help="built greenlight-gym2_amd directory of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plan_constrain_cost.txt"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker))
    sys.path.insert(0, str(ROOT / "greenlight-gym2_amd"))
    import ctypes as C
    import torch
    if not torch.cuda.is_available():
        sys.exit("plan_constrain_cost.py needs a GPU (no fallback)")
    from gl_gym_amd import _lib as L
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    env = TomatoVecEnv(2, weather=synthetic_weather(n_rows=2000), dtype="float32", season_length=1, start_rows=[0], seed=5,
                       auto_reset=False)                             # for its handle and stream only
    dev, lib, h, st = env.device, env._lib, env._h, env._stream
    lines = [f"constrained ranking on the device: cost on {torch.cuda.get_device_name(0)} (tools/plan_constrain_cost.py)",
             f"device events, {N_WARM} warm-up windows, {N_SAMPLES} alternating samples; spread = (max - min) / median of a side's samples", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731
    inf = float("inf")

    # ---- (a) the stage on its own, against torch ops ------------------------------------------------------------------------------
    say(f"(a) glgym_plan_constrain (per step, feasibility-first, n_allow 0, every optional output) against the same computation with torch "
        f"ops; samples of {N_INNER} calls, us")
    for P, O, K, S in SHAPES:
        J, R, n = P * K, O * S, P * O * K * S
        ld = (n + 63) // 64 * 64
        g = torch.Generator().manual_seed(P + K)
        level = torch.rand(P, 1, K, 1, generator=g, dtype=torch.float64) + 0.5
        n_steps = torch.randint(1, 49, (P, O, K, S), generator=g, dtype=torch.int32)
        viol = torch.zeros(3, ld, dtype=torch.float64)
        for i, scale in enumerate((40.0, 0.7, 3.0)):
            viol[i, :n] = (scale * level * (1 + 0.05 * torch.rand(P, O, K, S, generator=g, dtype=torch.float64)) * n_steps).reshape(-1)
        budget = [float((viol[i, :n] / n_steps.reshape(-1)).median()) for i in range(3)]
        ret = torch.randn(J, generator=g, dtype=torch.float64) * 100
        viol, n_steps, ret = viol.to(dev), n_steps.reshape(-1).to(dev), ret.to(dev)
        failed = torch.zeros(J, dtype=torch.uint8, device=dev)
        score, excess = torch.zeros(J, dtype=torch.float64, device=dev), torch.zeros(J, dtype=torch.float64, device=dev)
        failed_out, feasible = torch.zeros(J, dtype=torch.uint8, device=dev), torch.zeros(J, dtype=torch.uint8, device=dev)
        n_viol, n_feasible = torch.zeros(J, dtype=torch.int32, device=dev), torch.zeros(P, dtype=torch.int32, device=dev)
        a = L.make_plan_args(L.PlanConstrainArgs, P, O, K, S, ld, 1, 0, L.CONSTRAIN_MODES["feasible_first"], (C.c_double * 3)(*budget),
                             (C.c_double * 3)(1.0, 1.0, 1.0), 0.0, ret.data_ptr(), failed.data_ptr(), viol.data_ptr(), n_steps.data_ptr(),
                             score.data_ptr(), failed_out.data_ptr(), feasible.data_ptr(), excess.data_ptr(), n_viol.data_ptr(),
                             n_feasible.data_ptr())
        b_t = torch.tensor(budget, dtype=torch.float64, device=dev).view(3, 1, 1, 1, 1)
        keep = {}

        def hip():
            L.check(lib.glgym_plan_constrain(h, C.byref(a), st()), "glgym_plan_constrain")

        def th():
            d = n_steps.view(P, O, K, S).clamp(min=1).double()
            e = (viol[:, :n].view(3, P, O, K, S) / d - b_t).clamp(min=0.0)
            gr = e.sum(dim=0).permute(0, 2, 1, 3).reshape(J, R)
            feas = (gr > 0).sum(dim=1) <= 0
            G = gr.mean(dim=1)
            adm = (failed == 0) & torch.isfinite(ret)
            low = torch.where(adm & feas, ret, torch.full_like(ret, inf)).view(P, K).amin(dim=1)
            floor = torch.where(torch.isinf(low), torch.zeros_like(low), low) - 1.0
            sc = torch.where(feas, ret, floor.repeat_interleave(K) - G)
            keep["score"] = torch.where(adm, sc, torch.full_like(sc, float("nan")))
            keep["n_feasible"] = (adm & feas).view(P, K).sum(dim=1)

        for _ in range(N_WARM):
            timed(torch, hip, 3)
            timed(torch, th, 3)
        t_hip, t_th = [], []
        for _ in range(N_SAMPLES):
            t_hip.append(timed(torch, hip, N_INNER))
            t_th.append(timed(torch, th, N_INNER))
        err = float((keep["score"] - score).abs().max())
        n_f = int(n_feasible.sum())
        assert 0 < n_f < J and int((keep["n_feasible"] - n_feasible).abs().max()) == 0
        m_hip, m_th = statistics.median(t_hip), statistics.median(t_th)
        say(f"    (P, O, K, S) = ({P}, {O}, {K}, {S}): {J} candidates x {R} runs, {n_f} feasible")
        say("      HIP  : " + " ".join(f"{v * 1e3:.1f}" for v in t_hip))
        say("      torch: " + " ".join(f"{v * 1e3:.1f}" for v in t_th))
        say(f"      medians {m_hip * 1e3:.1f} / {m_th * 1e3:.1f} us, ratio HIP / torch = {m_hip / m_th:.4f}; spread HIP {spread(t_hip) * 100:.1f} %, "
            f"torch {spread(t_th) * 100:.1f} %; {n * 28 / m_hip / 1e6:.1f} GB/s of violations and step counts read; max |score - torch's| = {err:.2e}")
    say()
    env.close()

    # ---- (b) the untouched paths against the parent commit's build ------------------------------------------------------------------
    pkgs = [ROOT / "greenlight-gym2_amd", Path(args.parent_pkg).resolve() if args.parent_pkg else ROOT / "greenlight-gym2_amd"]
    kids = [subprocess.Popen([sys.executable, __file__, "--worker", str(p)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True) for p in pkgs]
    for k in kids:
        assert k.stdout.readline().strip() == "ready", "a worker did not start"

    def sample(k, what):
        k.stdin.write(what + "\n")
        k.stdin.flush()
        return float(k.stdout.readline().split()[1])

    where = "the parent commit's build (--parent-pkg)" if args.parent_pkg else "THIS build again (no --parent-pkg given: no verdict)"
    say(f"(b) constraints=None on this build against {where}, each in a child process; fp32 ls5, {CEM_P} greenhouses x {CEM_K} candidates x "
        f"{CEM_H} steps, cem(n_iter={CEM_ITERS}, n_elite={CEM_ELITES}, carry=4); samples of {CEM_INNER} calls, ms")
    ok = True
    for what, name in (("planner", "Planner.cem"), ("rule", "RuleSearch.cem"), ("policy", "PolicySearch.cem")):
        new, old = [], []
        for _ in range(N_SAMPLES):
            new.append(sample(kids[0], what))
            old.append(sample(kids[1], what))
        ratio = statistics.median(new) / statistics.median(old)
        ok = ok and ratio <= 1.05
        say(f"    {name}: this build " + " ".join(f"{v:.3f}" for v in new))
        say(f"    {' ' * len(name)}  parent     " + " ".join(f"{v:.3f}" for v in old))
        say(f"      medians {statistics.median(new):.3f} / {statistics.median(old):.3f} ms, ratio = {ratio:.4f}; spread this build "
            f"{spread(new) * 100:.1f} %, parent {spread(old) * 100:.1f} %" + (f"   (requirement <= 1.05: {'met' if ratio <= 1.05 else 'NOT MET'})" if args.parent_pkg else ""))
    for k in kids:
        k.stdin.write("quit\n")
        k.stdin.flush()
        k.wait(timeout=60)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if (ok or not args.parent_pkg) else 1


if __name__ == "__main__":
    sys.exit(main())
