#!/usr/bin/env python3
"""What robust planning's two stages cost, measured on the GPU -> profiles/plan_scen_cost.txt.

    python tools/plan_scen_cost.py [--parent-pkg DIR] [--out profiles/plan_scen_cost.txt]

fp32, ls5, (P, K, S, H) = (64, 128, 8, 48): 65 536 children; device events, warmed up, alternating samples.
(a) glgym_plan_scenario (one step's prologue: crop blocks and the expanded action plane) and glgym_plan_aggregate on their own.
(b) One Planner.rollout in scenario mode (fork + H x (prologue, env-step, accumulate) + aggregate) against Planner.rollout of the parent
    commit's build on the same 65 536 children with crop="current": 1 024 candidates per greenhouse, each candidate's sequence repeated
    S times -- the same CROP build of the step kernel on a held block, no prologue.  --parent-pkg DIR: the greenlight-gym2_amd directory
    of a checkout of the PARENT commit with its library built; its rollout runs in a child process on that build (the block travels
    through a temporary file).  Without it, it runs on this build, the report says so and gives no verdict.  Requirement: ratio <= 1.05.
(c) The two stages against the same work written with torch ops in the same process: rand + broadcast multiply + repeat_interleave
    for the prologue, sort + cumsum + mean for the aggregate.  Requirement as for the CEM stages: the HIP median is not above the
    restatement's median by more than the spread (max - min) of the restatement's own samples.
No fallback: without a GPU this fails."""
import argparse
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
P0, K0, S0, H0, TAIL, SCALE = 64, 128, 8, 48, 4, 0.2
N_SAMPLES, N_INNER, N_WARM = 7, 5, 2
SEASON = 10


def setup(pkg):
    sys.path.insert(0, str(pkg))
    import torch
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    return torch, TomatoVecEnv, synthetic_weather


def parent_env(torch, TomatoVecEnv, w, P):
    """The P noisy parent environments both sides start from: seeded reset, four seeded steps (crop_T then holds the last draw)."""
    env = TomatoVecEnv(P, weather=w, dtype="float32", season_length=SEASON, start_rows=list(range(0, 96 * P, 96)), seed=5, auto_reset=False,
                       uncertainty_scale=SCALE)
    env.reset_tensor()
    g = torch.Generator().manual_seed(1)
    for _ in range(4):
        env.step_tensor((torch.rand(P, 6, generator=g) * 2 - 1).to(env.device))
    assert (env.scheme, env.n_sub) == ("ls5", 128)
    return env


def timed(torch, fn, n=N_INNER):
    """Device time of fn() in ms, mean of n windows between events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / n


def worker(pkg, P, K, H, block_file):
    """Planner.rollout(crop="current") on the build under pkg, on the block in block_file; answers "time" on stdin with one sample."""
    torch, TomatoVecEnv, synthetic_weather = setup(pkg)
    import numpy as np
    env = parent_env(torch, TomatoVecEnv, synthetic_weather(n_rows=35040), P)
    plan = env.planner(K, H, crop="current")
    block = torch.as_tensor(np.load(block_file), device=env.device).contiguous()
    for _ in range(N_WARM):
        timed(torch, lambda: plan.rollout(block), 1)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "time":
            break
        print(f"ms {timed(torch, lambda: plan.rollout(block)):.6f}", flush=True)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", default=None, help="built greenlight-gym2_amd directory of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plan_scen_cost.txt"))
    ap.add_argument("--worker", nargs=5, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker[0]), int(args.worker[1]), int(args.worker[2]), int(args.worker[3]), args.worker[4])
    torch, TomatoVecEnv, synthetic_weather = setup(ROOT / "greenlight-gym2_amd")
    if not torch.cuda.is_available():
        sys.exit("plan_scen_cost.py needs a GPU (no fallback)")
    import ctypes as C
    import numpy as np
    from gl_gym_amd import _lib as L
    P, K, S, H = P0, K0, S0, H0
    J, n = P * K, P * K * S
    lines = [f"robust planning on the device: cost on {torch.cuda.get_device_name(0)} (tools/plan_scen_cost.py)",
             f"fp32 ls5-128, (P, K, S, H) = ({P}, {K}, {S}, {H}): {J} candidates, {n} children; noise=\"step\", scale {SCALE}, n_tail {TAIL}; device "
             f"events, {N_WARM} warm-up windows, {N_SAMPLES} alternating samples of {N_INNER} calls each; spread = (max - min) / median of a side's "
             "samples", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731
    env = parent_env(torch, TomatoVecEnv, synthetic_weather(n_rows=35040), P)
    dev = env.device
    plan = env.planner(K, H, n_scenarios=S, n_tail=TAIL, scenario_seed=7)
    cand = (torch.rand(H, J, 6, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(dev).contiguous()
    lib, h, st = env._lib, env._h, env._stream

    # ---- (a) the two stages on their own ---------------------------------------------------------------------------------------
    plan.rollout(cand)                                           # real returns, flags, violations and step counts for the aggregate
    assert int(plan.n_steps_t.min()) == H and int(plan.failed_t.max()) == 0
    sc = L.make_plan_args(L.PlanScenarioArgs, P, K, S, plan.ld, 1, 0, SCALE, 7, 0, plan.scenario_base_t.data_ptr(), plan.crop_T.data_ptr(),
                          cand[1].data_ptr(), plan.stage_t.data_ptr())
    ag = L.make_plan_args(L.PlanAggregateArgs, J, S, TAIL, plan.ld, plan.ld_cand, plan.ret_t.data_ptr(), plan.failed_t.data_ptr(),
                          plan.viol_T.data_ptr(), plan.n_steps_t.data_ptr(), plan.ret_cand_t.data_ptr(), plan.failed_cand_t.data_ptr(),
                          plan.viol_cand_T.data_ptr(), plan.steps_cand_t.data_ptr())

    def hip_prologue():
        L.check(lib.glgym_plan_scenario(h, C.byref(sc), st()), "glgym_plan_scenario")

    def hip_aggregate():
        L.check(lib.glgym_plan_aggregate(h, C.byref(ag), st()), "glgym_plan_aggregate")

    for fn in (hip_prologue, hip_aggregate):
        timed(torch, fn, 3)
    t_p, t_a = timed(torch, hip_prologue, 20), timed(torch, hip_aggregate, 20)
    wr = n * (34 + 6) * 4
    say("(a) single stages, mean of 20 calls")
    say(f"      glgym_plan_scenario (one step: {n} crop blocks + the expanded action plane): {t_p * 1e3:.1f} us ({wr / t_p / 1e6:.0f} GB/s written)")
    say(f"      glgym_plan_aggregate ({J} candidates x {S} scenarios): {t_a * 1e3:.1f} us")
    say(f"      per rollout: {H} prologues + 1 aggregate = {(H * t_p + t_a) * 1e3:.1f} us")
    say()

    # ---- (b) a scenario rollout against the parent commit's held-block rollout --------------------------------------------------
    with tempfile.TemporaryDirectory() as tmp:
        if args.parent_pkg:
            block_file = str(Path(tmp) / "block.npy")
            np.save(block_file, cand.repeat_interleave(S, dim=1).cpu().numpy())
            child = subprocess.Popen([sys.executable, __file__, "--worker", str(Path(args.parent_pkg).resolve()), str(P), str(K * S), str(H),
                                      block_file], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            assert child.stdout.readline().strip() == "ready", "the parent-commit worker did not start"

            def held_sample():
                child.stdin.write("time\n")
                child.stdin.flush()
                return float(child.stdout.readline().split()[1])
            where = "a child process on the parent commit's build (--parent-pkg)"
        else:
            child, other, wide = None, env.planner(K * S, H, crop="current"), cand.repeat_interleave(S, dim=1).contiguous()
            held_sample = lambda: timed(torch, lambda: other.rollout(wide))  # noqa: E731
            where = "THIS build (no --parent-pkg given; its step kernels are the parent commit's instruction for instruction)"
        for _ in range(N_WARM):
            timed(torch, lambda: plan.rollout(cand), 1)
            if not child:
                held_sample()
        sn, hd = [], []
        for _ in range(N_SAMPLES):
            sn.append(timed(torch, lambda: plan.rollout(cand)))
            hd.append(held_sample())
        if child:
            child.stdin.write("quit\n")
            child.stdin.flush()
            child.wait(timeout=60)
    assert int(plan.n_steps_t.min()) == H and int(plan.failed_t.max()) == 0 and int(plan.failed_cand_t.max()) == 0
    m_sn, m_hd = statistics.median(sn), statistics.median(hd)
    ratio_b = m_sn / m_hd
    say(f"(b) Planner.rollout(crop=\"current\") on the same {n} children runs in {where}")
    say("      scenario rollout (fork + 48 x (prologue, step, accumulate) + aggregate), ms: " + " ".join(f"{v:.3f}" for v in sn))
    say("      held-block rollout (fork + 48 x (step, accumulate)), ms                    : " + " ".join(f"{v:.3f}" for v in hd))
    say(f"      medians {m_sn:.3f} / {m_hd:.3f} ms; spread of the scenario samples {spread(sn) * 100:.1f} %, of the held-block samples "
        f"{spread(hd) * 100:.1f} %")
    say(f"      ratio scenario / held-block = {ratio_b:.4f}" + (f"   (requirement <= 1.05: {'met' if ratio_b <= 1.05 else 'NOT MET'})" if child else ""))
    say(f"      scenario rollout rate {n * H / m_sn * 1e3:.3e} scenario env-steps/s")
    say()

    # ---- (c) the two stages against torch ops -------------------------------------------------------------------------------------
    p0 = torch.as_tensor(np.asarray(env.p, dtype=np.float64)[128:162].astype(np.float32), device=dev)
    crop_th, stage_th = torch.zeros_like(plan.crop_T), torch.zeros_like(plan.stage_t)
    keep = {}

    def th_prologue():
        z = (torch.rand(P * S, 34, dtype=torch.float32, device=dev) - 0.5) * SCALE
        v = p0 + z * p0
        v[:, 16] = v[:, 13] / v[:, 14]
        crop_th[:, :n].view(34, P, K, S).copy_(v.view(P, 1, S, 34).permute(3, 0, 1, 2).expand(34, P, K, S))
        stage_th.copy_(cand[1].repeat_interleave(S, dim=0))

    def th_aggregate():
        r = plan.ret_t.view(J, S)
        bad = ((plan.failed_t.view(J, S) != 0) | ~torch.isfinite(r)).any(dim=1)
        tail = r.sort(dim=1).values.cumsum(dim=1)[:, TAIL - 1] / TAIL
        keep["ret"] = torch.where(bad, torch.full_like(tail, float("nan")), tail)
        keep["viol"] = plan.viol_T[:, :n].view(3, J, S).mean(dim=2)
        keep["steps"] = plan.n_steps_t.view(J, S).amin(dim=1)

    def hip_stages():
        hip_prologue()
        hip_aggregate()

    def th_stages():
        th_prologue()
        th_aggregate()

    for _ in range(N_WARM):
        timed(torch, hip_stages, 1)
        timed(torch, th_stages, 1)
    hip, th = [], []
    for _ in range(N_SAMPLES):
        hip.append(timed(torch, hip_stages))
        th.append(timed(torch, th_stages))
    err = float((keep["ret"] - plan.ret_cand_t).abs().max())      # both sides score the same returns (summation order aside)
    m_hip, m_th = statistics.median(hip), statistics.median(th)
    t_tp, t_ta = timed(torch, th_prologue, 20), timed(torch, th_aggregate, 20)
    ok_c = m_hip <= m_th * (1 + spread(th))
    say("(c) prologue + aggregate, HIP, us            : " + " ".join(f"{v * 1e3:.1f}" for v in hip))
    say("      the same stages with torch ops, us     : " + " ".join(f"{v * 1e3:.1f}" for v in th))
    say(f"      medians {m_hip * 1e3:.1f} / {m_th * 1e3:.1f} us, ratio HIP / torch = {m_hip / m_th:.4f}; spread of the torch samples "
        f"{spread(th) * 100:.1f} %, of the HIP samples {spread(hip) * 100:.1f} %   (requirement: HIP <= torch x (1 + its spread): "
        f"{'met' if ok_c else 'NOT MET'})")
    say(f"      torch single stages, mean of 20 calls: prologue {t_tp * 1e3:.1f} us, aggregate {t_ta * 1e3:.1f} us; max |score - torch's| = {err:.2e}")
    say()
    env.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if ((ratio_b <= 1.05 or not args.parent_pkg) and ok_c) else 1


if __name__ == "__main__":
    sys.exit(main())
