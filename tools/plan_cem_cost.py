#!/usr/bin/env python3
"""What the cross-entropy method's stages cost, measured on the GPU -> profiles/plan_cem_cost.txt.

    python tools/plan_cem_cost.py [--parent-pkg DIR] [--out profiles/plan_cem_cost.txt]

fp32, ls5, E = 64, (P, K, H) = (64, 1 024, 48) and (8, 8 192, 48); device events, warmed up, alternating samples.
(a) One CEM iteration end to end (glgym_plan_sample -> fork + rollout -> glgym_plan_elites -> glgym_plan_refit) against Planner.rollout
    alone on the same parent states and on the first sampled block.  The distribution is set back to N(0, init_std) before every timed
    iteration, untimed: an env-step's cost depends on its actions (the sub-stepper refines after large control moves), so both sides
    must step populations of the same distribution.  --parent-pkg DIR: the greenlight-gym2_amd directory of a checkout
    of the PARENT commit with its library built; Planner.rollout then runs in a child process on that build (the block travels through
    a temporary file).  Without it, it runs on this build, the report says so and gives no verdict on (a).  Requirement at (64, 1 024, 48): ratio <= 1.05.
(b) sample + elites + refit against a torch-op restatement of the same three stages (randn, topk, gather, mean / std; beta = 0 on both
    sides) in the same process.  Requirement at (64, 1 024, 48): the HIP median is not above the restatement's median by more than the
    spread (max - min) of the restatement's own samples.
The second shape is recorded without a bar.  No fallback: without a GPU this fails."""
import argparse
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = ((64, 1024, 48), (8, 8192, 48))
E0, ALPHA, MIN_STD, INIT_STD = 64, 0.1, 0.05, 0.5
N_SAMPLES, N_INNER, N_WARM = 7, 5, 2
SEASON = 10


def setup(pkg):
    sys.path.insert(0, str(pkg))
    import torch
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    return torch, TomatoVecEnv, synthetic_weather


def parent_env(torch, TomatoVecEnv, w, P):
    """The P parent environments both sides start from: seeded reset, four seeded steps."""
    env = TomatoVecEnv(P, weather=w, dtype="float32", season_length=SEASON, start_rows=list(range(0, 96 * P, 96)), seed=5, auto_reset=False)
    env.reset_tensor()
    g = torch.Generator().manual_seed(1)
    for _ in range(4):
        env.step_tensor((torch.rand(P, 6, generator=g) * 2 - 1).to(env.device))
    assert (env.scheme, env.n_sub) == ("ls5", 128)
    return env


def timed(torch, fn, n=N_INNER, prepare=None):
    """Device time of fn() in ms, mean of n windows between events; prepare() runs before each window, untimed."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        if prepare:
            prepare()
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / n


def worker(pkg, P, K, H, block_file):
    """Planner.rollout on the build under pkg, on the block in block_file; answers "time" on stdin with one sample."""
    torch, TomatoVecEnv, synthetic_weather = setup(pkg)
    import numpy as np
    env = parent_env(torch, TomatoVecEnv, synthetic_weather(n_rows=35040), P)
    plan = env.planner(K, H)
    block = torch.as_tensor(np.load(block_file), device=env.device).contiguous()
    for _ in range(N_WARM):
        timed(torch, lambda: plan.rollout(block), 1)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "time":
            break
        print(f"ms {timed(torch, lambda: plan.rollout(block)):.6f}", flush=True)


def torch_stages(torch, mean, std, ret, failed, K, E):
    """The same three stages with torch ops (beta = 0): -> the new mean and std."""
    H, P, _ = mean.shape
    a = torch.randn(H, P, K, 6, dtype=torch.float32, device=mean.device)
    a = a.mul_(std[:, :, None]).add_(mean[:, :, None]).clamp_(-1.0, 1.0)
    a[:, :, 0] = mean.clamp(-1.0, 1.0)
    r = torch.where((failed != 0) | ~torch.isfinite(ret), torch.full_like(ret, float("-inf")), ret)
    top = r.topk(E, dim=1).indices
    el = a.gather(2, top[None, :, :, None].expand(H, P, E, 6))
    m, s = el.mean(dim=2), el.std(dim=2, unbiased=False)
    return ALPHA * mean + (1 - ALPHA) * m, (ALPHA * std + (1 - ALPHA) * s).clamp_min(MIN_STD)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", default=None, help="built greenlight-gym2_amd directory of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plan_cem_cost.txt"))
    ap.add_argument("--worker", nargs=5, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker[0]), int(args.worker[1]), int(args.worker[2]), int(args.worker[3]), args.worker[4])
    torch, TomatoVecEnv, synthetic_weather = setup(ROOT / "greenlight-gym2_amd")
    if not torch.cuda.is_available():
        sys.exit("plan_cem_cost.py needs a GPU (no fallback)")
    import numpy as np
    lines = [f"cross-entropy method on the device: cost on {torch.cuda.get_device_name(0)} (tools/plan_cem_cost.py)",
             f"fp32 ls5-128, E = {E0}, alpha = {ALPHA}, min_std = {MIN_STD}, init_std = {INIT_STD}, beta = 0; device events, {N_WARM} warm-up windows, "
             f"{N_SAMPLES} alternating samples of {N_INNER} calls each; spread = (max - min) / median of a side's samples", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731
    w = synthetic_weather(n_rows=35040)
    met = True
    for which, (P, K, H) in enumerate(SHAPES):
        bar = which == 0
        env = parent_env(torch, TomatoVecEnv, w, P)
        plan = env.planner(K, H)
        mean_t = torch.zeros(H, P, 6, dtype=torch.float32, device=env.device)
        std_t = torch.full((H, P, 6), INIT_STD, dtype=torch.float32, device=env.device)
        state = {"draw": 0}

        def iteration():
            block = plan.sample(mean_t, std_t, seed=7, draw_index=state["draw"])
            state["draw"] += 1
            plan.rollout(block)
            plan.elites(E0)
            plan.refit(mean_t, std_t, ALPHA, MIN_STD)

        def reset_dist():
            mean_t.zero_()
            std_t.fill_(INIT_STD)

        first = plan.sample(mean_t, std_t, seed=7, draw_index=0).clone()
        say(f"(P, K, H) = ({P}, {K}, {H}): {P * K} children, action block {first.numel() * 4 / 1e6:.1f} MB")
        # ---- (a) one iteration against the rollout alone ---------------------------------------------------------------------
        with tempfile.TemporaryDirectory() as tmp:
            if args.parent_pkg:
                block_file = str(Path(tmp) / "block.npy")
                np.save(block_file, first.cpu().numpy())
                child = subprocess.Popen([sys.executable, __file__, "--worker", str(Path(args.parent_pkg).resolve()), str(P), str(K), str(H),
                                          block_file], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
                assert child.stdout.readline().strip() == "ready", "the parent-commit worker did not start"

                def rollout_sample():
                    child.stdin.write("time\n")
                    child.stdin.flush()
                    return float(child.stdout.readline().split()[1])
                where = "a child process on the parent commit's build (--parent-pkg)"
            else:
                child, other = None, env.planner(K, H)
                rollout_sample = lambda: timed(torch, lambda: other.rollout(first))  # noqa: E731
                where = "THIS build (no --parent-pkg given; its step kernels are the parent commit's instruction for instruction)"
            for _ in range(N_WARM):
                timed(torch, iteration, 1)
                if not child:
                    rollout_sample()
            it, ro = [], []
            for _ in range(N_SAMPLES):
                it.append(timed(torch, iteration, prepare=reset_dist))     # every population from N(0, init_std), as the rollout's block
                ro.append(rollout_sample())
            if child:
                child.stdin.write("quit\n")
                child.stdin.flush()
                child.wait(timeout=60)
        assert int(plan.n_steps_t.min()) == H and int(plan.failed_t.max()) == 0 and int(plan.n_elite_t.min()) == E0
        m_it, m_ro = statistics.median(it), statistics.median(ro)
        ratio_a = m_it / m_ro
        say(f"  (a) Planner.rollout alone runs in {where}")
        say("      one CEM iteration (sample + fork + rollout + elites + refit), ms: " + " ".join(f"{v:.3f}" for v in it))
        say("      Planner.rollout (fork + rollout), ms                            : " + " ".join(f"{v:.3f}" for v in ro))
        say(f"      medians {m_it:.3f} / {m_ro:.3f} ms; spread of the iteration samples {spread(it) * 100:.1f} %, of the rollout samples "
            f"{spread(ro) * 100:.1f} %")
        say(f"      ratio iteration / rollout = {ratio_a:.4f}" + (f"   (requirement <= 1.05: {'met' if ratio_a <= 1.05 else 'NOT MET'})" if bar and child else ""))
        say(f"      iteration rate {P * K * H / m_it * 1e3:.3e} candidate env-steps/s")
        # ---- (b) the three stages against torch ops ----------------------------------------------------------------------------
        plan.rollout(first)                                  # returns and failure flags of a real population for both sides
        ret, failed = plan.ret_t.view(P, K).clone(), plan.failed_t.view(P, K).clone()

        def hip_stages():                                    # without a rollout in between, elites and refit work on `first`, the
            plan.sample(mean_t, std_t, seed=7, draw_index=state["draw"])     # population of the rollout above: the same work
            state["draw"] += 1
            plan.elites(E0)
            plan.refit(mean_t, std_t, ALPHA, MIN_STD)

        keep = {}

        def th_stages():
            keep["m"], keep["s"] = torch_stages(torch, mean_t, std_t, ret, failed, K, E0)

        for _ in range(N_WARM):
            timed(torch, hip_stages, 1)
            timed(torch, th_stages, 1)
        hip, th = [], []
        for _ in range(N_SAMPLES):
            hip.append(timed(torch, hip_stages, prepare=reset_dist))
            th.append(timed(torch, th_stages, prepare=reset_dist))
        # both sides rank the same returns: the same elite sets (the order inside a tie aside)
        reset_dist()
        hip_stages()
        top = torch.where((failed != 0) | ~torch.isfinite(ret), torch.full_like(ret, float("-inf")), ret).topk(E0, dim=1).indices
        same_sets = bool((plan.elite_k_t[:P * E0].view(P, E0).long().sort(dim=1).values == top.sort(dim=1).values).all())
        m_hip, m_th = statistics.median(hip), statistics.median(th)
        t_s = timed(torch, lambda: plan.sample(mean_t, std_t, seed=7, draw_index=1), 20)
        t_e = timed(torch, lambda: plan.elites(E0), 20)
        t_r = timed(torch, lambda: plan.refit(mean_t, std_t, ALPHA, MIN_STD), 20)
        ok_b = m_hip <= m_th * (1 + spread(th))
        say("  (b) sample + elites + refit, HIP, us        : " + " ".join(f"{v * 1e3:.1f}" for v in hip))
        say("      the same stages with torch ops, us      : " + " ".join(f"{v * 1e3:.1f}" for v in th))
        say(f"      medians {m_hip * 1e3:.1f} / {m_th * 1e3:.1f} us, ratio HIP / torch = {m_hip / m_th:.4f}; spread of the torch samples "
            f"{spread(th) * 100:.1f} %, of the HIP samples {spread(hip) * 100:.1f} %" +
            (f"   (requirement: HIP <= torch x (1 + its spread): {'met' if ok_b else 'NOT MET'})" if bar else ""))
        say(f"      single stages, mean of 20 calls: sample {t_s * 1e3:.1f} us ({first.numel() * 4 / t_s / 1e6:.0f} GB/s written), elites "
            f"{t_e * 1e3:.1f} us ({P * K * K / t_e / 1e6:.1f} G comparisons/s), refit {t_r * 1e3:.1f} us; elite sets equal to torch.topk's: {same_sets}")
        say()
        if bar:
            met = (ratio_a <= 1.05 or not args.parent_pkg) and ok_b
        del plan
        env.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if met else 1


if __name__ == "__main__":
    sys.exit(main())
