#!/usr/bin/env python3
"""What closed-loop neural-policy rollouts cost, measured on the GPU -> profiles/plan_policy_cost.txt.

    python tools/plan_policy_cost.py [--parent-pkg DIR] [--out profiles/plan_policy_cost.txt]

fp32, ls5, pred_horizon = 0 (23 observation columns), (P, K, H) = (64, 1 024, 48): 65 536 children with a policy of their own each;
nets () (linear, 144 parameters) and (32,) (tanh, 966 parameters); device events, warmed up, alternating samples.
(a) Recorded, no requirement: glgym_policy_rows on its own at that shape against the same computation with torch ops -- the per-candidate
    weights gathered from the same theta block, torch.baddbmm per layer, tanh, clamp.
(b) Recorded, no requirement: one PolicySearch.rollout (fork + 48 x (observation, policy, step, accumulate)) against Planner.rollout(actions_t
    = the actions that rollout recorded) of the parent commit's build on the same children.  The closed-loop side pays an observation
    launch and D x 4 bytes of theta per child and step on top of the replay.
(c) Requirement, ratio <= 1.05: Planner.rollout(actions_t = uniform random actions) and RuleSearch.rollout(theta) of this build against
    the parent commit's (their code is unchanged).
The policies of (b) are random draws: their actions keep their sign from step to step, which walks the controls to their bounds -- the
workload on which the step kernels retry most (profiles/r06_saturated_controls_soak.txt).  Both sides of (b) integrate the same actions.
--parent-pkg DIR: the greenlight-gym2_amd directory of a checkout of the PARENT commit with its library built; its rollouts run in child
processes on that build.  Without it they run on this build, the report says so and gives no verdict.
No fallback: without a GPU this fails."""
import argparse
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
P0, K0, H0 = 64, 1024, 48
N_SAMPLES, N_INNER, N_WARM = 7, 3, 2
SEASON = 10
NETS = ((), (32,))
TUNE = {"temp_setpoint_day": (17.0, 23.0), "temp_setpoint_night": (14.0, 19.0), "co2_day": (400.0, 1200.0), "rh_max": (75.0, 95.0),
        "lamps_off": (12.0, 22.0)}                           # examples/tune_rule_based.py


def setup(pkg):
    sys.path.insert(0, str(pkg))
    import torch
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    return torch, TomatoVecEnv, synthetic_weather


def parent_env(torch, TomatoVecEnv, w, P):
    """The P parent environments every side starts from: seeded reset, four steps under the default controller."""
    from gl_gym_amd.baseline import RuleBasedController
    env = TomatoVecEnv(P, weather=w, dtype="float32", season_length=SEASON, pred_horizon=0.0, start_rows=list(range(0, 96 * P, 96)), seed=5,
                       auto_reset=False)
    env.reset_tensor()
    for _ in range(4):
        env.step_tensor(controller=RuleBasedController(), want_obs=True)
    assert (env.scheme, env.n_sub, env.obs_dim) == ("ls5", 128, 23)
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


def worker(pkg, P, K, H, kind, block_file):
    """Planner.rollout(actions_t) (kind "actions") or RuleSearch.rollout(theta) (kind "rule") on the build under pkg; answers "time" on
    stdin with one sample."""
    torch, TomatoVecEnv, synthetic_weather = setup(pkg)
    env = parent_env(torch, TomatoVecEnv, synthetic_weather(n_rows=35040), P)
    block = torch.load(block_file).to(env.device).contiguous()
    if kind == "actions":
        plan = env.planner(K, H)
        run = lambda: plan.rollout(actions_t=block)  # noqa: E731
    else:
        search = env.rule_search(K, H, tune=TUNE)
        plan, run = search.plan, (lambda: search.rollout(block))
    for _ in range(N_WARM):
        timed(torch, run, 1)
    print(f"ready {float(plan.ret_t.sum()):.17g}", flush=True)
    for line in sys.stdin:
        if line.strip() != "time":
            break
        print(f"ms {timed(torch, run):.6f}", flush=True)


class Other:
    """The other side of a comparison: a child process on the parent commit's build, or (without --parent-pkg) this build."""

    def __init__(self, torch, pkg, P, K, H, kind, block, local_run, local_plan):
        self.torch, self.child, self.tmp = torch, None, None
        if pkg:
            self.tmp = tempfile.NamedTemporaryFile(suffix=".pt")
            torch.save(block.cpu(), self.tmp.name)
            self.child = subprocess.Popen([sys.executable, __file__, "--worker", str(Path(pkg).resolve()), str(P), str(K), str(H), kind, self.tmp.name],
                                          stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            ready = self.child.stdout.readline().split()
            assert ready and ready[0] == "ready", "the parent-commit worker did not start"
            self.sum = float(ready[1])
        else:
            self.run = local_run
            for _ in range(N_WARM):
                timed(torch, local_run, 1)
            self.sum = float(local_plan.ret_t.sum())

    def sample(self):
        if not self.child:
            return timed(self.torch, self.run)
        self.child.stdin.write("time\n")
        self.child.stdin.flush()
        return float(self.child.stdout.readline().split()[1])

    def close(self):
        if self.child:
            self.child.stdin.write("quit\n")
            self.child.stdin.flush()
            self.child.wait(timeout=60)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def compare(torch, mine, other):
    for _ in range(N_WARM):
        timed(torch, mine, 1)
    a, b = [], []
    for _ in range(N_SAMPLES):
        a.append(timed(torch, mine))
        b.append(other.sample())
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", default=None, help="built greenlight-gym2_amd directory of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plan_policy_cost.txt"))
    ap.add_argument("--worker", nargs=6, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker[0]), *(int(v) for v in args.worker[1:4]), args.worker[4], args.worker[5])
    torch, TomatoVecEnv, synthetic_weather = setup(ROOT / "greenlight-gym2_amd")
    if not torch.cuda.is_available():
        sys.exit("plan_policy_cost.py needs a GPU (no fallback)")
    import ctypes as C
    import numpy as np
    from gl_gym_amd import _lib as L
    from gl_gym_amd.planner import MLPSpec
    P, K, H = P0, K0, H0
    n = P * K
    where = ("child processes on the parent commit's build (--parent-pkg)" if args.parent_pkg else
             "THIS build (no --parent-pkg given; its step kernels are the parent commit's instruction for instruction)")
    lines = [f"closed-loop neural-policy rollouts on the device: cost on {torch.cuda.get_device_name(0)} (tools/plan_policy_cost.py)",
             f"fp32 ls5-128, pred_horizon 0 (23 observation columns), action steps (verify mode auto: unverified), (P, K, H) = ({P}, {K}, {H}): "
             f"{n} candidate policies = children, share=\"greenhouse\"; device events, {N_WARM} warm-up windows, {N_SAMPLES} alternating samples "
             f"of {N_INNER} calls each; spread = (max - min) / median of a side's samples; the other side of (b) and (c) runs in {where}", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731
    env = parent_env(torch, TomatoVecEnv, synthetic_weather(n_rows=35040), P)
    dev = env.device
    obs0 = env.obs_t.double().cpu().numpy()
    norm = (obs0.mean(axis=0), obs0.var(axis=0) + 1.0, 1e-8, 10.0)
    ok = True
    for hidden in NETS:
        sizes = (23,) + hidden + (6,)
        scale = [v for l in range(len(sizes) - 1) for v in (1.0 / np.sqrt(sizes[l]), 0.5)]
        spec = MLPSpec(23, hidden, activation="tanh", squash="clip", scale=scale, obs_norm=norm)
        ps = env.policy_search(K, H, spec)
        g = torch.Generator().manual_seed(2)
        theta = (torch.rand(ps.Ht, n, 6, generator=g) * 2 - 1).to(dev).contiguous()
        ps.rollout(theta, record=True)
        closed_sum, n_failed = float(ps.plan.ret_t.sum()), int(ps.plan.failed_t.sum())
        assert int(ps.plan.n_steps_t.min()) == H
        actions = ps.actions.contiguous()
        name = f"net {hidden if hidden else '()'}: D = {spec.D} parameters ({spec.D * 4} bytes per child and step), Ht = {spec.Ht}"
        say(name)

        # ---- (a) the policy stage on its own against torch ops ---------------------------------------------------------------------
        obs = ps.obs_t                                            # the children's last observations [n, 23]
        act = torch.zeros(n, 6, dtype=torch.float32, device=dev)
        ra = L.make_plan_args(L.PolicyRowsArgs, n, ps.J, 0, ps.row_mode, ps._net, obs.data_ptr(), theta.data_ptr(), act.data_ptr())

        def hip_rows():
            L.check(env._lib.glgym_policy_rows(env._h, C.byref(ra), env._stream()), "glgym_policy_rows")

        sc_t = torch.as_tensor(spec.scale, device=dev)
        mean_t, inv_t = ps._mean_t, ps._inv_std_t

        def th_rows():
            flat = theta.permute(1, 0, 2).reshape(n, spec.Ht * 6)         # the gather from the block: component i of row j at [j, i]
            a = ((obs - mean_t) * inv_t).clamp_(-spec.clip_obs, spec.clip_obs).unsqueeze(2)
            at = 0
            for l, (o, i) in enumerate(spec.shapes):
                W = flat[:, at:at + o * i].view(n, o, i)
                b = flat[:, at + o * i:at + o * (i + 1)].unsqueeze(2)
                at += o * (i + 1)
                a = torch.baddbmm(b * sc_t[2 * l + 1], W, a, alpha=float(sc_t[2 * l]))
                if l < len(spec.shapes) - 1:
                    a = torch.tanh(a)
            return a.squeeze(2).clamp_(-1, 1)

        hip_rows()
        diff = float((th_rows() - act).abs().max())
        for fn in (hip_rows, th_rows):
            timed(torch, fn, 3)
        rows_t, th_t = [], []
        for _ in range(N_SAMPLES):
            rows_t.append(timed(torch, hip_rows, 20))
            th_t.append(timed(torch, th_rows, 20))
        m_rows, m_th = statistics.median(rows_t), statistics.median(th_t)
        say(f"  (a) glgym_policy_rows ({n} rows, weights of their own), us per step : " + " ".join(f"{v * 1e3:.1f}" for v in rows_t)
            + f"   median {m_rows * 1e3:.1f} us = {spec.D * 4 * n / (m_rows * 1e-3) / 1e12:.2f} TB/s of theta")
        say("      the same with torch ops (gather, baddbmm, tanh, clamp), us per step   : " + " ".join(f"{v * 1e3:.1f}" for v in th_t)
            + f"   median {m_th * 1e3:.1f} us; largest difference of an action {diff:.2e}")
        say(f"      ratio kernel / torch = {m_rows / m_th:.3f}" + ("   (the kernel is SLOWER than its torch restatement)" if m_rows > m_th else ""))

        # ---- (b) the closed-loop rollout against the parent commit's open-loop replay of its actions --------------------------------
        local = env.planner(K, H)
        other = Other(torch, args.parent_pkg, P, K, H, "actions", actions, lambda: local.rollout(actions_t=actions), local)
        cl, op = compare(torch, lambda: ps.rollout(theta), other)
        other.close()
        m_cl, m_op = statistics.median(cl), statistics.median(op)
        say(f"  (b) random policies: {float((ps.plan.u.float() <= 0).float().mean() + (ps.plan.u.float() >= 1).float().mean()) * 100:.0f} % of the "
            f"children's controls end the rollout on a bound")
        say(f"      sum of the {n} returns: closed loop {closed_sum:.17g}, open-loop replay {other.sum:.17g} "
            f"({'equal' if closed_sum == other.sum else 'DIFFERENT'}); {n_failed} children failed")
        say("      closed-loop rollout (fork + 48 x (observation, policy, step, accumulate)), ms : " + " ".join(f"{v:.3f}" for v in cl))
        say("      open-loop rollout of the recorded actions (fork + 48 x (step, accumulate)), ms: " + " ".join(f"{v:.3f}" for v in op))
        say(f"      medians {m_cl:.3f} / {m_op:.3f} ms; spreads {spread(cl) * 100:.1f} % / {spread(op) * 100:.1f} %; ratio = {m_cl / m_op:.4f} "
            f"(recorded, no requirement); the policy stage is {m_rows * H / m_cl * 100:.2f} % of the closed-loop rollout over its {H} steps")
        say()

    # ---- (c) the existing rollouts against the parent commit's: requirement <= 1.05 ----------------------------------------------------
    plan = env.planner(K, H)
    g = torch.Generator().manual_seed(3)
    fresh = (torch.rand(H, n, 6, generator=g) * 2 - 1).to(dev).contiguous()      # the planner's usual population: fresh actions at every step
    other = Other(torch, args.parent_pkg, P, K, H, "actions", fresh, lambda: plan.rollout(actions_t=fresh), plan)
    a, b = compare(torch, lambda: plan.rollout(actions_t=fresh), other)
    other.close()
    r_plan = statistics.median(a) / statistics.median(b)
    say("(c) Planner.rollout(actions_t = uniform random actions), this build / the parent commit's, ms: " + " ".join(f"{v:.3f}" for v in a) + "  /  " + " ".join(f"{v:.3f}" for v in b))
    say(f"      medians {statistics.median(a):.3f} / {statistics.median(b):.3f} ms; spreads {spread(a) * 100:.1f} % / {spread(b) * 100:.1f} %; "
        f"ratio = {r_plan:.4f}" + (f"   (requirement <= 1.05: {'met' if r_plan <= 1.05 else 'NOT MET'})" if args.parent_pkg else ""))
    search = env.rule_search(K, H, tune=TUNE)
    g = torch.Generator().manual_seed(2)
    rtheta = (0.3 * torch.randn(search.Ht, n, 6, generator=g)).clamp_(-1, 1).to(dev).contiguous()
    local = env.rule_search(K, H, tune=TUNE)
    other = Other(torch, args.parent_pkg, P, K, H, "rule", rtheta, lambda: local.rollout(rtheta), local.plan)
    a, b = compare(torch, lambda: search.rollout(rtheta), other)
    other.close()
    r_rule = statistics.median(a) / statistics.median(b)
    say("    RuleSearch.rollout(theta), this build / the parent commit's, ms  : " + " ".join(f"{v:.3f}" for v in a) + "  /  " + " ".join(f"{v:.3f}" for v in b))
    say(f"      medians {statistics.median(a):.3f} / {statistics.median(b):.3f} ms; spreads {spread(a) * 100:.1f} % / {spread(b) * 100:.1f} %; "
        f"ratio = {r_rule:.4f}" + (f"   (requirement <= 1.05: {'met' if r_rule <= 1.05 else 'NOT MET'})" if args.parent_pkg else ""))
    say()
    ok = r_plan <= 1.05 and r_rule <= 1.05
    env.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if (ok or not args.parent_pkg) else 1


if __name__ == "__main__":
    sys.exit(main())
