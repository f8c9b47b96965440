#!/usr/bin/env python3
"""What rollout collection costs, measured on the GPU -> profiles/collect_cost.txt.

    python tools/collect_cost.py [--parent-pkg DIR] [--out profiles/collect_cost.txt]

fp32, ls5, the wrapper stack of examples/device_rollout.py (TomatoVecEnv -> VecMonitorGPU -> VecNormalizeGPU, 23 observation columns),
65 536 environments, rollouts of 64 steps, tanh nets 23 -> 64 -> 64 -> 6 and 23 -> 64 -> 64 -> 1; device events, warmed up, five
alternating repeats with their spreads, no profiler.
(a) Recorded as a ratio: the stage between two env-steps as the collector runs it (the two nn.Sequential forwards in torch, then
    one glgym_ac_rows launch) against the same stage as the torch ops of examples/device_rollout.py (the same forwards, randn_like,
    the sample, the clamp, the log-probability, four buffer copies).
(b) Recorded as a ratio: glgym_gae at T = 64 against that example's backward torch loop.
(c) Requirement, the collector must not be slower: RolloutCollector.collect() (TorchHeads on the same nets) against the collect() of
    examples/device_rollout.py (restated here op for op) on the parent commit's build, alternated.
(d) Requirement, ratio <= 1.05: a plain step_tensor loop of this build against the parent commit's build.
--parent-pkg DIR: the greenlight-gym2_amd directory of a checkout of the PARENT commit with its library built; the other sides of (c)
and (d) run in child processes on that build.  Without it they run on this build, the report says so and gives no verdict.
No fallback: without a GPU this fails."""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
B0, T0, HIDDEN = 65536, 64, 64
GAMMA, LAM = 0.9631, 0.95
N_SAMPLES, N_WARM = 5, 2


def setup(pkg):
    sys.path.insert(0, str(pkg))
    import torch
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    from gl_gym_amd.vec_monitor import VecMonitorGPU
    from gl_gym_amd.vec_normalize import VecNormalizeGPU
    w = synthetic_weather(n_rows=35040)
    starts = list(range(0, 35040 - 5760 - 60, 96))

    def make(B):
        base = TomatoVecEnv(B, weather=w, dtype="float32", scheme="ls5", season_length=60, start_rows=starts,
                            start_days=[s / 96.0 for s in starts], seed=666)
        return base, VecNormalizeGPU(VecMonitorGPU(base), norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=GAMMA)
    return torch, make


def torch_nets(torch, D, dev):
    torch.manual_seed(0)
    lin, act = torch.nn.Linear, torch.nn.Tanh
    pi = torch.nn.Sequential(lin(D, HIDDEN), act(), lin(HIDDEN, HIDDEN), act(), lin(HIDDEN, 6)).to(dev)
    vf = torch.nn.Sequential(lin(D, HIDDEN), act(), lin(HIDDEN, HIDDEN), act(), lin(HIDDEN, 1)).to(dev)
    return pi, vf, torch.zeros(6, device=dev)


def timed(torch, fn, n=1):
    """Device time of fn() in ms, mean of n windows between events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / n


class TorchRollout:
    """collect() of examples/device_rollout.py, op for op, on an environment stack of its own."""

    def __init__(self, torch, env, B, T, D):
        self.torch, self.env, self.B, self.T = torch, env, B, T
        dev = env.device
        self.pi, self.vf, self.log_std = torch_nets(torch, D, dev)
        e = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
        self.buf = dict(obs=e(T, B, D), act=e(T, B, 6), rew=e(T, B), done=e(T, B), val=e(T, B), logp=e(T, B))
        self.obs = env.reset_tensor()

    def stage(self, t, obs):
        torch, buf, log_std = self.torch, self.buf, self.log_std
        mean, value = self.pi(obs), self.vf(obs).squeeze(-1)
        noise = torch.randn_like(mean)
        act = mean + noise * log_std.exp()
        buf["obs"][t].copy_(obs); buf["act"][t].copy_(act); buf["val"][t].copy_(value)
        buf["logp"][t].copy_((-0.5 * noise.pow(2) - log_std - 0.9189385).sum(-1))
        return act.clamp(-1.0, 1.0)

    def gae(self, last_v):
        torch, buf, B, T = self.torch, self.buf, self.B, self.T
        adv = torch.zeros(B, device=last_v.device)
        advs = torch.empty(T, B, device=last_v.device)
        for t in reversed(range(T)):
            nonterm = 1.0 - buf["done"][t]
            delta = buf["rew"][t] + GAMMA * last_v * nonterm - buf["val"][t]
            adv = delta + GAMMA * LAM * nonterm * adv
            advs[t] = adv; last_v = buf["val"][t]
        return advs

    def collect(self):
        with self.torch.no_grad():
            obs = self.obs
            for t in range(self.T):
                act = self.stage(t, obs)
                obs, rew, done, _ = self.env.step_tensor(act)
                self.buf["rew"][t].copy_(rew); self.buf["done"][t].copy_(done)
            self.obs = obs
            return self.gae(self.vf(obs).squeeze(-1))


def worker(pkg, kind, B, T):
    """The torch collect() ("collect") or a plain step_tensor loop of T steps ("steps") on the build under pkg; answers "time" on stdin
    with one sample."""
    torch, make = setup(pkg)
    base, env = make(B)
    if kind == "collect":
        run = TorchRollout(torch, env, B, T, base.obs_dim).collect
    else:
        run = step_loop(torch, base, B, T)
    for _ in range(N_WARM):
        timed(torch, run)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "time":
            break
        print(f"ms {timed(torch, run):.6f}", flush=True)


def step_loop(torch, base, B, T):
    """T env-steps from a seeded reset under fresh uniform actions at every step: the same work at every sample, on either build."""
    g = torch.Generator().manual_seed(1)
    actions = (torch.rand(T, B, 6, generator=g) * 2 - 1).to(base.device).contiguous()

    def run():
        base.reset_tensor(seed=666)
        for t in range(T):
            base.step_tensor(actions[t])
    return run


class Other:
    """The other side of a comparison: a child process on the parent commit's build, or (without --parent-pkg) this build."""

    def __init__(self, torch, pkg, kind, B, T, local_run):
        self.torch, self.child, self.run = torch, None, local_run
        if pkg:
            self.child = subprocess.Popen([sys.executable, __file__, "--worker", str(Path(pkg).resolve()), kind, str(B), str(T)],
                                          stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            assert self.child.stdout.readline().strip() == "ready", "the parent-commit worker did not start"
        else:
            for _ in range(N_WARM):
                timed(torch, self.run())

    def sample(self):
        if not self.child:
            return timed(self.torch, self.run())
        self.child.stdin.write("time\n")
        self.child.stdin.flush()
        return float(self.child.stdout.readline().split()[1])

    def close(self):
        if self.child:
            self.child.stdin.write("quit\n")
            self.child.stdin.flush()
            self.child.wait(timeout=120)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def alternate(torch, mine, other, n_inner=1):
    for _ in range(N_WARM):
        timed(torch, mine)
    a, b = [], []
    for _ in range(N_SAMPLES):
        a.append(timed(torch, mine, n_inner))
        b.append(other() if callable(other) else other.sample())
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", default=None, help="built greenlight-gym2_amd directory of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "collect_cost.txt"))
    ap.add_argument("--n-envs", type=int, default=B0)
    ap.add_argument("--n-steps", type=int, default=T0)
    ap.add_argument("--worker", nargs=4, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker[0]), args.worker[1], int(args.worker[2]), int(args.worker[3]))
    torch, make = setup(ROOT / "greenlight-gym2_amd")
    if not torch.cuda.is_available():
        sys.exit("collect_cost.py needs a GPU (no fallback)")
    import ctypes as C
    from gl_gym_amd import RolloutCollector, TorchHeads, _lib as L
    B, T = args.n_envs, args.n_steps
    where = ("child processes on the parent commit's build (--parent-pkg)" if args.parent_pkg else
             "THIS build (no --parent-pkg given; its step kernels are the parent commit's instruction for instruction)")
    lines = [f"rollout collection on the device: cost on {torch.cuda.get_device_name(0)} (tools/collect_cost.py)",
             f"fp32 ls5-128, VecNormalizeGPU(VecMonitorGPU(TomatoVecEnv)), {B} environments x {T} steps, tanh nets 23-{HIDDEN}-{HIDDEN}-6 and "
             f"23-{HIDDEN}-{HIDDEN}-1; device events, {N_WARM} warm-up windows, {N_SAMPLES} alternating repeats; spread = (max - min) / median of a "
             f"side's repeats; the other side of (c) and (d) runs in {where}", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731
    fmt = lambda v, k=1.0, d=3: " ".join(f"{x * k:.{d}f}" for x in v)  # noqa: E731
    base, env = make(B)
    dev, D = base.device, base.obs_dim
    base2, env2 = make(B)
    ref = TorchRollout(torch, env2, B, T, D)                     # the torch side of (a) and (b), on a stack of its own
    col = RolloutCollector(env, T, TorchHeads(ref.pi, ref.vf, ref.log_std), gamma=GAMMA, gae_lambda=LAM, seed=0)      # the same nets on both sides
    col.reset(seed=666)
    col.collect()
    ref.collect()

    # ---- (a) the stage on its own --------------------------------------------------------------------------------------------------------
    obs = col.obs_t

    def hip_stage():
        col.policy.heads(obs)
        col.ac_rows(obs, 0, slot=0)

    with torch.no_grad():
        th_stage = lambda: ref.stage(0, obs)  # noqa: E731
        hip_stage()
        col.ac_rows(obs, 0, slot=1, deterministic=True)
        diff = float((col.buffer["actions"][1] - ref.pi(obs)).abs().max())
        for fn in (hip_stage, th_stage):
            timed(torch, fn, 3)
        a, b = alternate(torch, hip_stage, lambda: timed(torch, th_stage, 20), 20)
        only = statistics.median([timed(torch, lambda: col.ac_rows(obs, 0, slot=0), 20) for _ in range(N_SAMPLES)])
    m_a, m_b = statistics.median(a), statistics.median(b)
    say(f"(a) heads in torch + glgym_ac_rows ({B} rows: noise, sample, clip, log-probability, four buffer writes), us : {fmt(a, 1e3, 1)}   median {m_a * 1e3:.1f}")
    say(f"    the same stage as the torch ops of examples/device_rollout.py, us                                   : {fmt(b, 1e3, 1)}   median {m_b * 1e3:.1f}")
    say(f"    spreads {spread(a) * 100:.1f} % / {spread(b) * 100:.1f} %; ratio = {m_a / m_b:.3f}; glgym_ac_rows alone {only * 1e3:.1f} us; largest difference of a mean action {diff:.2e}")
    say()

    # ---- (b) GAE ------------------------------------------------------------------------------------------------------------------------
    buf = col.buffer
    ref.buf["rew"].copy_(buf["rewards"]); ref.buf["done"].copy_(buf["dones"]); ref.buf["val"].copy_(buf["values"])
    hip_gae = lambda: L.check(env._lib.glgym_gae(env._h, C.byref(col._gae), env._stream()), "glgym_gae")  # noqa: E731
    with torch.no_grad():
        th_gae = lambda: ref.gae(buf["last_values"])  # noqa: E731
        hip_gae()
        diff = float((th_gae() - buf["advantages"]).abs().max())
        a, b = alternate(torch, hip_gae, lambda: timed(torch, th_gae, 5), 5)
    m_a, m_b = statistics.median(a), statistics.median(b)
    say(f"(b) glgym_gae (T = {T}, {B} environments), us      : {fmt(a, 1e3, 1)}   median {m_a * 1e3:.1f}")
    say(f"    the backward torch loop of the example, us     : {fmt(b, 1e3, 1)}   median {m_b * 1e3:.1f}")
    say(f"    spreads {spread(a) * 100:.1f} % / {spread(b) * 100:.1f} %; ratio kernel / torch = {m_a / m_b:.3f}; largest difference of an advantage {diff:.2e}")
    say()

    # ---- (c) collect() against the torch collect() on the parent commit's build ---------------------------------------------------------
    other = Other(torch, args.parent_pkg, "collect", B, T, lambda: ref.collect)
    a, b = alternate(torch, col.collect, other)
    other.close()
    m_a, m_b = statistics.median(a), statistics.median(b)
    overlap = max(a) >= min(b) and max(b) >= min(a)
    say(f"(c) RolloutCollector.collect() with TorchHeads ({B} x {T}), ms                  : {fmt(a)}   median {m_a:.3f} = {B * T / m_a * 1e3:.3e} env-steps/s")
    say(f"    collect() of examples/device_rollout.py (torch ops around the same env), ms : {fmt(b)}   median {m_b:.3f} = {B * T / m_b * 1e3:.3e} env-steps/s")
    say(f"    spreads {spread(a) * 100:.1f} % / {spread(b) * 100:.1f} %; ratio collector / torch = {m_a / m_b:.4f}"
        + ("   (the samples of the two sides overlap)" if overlap else "")
        + (f"   (requirement, not slower: {'met' if m_a <= m_b else 'NOT MET'})" if args.parent_pkg else ""))
    r_c = m_a / m_b
    say()

    # ---- (d) the untouched path: a plain step_tensor loop -------------------------------------------------------------------------------
    mine = step_loop(torch, base, B, T)
    other = Other(torch, args.parent_pkg, "steps", B, T, lambda: mine)
    a, b = alternate(torch, mine, other)
    other.close()
    r_d = statistics.median(a) / statistics.median(b)
    say(f"(d) a seeded reset and {T} plain step_tensor calls, this build / the parent commit's, ms: {fmt(a)}  /  {fmt(b)}")
    say(f"    medians {statistics.median(a):.3f} / {statistics.median(b):.3f} ms = {statistics.median(a) / T * 1e3:.1f} / {statistics.median(b) / T * 1e3:.1f} us per "
        f"env-step; spreads {spread(a) * 100:.1f} % / {spread(b) * 100:.1f} %; ratio = {r_d:.4f}"
        + (f"   (requirement <= 1.05: {'met' if r_d <= 1.05 else 'NOT MET'})" if args.parent_pkg else ""))
    base.close()
    base2.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if (not args.parent_pkg or (r_c <= 1.0 and r_d <= 1.05)) else 1


if __name__ == "__main__":
    sys.exit(main())
