#!/usr/bin/env python3
"""Rollout collection through the library's collector, then three PPO iterations in torch: the stack and the nets of
examples/device_rollout.py (TomatoVecEnv -> VecMonitorGPU -> VecNormalizeGPU, tanh nets of width 64).  The heads are the torch modules
the optimiser trains (gl_gym_amd.collector.TorchHeads); everything behind them -- the seeded action noise, the sample, the clip, the
log-probability, the buffer writes -- is one glgym_ac_rows launch per step, and GAE one glgym_gae launch per rollout
(RolloutCollector).  A clipped-surrogate PPO epoch with Adam follows each rollout; the next rollout reads the updated modules.

    python examples/collect_rollouts.py --n-envs 65536 --n-steps 64

Prints the collection rate and, for the first minibatch of every iteration, max |ratio - 1|: torch re-evaluates the log-probabilities
the kernel wrote, so before the optimiser step the ratio is 1 up to float32 rounding (recorded, no bar).
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "greenlight-gym2_amd"))

import torch  # noqa: E402

from gl_gym_amd import RolloutCollector, TorchHeads  # noqa: E402
from gl_gym_amd.tomato_env import TomatoVecEnv  # noqa: E402
from gl_gym_amd.utils import synthetic_weather  # noqa: E402
from gl_gym_amd.vec_monitor import VecMonitorGPU  # noqa: E402
from gl_gym_amd.vec_normalize import VecNormalizeGPU  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=65536)
    ap.add_argument("--n-steps", type=int, default=64, help="rollout length per env (PPO n_steps)")
    ap.add_argument("--scheme", default="ls5", choices=["ls5", "rk4", "rk3", "rk2"])
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--minibatches", type=int, default=4)
    args = ap.parse_args()

    w = synthetic_weather(n_rows=35040)
    starts = list(range(0, 35040 - 5760 - 60, 96))
    base = TomatoVecEnv(args.n_envs, weather=w, dtype="float32", scheme=args.scheme, season_length=60, start_rows=starts,
                        start_days=[s / 96.0 for s in starts], seed=666)
    gamma, lam, clip = 0.9631, 0.95, 0.2
    env = VecNormalizeGPU(VecMonitorGPU(base), norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=gamma)
    B, T, D = args.n_envs, args.n_steps, base.obs_dim

    torch.manual_seed(0)
    dev, H = base.device, args.hidden
    pi = torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.Tanh(), torch.nn.Linear(H, H), torch.nn.Tanh(), torch.nn.Linear(H, 6)).to(dev)
    vf = torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.Tanh(), torch.nn.Linear(H, 1)).to(dev)
    log_std = torch.nn.Parameter(torch.zeros(6, device=dev))
    col = RolloutCollector(env, T, TorchHeads(pi, vf, log_std), gamma=gamma, gae_lambda=lam, seed=0)
    col.reset(seed=666)
    opt = torch.optim.Adam(list(pi.parameters()) + list(vf.parameters()) + [log_std], lr=3e-4)

    col.collect()                                        # warm-up (kernel code objects)
    torch.cuda.synchronize()
    for it in range(args.iterations):
        t0 = time.perf_counter()
        buf = col.collect()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        obs, act = buf["observations"].reshape(T * B, D), buf["actions"].reshape(T * B, 6)
        old_logp, adv, ret = buf["log_probs"].reshape(-1), buf["advantages"].reshape(-1), buf["returns"].reshape(-1)
        worst, losses = 0.0, []
        for mb, idx in enumerate(torch.randperm(T * B, device=obs.device).chunk(args.minibatches)):
            mean, value = pi(obs[idx]), vf(obs[idx]).squeeze(-1)
            noise = (act[idx] - mean) / log_std.exp()
            logp = (-0.5 * noise.pow(2) - log_std - 0.9189385).sum(-1)
            ratio = (logp - old_logp[idx]).exp()
            if mb == 0:
                worst = float((ratio - 1).abs().max())
            a = adv[idx]
            a = (a - a.mean()) / (a.std() + 1e-8)
            loss = -torch.min(ratio * a, ratio.clamp(1 - clip, 1 + clip) * a).mean() + 0.5 * (ret[idx] - value).pow(2).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss))
        print(f"iteration {it}: {B} envs x {T} steps collected in {el * 1e3:.1f} ms: {B * T / el:.3e} env-steps/s; "
              f"first minibatch max |ratio - 1| = {worst:.3e}; loss {losses[0]:+.4f} -> {losses[-1]:+.4f}")
    mon = env.venv
    print(f"advantage mean {float(buf['advantages'].mean()):+.4f}, normalised reward mean {float(buf['rewards'].mean()):+.4f}, "
          f"episodes finished so far {int(mon.finished_t.sum())}, ODE failures {base.metrics()['n_ode_fail']:.0f}")
    base.close()


if __name__ == "__main__":
    main()
