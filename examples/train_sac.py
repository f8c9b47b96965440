#!/usr/bin/env python3
"""Soft actor-critic on the device: the replay ring, the squashed actor's sampling stage, the loss stages and the Polyak update are library
launches (gl_gym_amd.ReplayCollector, gl_gym_amd.SAC); the actor, the two critics, their target copies, autograd through them and the
optimisers are torch.  The stack of examples/train_ppo.py (TomatoVecEnv -> VecMonitorGPU -> VecNormalizeGPU) with the reference's SAC
hyper-parameters (configs/agents/sac.yml): actor 3 x 256 and critics 3 x 512 with SiLU, tau 0.0135, gamma 0.9631, Adam with amsgrad at
7e-4, Gaussian action noise of sigma 0.05, an automatic entropy coefficient, one gradient step per env-step.  Its batch_size of 128
belongs to 8 environments; here every env-step adds n_envs transitions, and the minibatch is --batch-size rows (default: n_envs).

    python examples/train_sac.py --n-envs 65536 --n-slots 16

Per iteration: the collection rate, the time of the gradient steps and their statistics (SAC.STATS).
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "greenlight-gym2_amd"))

import torch  # noqa: E402

from gl_gym_amd import SAC, ReplayCollector  # noqa: E402
from gl_gym_amd.tomato_env import TomatoVecEnv  # noqa: E402
from gl_gym_amd.utils import synthetic_weather  # noqa: E402
from gl_gym_amd.vec_monitor import VecMonitorGPU  # noqa: E402
from gl_gym_amd.vec_normalize import VecNormalizeGPU  # noqa: E402


def mlp(sizes):
    layers = []
    for a, b in zip(sizes[:-2], sizes[1:-1]):
        layers += [torch.nn.Linear(a, b), torch.nn.SiLU()]
    return torch.nn.Sequential(*layers, torch.nn.Linear(sizes[-2], sizes[-1]))


class Actor(torch.nn.Module):
    """[B, D] -> (mean [B, 6], log_std [B, 6]): a shared trunk and two linear heads, as stable_baselines3's SAC actor."""

    def __init__(self, D, H=256, n=3):
        super().__init__()
        self.trunk = torch.nn.Sequential(*[m for k in range(n) for m in (torch.nn.Linear(D if k == 0 else H, H), torch.nn.SiLU())])
        self.mu, self.log_std = torch.nn.Linear(H, 6), torch.nn.Linear(H, 6)

    def forward(self, obs):
        h = self.trunk(obs)
        return self.mu(h), self.log_std(h)


class Critic(torch.nn.Module):
    """(obs [M, D], action [M, 6]) -> q [M]."""

    def __init__(self, D, H=512, n=3):
        super().__init__()
        self.q = mlp([D + 6] + [H] * n + [1])

    def forward(self, obs, action):
        return self.q(torch.cat([obs, action], dim=-1)).squeeze(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=65536)
    ap.add_argument("--n-slots", type=int, default=16, help="replay ring: n_slots - 1 slots of n_envs transitions")
    ap.add_argument("--batch-size", type=int, default=None, help="minibatch rows (default: n_envs; the reference's 128 is for 8 environments)")
    ap.add_argument("--scheme", default="ls5", choices=["ls5", "rk4", "rk3", "rk2"])
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--train-freq", type=int, default=4, help="env-steps per iteration")
    ap.add_argument("--gradient-steps", type=int, default=4, help="gradient steps per iteration")
    ap.add_argument("--warmup-steps", type=int, default=2, help="env-steps with uniform actions before the first update (learning_starts)")
    args = ap.parse_args()

    w = synthetic_weather(n_rows=35040)
    starts = list(range(0, 35040 - 5760 - 60, 96))
    base = TomatoVecEnv(args.n_envs, weather=w, dtype="float32", scheme=args.scheme, season_length=60, start_rows=starts,
                        start_days=[s / 96.0 for s in starts], seed=666)
    gamma, tau, lr = 0.9631, 0.0135, 7e-4
    env = VecNormalizeGPU(VecMonitorGPU(base), norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=gamma)
    B, D = args.n_envs, base.obs_dim
    M = args.batch_size or B

    torch.manual_seed(0)
    dev = base.device
    actor, critic1, critic2 = Actor(D).to(dev), Critic(D).to(dev), Critic(D).to(dev)
    col = ReplayCollector(env, actor, args.n_slots, seed=0, action_noise_sigma=0.05)
    col.reset(seed=666)
    actor_opt = torch.optim.Adam(actor.parameters(), lr=lr, amsgrad=True)
    critic_opt = torch.optim.Adam(list(critic1.parameters()) + list(critic2.parameters()), lr=lr, amsgrad=True)
    sac = SAC(col, critic1, critic2, actor_opt, critic_opt, batch_size=M, gamma=gamma, tau=tau, ent_coef="auto", target_entropy=-6.0,
              target_update_interval=1, seed=0, max_gradient_steps=args.gradient_steps)

    col.collect(args.warmup_steps, explore="uniform")
    sac.update(1)                                        # warm-up (kernel code objects, optimiser states)
    torch.cuda.synchronize()
    for it in range(args.iterations):
        t0 = time.perf_counter()
        ring = col.collect(args.train_freq)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        stats = sac.update(args.gradient_steps)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        last = dict(zip(SAC.STATS, stats[-1].cpu().tolist()))
        print(f"iteration {it}: {B} envs x {args.train_freq} steps collected in {(t1 - t0) * 1e3:.1f} ms: {B * args.train_freq / (t1 - t0):.3e} env-steps/s; "
              f"{args.gradient_steps} gradient steps of {M} rows in {(t2 - t1) * 1e3:.1f} ms; ring {col.n_valid} of {col.S - 1} slots; normalised reward mean "
              f"{float(ring['rewards'].mean()):+.4f}; critic_loss {last['critic_loss']:.5f}, actor_loss {last['actor_loss']:+.5f}, "
              f"ent_coef_loss {last['ent_coef_loss']:+.5f}, alpha {last['alpha']:.5f}, logp_mean {last['logp_mean']:+.4f}")
    mon = env.venv
    print(f"episodes finished so far {int(mon.finished_t.sum())}, ODE failures {base.metrics()['n_ode_fail']:.0f}")
    base.close()


if __name__ == "__main__":
    main()
