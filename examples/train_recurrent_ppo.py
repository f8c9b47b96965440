#!/usr/bin/env python3
"""Recurrent PPO on the device: rollouts with a carried LSTM state by gl_gym_amd.RecurrentCollector, truncated back-propagation through
time over sequence minibatches by gl_gym_amd.RecurrentPPO -- the stack of examples/train_ppo.py (TomatoVecEnv -> VecMonitorGPU ->
VecNormalizeGPU) with the reference's RecurrentPPO hyper-parameters (configs/agents/recurrentppo.yml: MlpLstmPolicy with one LSTM layer of
64 and separate actor and critic LSTMs, pi 2 x 256 and vf 2 x 128 with silu, gamma 0.9631, lambda 0.9167, clip 0.2, normalised advantages,
ent_coef 0.05434, vf_coef 0.8225, max_grad_norm 0.3, Adam with amsgrad at 2e-5).  Its batch_size belongs to 8 environments; here a rollout
is n_envs x n_steps transitions cut into sequences of --seq-len steps, and an epoch into --minibatches minibatches of whole sequences.

    python examples/train_recurrent_ppo.py --n-envs 65536 --n-steps 64 --seq-len 16

Per iteration: the collection rate, the time of the update (the LSTM cells, the sequence gathers and the loss with its gradients are
library launches; the gate products, the heads, their backward pass and Adam are torch) and the mean normalised reward of the rollout.
"""
import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "greenlight-gym2_amd"))

import torch  # noqa: E402

from gl_gym_amd import RecurrentCollector, RecurrentHeads, RecurrentPPO  # noqa: E402
from gl_gym_amd.tomato_env import TomatoVecEnv  # noqa: E402
from gl_gym_amd.utils import synthetic_weather  # noqa: E402
from gl_gym_amd.vec_monitor import VecMonitorGPU  # noqa: E402
from gl_gym_amd.vec_normalize import VecNormalizeGPU  # noqa: E402


def mlp(n_in, width, n_out, dev):
    lin, act = torch.nn.Linear, torch.nn.SiLU
    return torch.nn.Sequential(lin(n_in, width), act(), lin(width, width), act(), lin(width, n_out)).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-envs", type=int, default=65536)
    ap.add_argument("--n-steps", type=int, default=64, help="rollout length per env (PPO n_steps)")
    ap.add_argument("--seq-len", type=int, default=16, help="steps of a sequence: the truncation length of back-propagation through time")
    ap.add_argument("--scheme", default="ls5", choices=["ls5", "rk4", "rk3", "rk2"])
    ap.add_argument("--lstm", type=int, default=64)
    ap.add_argument("--pi-width", type=int, default=256)
    ap.add_argument("--vf-width", type=int, default=128)
    ap.add_argument("--arrangement", default="separate", choices=["separate", "shared", "actor_only"])
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--epochs", type=int, default=8)
    ap.add_argument("--minibatches", type=int, default=4)
    args = ap.parse_args()

    w = synthetic_weather(n_rows=35040)
    starts = list(range(0, 35040 - 5760 - 60, 96))
    base = TomatoVecEnv(args.n_envs, weather=w, dtype="float32", scheme=args.scheme, season_length=60, start_rows=starts,
                        start_days=[s / 96.0 for s in starts], seed=666)
    gamma, lam = 0.9631, 0.9167
    env = VecNormalizeGPU(VecMonitorGPU(base), norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=gamma)
    B, T, D, H = args.n_envs, args.n_steps, base.obs_dim, args.lstm

    torch.manual_seed(0)
    dev = base.device
    lstm = lambda: torch.nn.LSTM(D, H).to(dev)  # noqa: E731
    log_std = torch.nn.Parameter(torch.zeros(6, device=dev))
    separate = args.arrangement == "separate"
    vf_in = D if args.arrangement == "actor_only" else H
    heads = RecurrentHeads(lstm(), mlp(H, args.pi_width, 6, dev), mlp(vf_in, args.vf_width, 1, dev), log_std,
                           lstm_vf=lstm() if separate else None, shared_lstm=args.arrangement == "shared")
    col = RecurrentCollector(env, T, heads, seq_len=args.seq_len, gamma=gamma, gae_lambda=lam, seed=0)
    col.reset(seed=666)
    opt = torch.optim.Adam(heads.parameters(), lr=2e-5, amsgrad=True)
    ppo = RecurrentPPO(col, opt, n_epochs=args.epochs, n_minibatches=args.minibatches, clip_range=0.2, normalize_advantage=True,
                       ent_coef=0.05434, vf_coef=0.8225, max_grad_norm=0.3, seed=0)

    col.collect()                                        # warm-up (kernel code objects)
    torch.cuda.synchronize()
    for it in range(args.iterations):
        t0 = time.perf_counter()
        buf = col.collect()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        stats = ppo.update()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        st = stats.cpu()
        first, last = dict(zip(RecurrentPPO.STATS, st[0, 0].tolist())), dict(zip(RecurrentPPO.STATS, st[-1, -1].tolist()))
        print(f"iteration {it}: {B} envs x {T} steps collected in {(t1 - t0) * 1e3:.1f} ms: {B * T / (t1 - t0):.3e} env-steps/s; "
              f"update ({args.epochs} epochs x {len(ppo.sizes)} minibatches of sequences of {args.seq_len}) in {(t2 - t1) * 1e3:.1f} ms; "
              f"normalised reward mean {float(buf['rewards'].mean()):+.4f}; loss {first['loss']:+.4f} -> {last['loss']:+.4f}, "
              f"approx_kl {last['approx_kl']:.3e}, clip_fraction {last['clip_fraction']:.3f}, first minibatch max ratio {first['max_ratio']:.6f}")
    mon = env.venv
    print(f"episodes finished so far {int(mon.finished_t.sum())}, ODE failures {base.metrics()['n_ode_fail']:.0f}")
    base.close()


if __name__ == "__main__":
    main()
