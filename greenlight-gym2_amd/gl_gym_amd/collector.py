"""Rollout collection on the device (include/glgym.h glgym_ac_rows / glgym_gae): what stable_baselines3's
OnPolicyAlgorithm.collect_rollouts does between two optimiser phases -- observation -> stochastic policy and value -> env-step ->
buffer, then GAE(lambda).  The two heads are torch modules (TorchHeads); everything behind them -- the action noise, the sample, the
clip, the log-probability, the buffer writes -- is one library launch per step, and the advantages are one launch per rollout.  The
buffer, the noise and the advantages never leave the device; the optimiser phase over the buffer is gl_gym_amd.ppo.PPO, or the caller's.

    heads = TorchHeads(pi_module, vf_module, log_std)   # the modules the optimiser trains: nothing to copy back after a step
    col = RolloutCollector(env, 64, heads, gamma=0.9631)
    col.reset(seed=0)
    batch = col.collect()                               # dict of persistent device tensors, no synchronisation

Noise is Philox keyed by (seed, env index, step, draw): env b's actions do not depend on the number of envs or on torch's generator.
`draw_base_t`, a device word added to every draw index, advances by one per collect() (the Planner's convention)."""
from __future__ import annotations

import ctypes as C

from . import _lib as L


def _torch():
    import torch
    return torch


class TorchHeads:
    """A Gaussian policy and a value function as torch modules of any size (e.g. the reference's 3 x 256 policy and 3 x 512 value nets)
    and a state-independent log_std, evaluated under no_grad in front of every glgym_ac_rows call, which reads their outputs (mean_in /
    value_in).  pi_module: [B, obs_dim] -> [B, 6]; vf_module: [B, obs_dim] -> [B, 1] or [B]; log_std: a float32 [6] tensor or parameter,
    read at every collect().  The modules' outputs are torch allocations (the caching allocator's, at every step): what the collector
    itself adds stays allocation-free."""

    def __init__(self, pi_module, vf_module, log_std):
        t = self.torch = _torch()
        self.pi_module, self.vf_module, self._log_std_src = pi_module, vf_module, log_std
        self.device = log_std.device
        self.log_std = t.zeros(L.NU, dtype=t.float32, device=self.device)
        self.std = t.zeros(L.NU, dtype=t.float32, device=self.device)
        self.mean_t = self.value_t = None

    def bind(self, B):
        """Allocate the [B, 6] and [B] tensors the library reads the heads' outputs from."""
        t = self.torch
        self.mean_t = t.zeros(B, L.NU, dtype=t.float32, device=self.device)
        self.value_t = t.zeros(B, dtype=t.float32, device=self.device)

    def heads(self, obs_t):
        with self.torch.no_grad():
            self.mean_t.copy_(self.pi_module(obs_t).reshape(self.mean_t.shape))
            self.value_t.copy_(self.vf_module(obs_t).reshape(self.value_t.shape))

    def refresh(self):
        """log_std from its source, std = exp(log_std): the one transcendental outside the normals, once per collect()."""
        self.log_std.copy_(self._log_std_src.detach().reshape(L.NU))
        self.torch.exp(self.log_std, out=self.std)


class RolloutCollector:
    """n_steps x num_envs transitions per collect(), gathered on the device.  env: anything with reset_tensor / step_tensor / num_envs /
    obs_dim / device -- a bare TomatoVecEnv or the VecNormalizeGPU(VecMonitorGPU(...)) stack -- that also hands on the base
    environment's library handle and stream (`_lib`, `_h`, `_stream()`, which the package's wrappers forward from TomatoVecEnv): the
    two library calls are launched on them.  policy: a TorchHeads.

    Per step: the heads in torch, one glgym_ac_rows launch (observation into its buffer slot, noise, action, clipped action,
    log-probability, value), env.step_tensor on the clipped actions, two [B] copies (reward, done).  After the last step the value of the
    final observation (a value_only call) and one glgym_gae.  Everything of the collector's is allocated here and collect() never
    synchronises; the heads' outputs come from torch's caching allocator at every step."""

    def __init__(self, env, n_steps: int, policy, gamma: float = 0.99, gae_lambda: float = 0.95, seed: int = 0):
        t = self.torch = _torch()
        self.env, self.policy = env, policy
        self.T, self.B, self.D = int(n_steps), int(env.num_envs), int(env.obs_dim)
        self.device = t.device(env.device)
        if self.T < 1:
            raise ValueError("n_steps must be >= 1")
        if not (0.0 <= float(gamma) <= 1.0 and 0.0 <= float(gae_lambda) <= 1.0):
            raise ValueError("gamma and gae_lambda must lie in [0, 1]")
        self.gamma, self.gae_lambda, self.seed = float(gamma), float(gae_lambda), int(seed)
        T, B, D = self.T, self.B, self.D
        z = lambda *s, dtype=t.float32: t.zeros(*s, dtype=dtype, device=self.device)  # noqa: E731
        self.buffer = dict(observations=z(T, B, D), actions=z(T, B, L.NU), rewards=z(T, B), dones=z(T, B, dtype=t.uint8),
                           episode_starts=z(T, B, dtype=t.uint8), values=z(T, B), log_probs=z(T, B), advantages=z(T, B),
                           returns=z(T, B), last_values=z(B))
        self.action_env_t = z(B, L.NU)                        # what the env-step reads in place
        self.draw_base_t = z(1, dtype=t.int64)                # device word added to every draw index: + 1 per collect()
        self._last_done = t.ones(B, dtype=t.uint8, device=self.device)
        self.obs_t = None
        policy.bind(B)
        self._lib = L.load()
        a = self._ac = L.AcRowsArgs()
        a.struct_size, a.B, a.in_dim = C.sizeof(L.AcRowsArgs), B, D
        a.mean_in, a.value_in = policy.mean_t.data_ptr(), policy.value_t.data_ptr()
        a.log_std, a.std = policy.log_std.data_ptr(), policy.std.data_ptr()
        a.draw_index, a.draw_base = 0, self.draw_base_t.data_ptr()
        a.action_env, a.eps = self.action_env_t.data_ptr(), None
        b = self.buffer
        self._gae = L.make_plan_args(L.GaeArgs, T, B, b["rewards"].data_ptr(), b["dones"].data_ptr(), b["values"].data_ptr(),
                                     b["last_values"].data_ptr(), self.gamma, self.gae_lambda, b["advantages"].data_ptr(),
                                     b["returns"].data_ptr())
        self._slots = [(b["observations"][k].data_ptr(), b["actions"][k].data_ptr(), b["log_probs"][k].data_ptr(), b["values"][k].data_ptr())
                       for k in range(T)]

    def reset(self, seed=None):
        """Reset the env (with `seed` if given, which then also re-keys the action noise and rewinds draw_base_t) -> the observation."""
        self.obs_t = self.env.reset_tensor(seed)
        if seed is not None:
            self.seed = int(seed)
            self.draw_base_t.zero_()
        self._last_done.fill_(1)
        return self.obs_t

    def ac_rows(self, obs_t, step, slot=None, deterministic=False, value_only=False, value_ptr=None):
        """One glgym_ac_rows launch on the heads' present outputs: into buffer slot `slot`, or with value_only into value_ptr."""
        e, a = self.env, self._ac
        a.step, a.deterministic, a.value_only, a.seed, a.obs = int(step), int(deterministic), int(value_only), self.seed & (2 ** 64 - 1), obs_t.data_ptr()
        if value_only:
            a.obs_out = a.action = a.logp = None
            a.value = value_ptr
        else:
            a.obs_out, a.action, a.logp, a.value = self._slots[slot]
        L.check(self._lib.glgym_ac_rows(e._h, C.byref(a), e._stream()), "glgym_ac_rows")

    def collect(self, deterministic: bool = False):
        """-> the buffer: observations [T,B,D], actions [T,B,6] (raw, before the clip), rewards, dones (uint8), episode_starts (uint8),
        values, log_probs, advantages, returns [T,B], last_values [B].  The same tensors at every call."""
        t, b, p = self.torch, self.buffer, self.policy
        if self.obs_t is None:
            self.reset()
        with t.no_grad():
            p.refresh()
            b["episode_starts"][0].copy_(self._last_done)
            obs = self.obs_t
            for k in range(self.T):
                p.heads(obs)
                self.ac_rows(obs, k, slot=k, deterministic=deterministic)
                obs, rew, done = self.env.step_tensor(self.action_env_t)[:3]
                b["rewards"][k].copy_(rew)
                b["dones"][k].copy_(done)
            self.obs_t = obs
            p.heads(obs)
            self.ac_rows(obs, self.T, value_only=True, value_ptr=b["last_values"].data_ptr())
            e = self.env
            L.check(self._lib.glgym_gae(e._h, C.byref(self._gae), e._stream()), "glgym_gae")
            if self.T > 1:
                b["episode_starts"][1:].copy_(b["dones"][:-1])
            self._last_done.copy_(b["dones"][self.T - 1])
            self.draw_base_t.add_(1)
        return b
