"""Soft actor-critic on the device (include/glgym.h glgym_sac_rows / glgym_sac_rows_grad / glgym_sac_batch / glgym_sac_loss /
glgym_polyak): what stable_baselines3's SAC does between the networks' outputs and their gradients -- the replay ring and its seeded
sampling, the tanh-squashed Gaussian with its reparameterised backward pass, the critic, actor and entropy-coefficient losses with their
gradients, the Polyak update of the target critics.  The actor, the two critics, their target copies, autograd through them and the
optimisers stay torch's.

    col = ReplayCollector(env, actor, n_slots=16, seed=0, action_noise_sigma=0.05)      # actor: [B, D] -> (mean [B, 6], log_std [B, 6])
    sac = SAC(col, critic1, critic2, actor_opt, critic_opt, batch_size=65536, gamma=0.9631, tau=0.0135)   # critic: (obs, action) -> [M]
    col.collect(4, explore="uniform")                   # the learning_starts warm-up
    for _ in range(100):
        col.collect(1)
        stats = sac.update(1)                           # [gradient_steps, 8] float64 on the device (SAC.STATS), no synchronisation

Noise and sampling are Philox keyed by (seed, row, step, draw): they depend on neither the batch size nor torch's generator.

Known differences from stable_baselines3.  A done row's next observation is the first one of the next episode (the env resets itself); it
is multiplied by 1 - done = 0 in the target.  TomatoEnv terminates and never truncates, so time-limit bootstrapping is out of scope, as in
the on-policy collector.  The ring stores what the env stack hands out: under VecNormalizeGPU that is observations and rewards normalised
at collection time, whereas stable_baselines3 stores raw ones and normalises them again at sample time.  The entropy coefficient's
gradient leaves the actor-stage launch, so its Adam step is applied after the actor's; the coefficient every stage of a gradient step
uses was formed before, which makes the result the one of SAC.train's order; likewise the policy's sample is drawn after the critic step
instead of before it (the actor's weights and the noise key are the same at both points)."""
from __future__ import annotations

import copy
import ctypes as C
import math

from . import _lib as L


def _torch():
    import torch
    return torch


# SAC's own samples (the policy's and the next actions') draw at 2^63 + the gradient step: a collector draws at step_count >> 30, so the
# two never share a "SAC1" key even when they were given the same seed
SAC_DRAW0 = 1 << 63


def _stream_of(stream):
    return stream if stream is not None else C.c_void_p(_torch().cuda.current_stream().cuda_stream)


class SquashedBuffers:
    """What glgym_sac_rows and glgym_sac_rows_grad write for up to M rows: action [M, 6], logp [M], the saved eps, std, tanh [M, 6], and
    grad_mean, grad_log_std [M, 6]."""

    def __init__(self, M: int, device):
        t = _torch()
        z = lambda *s: t.zeros(*s, dtype=t.float32, device=device)  # noqa: E731
        self.M = int(M)
        self.action, self.eps, self.std, self.tanh, self.grad_mean, self.grad_log_std = (z(M, L.NU) for _ in range(6))
        self.logp, self.zero_logp = z(M), z(M)
        self.zero_action = z(M, L.NU)


def sac_rows(handle, stream, M, *, mean=None, log_std=None, seed=0, step=0, draw_index=0, draw_base=None, row0=0, deterministic=False,
             uniform=False, action_noise_sigma=0.0, obs=None, obs_out=None, in_dim=0, action=None, action_env=None, action_slot=None,
             logp=None, eps=None, eps2=None, std=None, tanh=None, corr=None):
    """One glgym_sac_rows launch.  Tensors or raw device addresses (ints); None leaves an output out."""
    p = lambda x: None if x is None else x if isinstance(x, int) else x.data_ptr()  # noqa: E731
    a = L.make_plan_args(L.SacRowsArgs, int(M), int(in_dim), int(step), int(bool(deterministic)), int(bool(uniform)), int(row0), p(mean),
                         p(log_std), int(seed) & (2 ** 64 - 1), int(draw_index), p(draw_base), float(action_noise_sigma), p(obs), p(obs_out),
                         p(action), p(action_env), p(action_slot), p(logp), p(eps), p(eps2), p(std), p(tanh), p(corr))
    L.check(L.load().glgym_sac_rows(handle, C.byref(a), _stream_of(stream)), "glgym_sac_rows")


def _make_sample_fn():
    t = _torch()

    class _SquashedSample(t.autograd.Function):
        @staticmethod
        def forward(ctx, mean, log_std, call, call_grad):
            mean_c, ls_c = mean.detach().contiguous(), log_std.detach().contiguous()
            action, logp = call(mean_c, ls_c)
            ctx.ls, ctx.call_grad = ls_c, call_grad
            return action, logp

        @staticmethod
        def backward(ctx, grad_action, grad_logp):
            gm, gs = ctx.call_grad(grad_action, grad_logp, ctx.ls)
            return gm, gs, None, None

    return _SquashedSample


_SAMPLE_FN = None


def squashed_sample(mean, log_std, *, handle, stream=None, seed=0, step=0, draw_index=0, draw_base=None, row0=0, deterministic=False,
                    buffers=None):
    """A reparameterised sample of the tanh-squashed Gaussian N(mean, exp(clamp(log_std, -20, 2))) per row -> (action [M, 6], logp [M]),
    differentiable with respect to mean and log_std [M, 6]: forward is one glgym_sac_rows launch, backward one glgym_sac_rows_grad launch.
    handle: the library handle of an environment (env._h).  buffers: a SquashedBuffers for at least M rows (default: allocated here); the
    results are views of it, valid until its next use."""
    global _SAMPLE_FN
    t = _torch()
    if _SAMPLE_FN is None:
        _SAMPLE_FN = _make_sample_fn()
    M = int(mean.shape[0])
    if tuple(mean.shape) != (M, L.NU) or tuple(log_std.shape) != (M, L.NU):
        raise ValueError("squashed_sample: mean and log_std must both be [M, 6]")
    buf = buffers if buffers is not None else SquashedBuffers(M, mean.device)
    if buf.M < M:
        raise ValueError(f"squashed_sample: buffers hold {buf.M} rows, the batch has {M}")
    lib = L.load()

    def call(mean_c, ls_c):
        sac_rows(handle, stream, M, mean=mean_c, log_std=ls_c, seed=seed, step=step, draw_index=draw_index, draw_base=draw_base, row0=row0,
                 deterministic=deterministic, action=buf.action, logp=buf.logp, eps=buf.eps, std=buf.std, tanh=buf.tanh)
        return buf.action[:M], buf.logp[:M]

    def call_grad(grad_action, grad_logp, ls_c):
        ga = buf.zero_action[:M] if grad_action is None else grad_action.to(t.float32).contiguous()
        gl = buf.zero_logp[:M] if grad_logp is None else grad_logp.to(t.float32).contiguous()
        a = L.make_plan_args(L.SacRowsGradArgs, M, ga.data_ptr(), gl.data_ptr(), buf.eps.data_ptr(), buf.std.data_ptr(), buf.tanh.data_ptr(),
                             ls_c.data_ptr(), buf.grad_mean.data_ptr(), buf.grad_log_std.data_ptr())
        L.check(lib.glgym_sac_rows_grad(handle, C.byref(a), _stream_of(stream)), "glgym_sac_rows_grad")
        return buf.grad_mean[:M], buf.grad_log_std[:M]

    return _SAMPLE_FN.apply(mean, log_std, call, call_grad)


def _make_loss_fn():
    t = _torch()

    class _SacLoss(t.autograd.Function):
        """forward: call(*detached contiguous inputs) -> (gradients, scalar); backward: the gradients times grad_output."""

        @staticmethod
        def forward(ctx, call, *xs):
            grads, loss = call(*[x.detach().reshape(-1).contiguous() for x in xs])
            ctx.grads, ctx.shapes = grads, [x.shape for x in xs]
            return loss

        @staticmethod
        def backward(ctx, grad_output):
            g = grad_output.to(t.float32)
            return (None,) + tuple((gr * g).reshape(s) for gr, s in zip(ctx.grads, ctx.shapes))

    return _SacLoss


_LOSS_FN = None


class ReplayCollector:
    """A replay ring of n_slots x num_envs transitions, filled on the device.  env: a bare TomatoVecEnv or the
    VecNormalizeGPU(VecMonitorGPU(...)) stack (anything with reset_tensor / step_tensor / num_envs / obs_dim / device that hands on `_lib`,
    `_h`, `_stream()`).  actor: a torch module [B, D] -> (mean [B, 6], log_std [B, 6]).

    The ring is slot-major -- obs [S, B, D], action [S, B, 6] (the executed action), reward [S, B], done [S, B] uint8 -- and an observation
    is stored once: the next observation of slot s is the observation of slot (s + 1) mod S, so n_slots - 1 slots hold transitions.
    Per step: the actor under no_grad, one glgym_sac_rows launch (observation into the slot, executed action into the slot and into the
    env's action tensor), env.step_tensor, two [B] copies (reward, done), the slot counters (host integers: every step adds B rows).  After
    the last step one [B, D] copy of the current observation into the next slot.  Nothing synchronises; nothing of the collector's is
    allocated after construction (the actor's outputs are torch's)."""

    def __init__(self, env, actor, n_slots: int, seed: int = 0, action_noise_sigma=None):
        t = self.torch = _torch()
        self.env, self.actor = env, actor
        self.S, self.B, self.D = int(n_slots), int(env.num_envs), int(env.obs_dim)
        if self.S < 2:
            raise ValueError("n_slots must be >= 2: a transition's next observation is the next slot's")
        sigma = 0.0 if action_noise_sigma is None else float(action_noise_sigma)
        if not (sigma >= 0.0 and math.isfinite(sigma)):
            raise ValueError("action_noise_sigma must be >= 0 and finite, or None")
        self.sigma, self.seed = sigma, int(seed)
        self.device = t.device(env.device)
        S, B, D = self.S, self.B, self.D
        z = lambda *s, dtype=t.float32: t.zeros(*s, dtype=dtype, device=self.device)  # noqa: E731
        self.ring = dict(observations=z(S, B, D), actions=z(S, B, L.NU), rewards=z(S, B), dones=z(S, B, dtype=t.uint8))
        self.action_env_t = z(B, L.NU)                        # what the env-step reads in place
        self.mean_t, self.log_std_t = z(B, L.NU), z(B, L.NU)
        self.draw_base_t = z(1, dtype=t.int64)
        self.obs_t = None
        self.pos = self.filled = self.step_count = 0
        self._lib = L.load()

    @property
    def n_valid(self):
        """Slots whose successor observation is written."""
        return min(self.filled, self.S - 1)

    @property
    def head(self):
        """The oldest valid slot."""
        return (self.pos - self.n_valid) % self.S

    @property
    def num_timesteps(self):
        return self.step_count * self.B

    def reset(self, seed=None):
        """Reset the env (with `seed` if given, which then also REPLACES the constructor's seed as the key of the action noise) and empty the
        ring -> the observation."""
        self.obs_t = self.env.reset_tensor(seed)
        if seed is not None:
            self.seed = int(seed)
        self.pos = self.filled = self.step_count = 0
        return self.obs_t

    def collect(self, n_steps: int = 1, explore: str = "policy", deterministic: bool = False):
        """n_steps env-steps into the ring -> the ring (the same tensors at every call).  explore = "uniform": actions uniform in [-1, 1]
        (the learning_starts warm-up), the actor is not evaluated."""
        if explore not in ("policy", "uniform"):
            raise ValueError('explore must be "policy" or "uniform"')
        t, r, e = self.torch, self.ring, self.env
        if self.obs_t is None:
            self.reset()
        uniform = explore == "uniform"
        with t.no_grad():
            obs = self.obs_t
            for _ in range(int(n_steps)):
                if not uniform:
                    mean, log_std = self.actor(obs)
                    self.mean_t.copy_(mean.reshape(self.mean_t.shape))
                    self.log_std_t.copy_(log_std.reshape(self.log_std_t.shape))
                k = self.pos
                sac_rows(e._h, e._stream(), self.B, mean=None if uniform else self.mean_t, log_std=None if uniform else self.log_std_t,
                         seed=self.seed, step=self.step_count % (1 << 30), draw_index=self.step_count >> 30, draw_base=self.draw_base_t,
                         deterministic=deterministic and not uniform, uniform=uniform, action_noise_sigma=self.sigma, obs=obs,
                         obs_out=r["observations"][k], in_dim=self.D, action_env=self.action_env_t, action_slot=r["actions"][k])
                obs, rew, done = e.step_tensor(self.action_env_t)[:3]
                r["rewards"][k].copy_(rew)
                r["dones"][k].copy_(done)
                self.pos = (k + 1) % self.S
                self.filled = min(self.filled + 1, self.S)
                self.step_count += 1
            self.obs_t = obs
            r["observations"][self.pos].copy_(obs)            # the newest transition's next observation
        return r


class SAC:
    """The gradient steps of soft actor-critic over a ReplayCollector's ring, in the order of stable_baselines3's SAC.train.  The actor is
    collector.actor; critic1 and critic2 map (obs [M, D], action [M, 6]) to [M] or [M, 1]; their target copies are made here.

    update(gradient_steps), per gradient step: glgym_sac_batch -> alpha = exp(log_alpha) -> the next actions and the target critics under
    no_grad, glgym_sac_loss (critic stage), critic step -> the actor with grad and squashed_sample, the critics on its actions,
    glgym_sac_loss (actor stage), backward through the critics into squashed_sample (the critics' gradients are discarded), actor step,
    then the entropy coefficient's own Adam step on the gradient the same launch left -> glgym_polyak every target_update_interval steps
    -> the draw word + 1.  Returns stats_t [gradient_steps, 8] (SAC.STATS; float64, on the device).  Never synchronises.
    Out of scope, refused: use_sde, n_critics != 2, learning-rate schedules, recurrent policies (the on-policy recurrent agent is
    gl_gym_amd.recurrent_ppo), prioritised replay."""

    STATS = L.SAC_STATS

    def __init__(self, collector, critic1, critic2, actor_optimizer, critic_optimizer, batch_size: int = 256, gamma: float = 0.99,
                 tau: float = 0.005, ent_coef="auto", target_entropy: float = -6.0, target_update_interval: int = 1, seed: int = 0,
                 ent_coef_lr=None, max_gradient_steps: int = 64, use_sde: bool = False, n_critics: int = 2, learning_rate=None,
                 recurrent: bool = False, prioritized_replay: bool = False):
        t = self.torch = _torch()
        if use_sde:
            raise NotImplementedError("SAC: use_sde (state-dependent exploration) is out of scope")
        if int(n_critics) != 2:
            raise NotImplementedError("SAC: n_critics must be 2 (the loss stage is the twin-critic one)")
        if callable(learning_rate):
            raise NotImplementedError("SAC: learning-rate schedules are out of scope (the optimisers are the caller's)")
        if recurrent:
            raise NotImplementedError("SAC: recurrent policies are out of scope")
        if prioritized_replay:
            raise NotImplementedError("SAC: prioritised replay is out of scope (sampling is uniform with replacement)")
        if not (0.0 <= float(gamma) <= 1.0 and 0.0 <= float(tau) <= 1.0):
            raise ValueError("gamma and tau must lie in [0, 1]")
        if int(batch_size) < 1 or int(target_update_interval) < 1:
            raise ValueError("batch_size and target_update_interval must be >= 1")
        auto = isinstance(ent_coef, str)
        if auto:
            if not ent_coef.startswith("auto"):
                raise ValueError('ent_coef must be "auto", "auto_<initial value>" or a number')
            init = float(ent_coef.split("_")[1]) if "_" in ent_coef else 1.0
        else:
            init = float(ent_coef)
        if not (init > 0.0 and math.isfinite(init)):
            raise ValueError("the (initial) entropy coefficient must be > 0 and finite")
        self.collector, self.critic1, self.critic2 = collector, critic1, critic2
        self.actor_optimizer, self.critic_optimizer = actor_optimizer, critic_optimizer
        self.M = self.batch_size = int(batch_size)
        self.gamma, self.tau, self.target_entropy = float(gamma), float(tau), float(target_entropy)
        self.target_update_interval, self.seed, self.auto_ent = int(target_update_interval), int(seed), auto
        self.n_updates = 0
        col = collector
        dev, D, M = col.device, col.D, self.M
        self.actor = col.actor
        self.target1, self.target2 = copy.deepcopy(critic1), copy.deepcopy(critic2)
        for p in list(self.target1.parameters()) + list(self.target2.parameters()):
            p.requires_grad_(False)
        z = lambda *s, dtype=t.float32: t.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        self.mb = dict(observations=z(M, D), next_observations=z(M, D), actions=z(M, L.NU), rewards=z(M), dones=z(M, dtype=t.uint8))
        self.pi_buffers, self.next_buffers = SquashedBuffers(M, dev), SquashedBuffers(M, dev)
        self.log_alpha = t.full((1,), math.log(init), dtype=t.float32, device=dev, requires_grad=auto)
        self.alpha_t, self.grad_log_alpha_t = z(1), z(1)
        self.ent_optimizer = None
        if auto:
            lr = ent_coef_lr if ent_coef_lr is not None else actor_optimizer.param_groups[0]["lr"]
            self.ent_optimizer = t.optim.Adam([self.log_alpha], lr=float(lr))
            self.log_alpha.grad = self.grad_log_alpha_t
        self.grad_q1, self.grad_q2, self.grad_logp, self.target_t = z(M), z(M), z(M), z(M)
        self.workspace = z(L.SAC_LOSS_WS_BYTES // 8, dtype=t.float64)
        self.draw_t = z(1, dtype=t.int64)                     # device word added to the draw index: + 1 per gradient step
        self._alloc_stats(int(max_gradient_steps))
        self._lib = L.load()
        # the Polyak table, uploaded once, 64 tensors per launch
        pairs = [(q, p) for tgt, src in ((self.target1, critic1), (self.target2, critic2)) for q, p in zip(tgt.parameters(), src.parameters())]
        for q, p in pairs:
            if not (q.is_contiguous() and p.is_contiguous() and q.dtype == t.float32 and p.dtype == t.float32):
                raise ValueError("SAC: the critics' parameters must be contiguous float32 tensors")
        self._polyak, self._polyak_tables = [], []
        self._polyak_pairs = [(q, p, q.data_ptr(), p.data_ptr()) for q, p in pairs]
        for o in range(0, len(pairs), L.SAC_MAX_TENSORS):
            part = pairs[o:o + L.SAC_MAX_TENSORS]
            dst = t.tensor([q.data_ptr() for q, _ in part], dtype=t.int64, device=dev)
            src = t.tensor([p.data_ptr() for _, p in part], dtype=t.int64, device=dev)
            cnt = t.tensor([q.numel() for q, _ in part], dtype=t.int64, device=dev)
            self._polyak_tables.append((dst, src, cnt))
            self._polyak.append(L.make_plan_args(L.PolyakArgs, len(part), dst.data_ptr(), src.data_ptr(), cnt.data_ptr(),
                                                 max(q.numel() for q, _ in part), self.tau))

    def _alloc_stats(self, G):
        t = self.torch
        z = lambda *s: t.zeros(*s, dtype=t.float64, device=self.collector.device)  # noqa: E731
        self.max_gradient_steps = G
        self.stats_t, self.critic_stats_t, self.actor_stats_t = z(G, 8), z(G, 8), z(G, 8)

    # ---- the stages of one gradient step ----------------------------------------------------------------------------------------------
    def batch(self):
        """Draw the minibatch of the present draw word from the ring -> its tensors (the same at every call)."""
        col, e, r, mb = self.collector, self.collector.env, self.collector.ring, self.mb
        a = L.make_plan_args(L.SacBatchArgs, col.S, col.B, col.D, self.M, col.head, col.n_valid, 0, self.seed & (2 ** 64 - 1), 0,
                             self.draw_t.data_ptr(), r["observations"].data_ptr(), r["actions"].data_ptr(), r["rewards"].data_ptr(),
                             r["dones"].data_ptr(), mb["observations"].data_ptr(), mb["next_observations"].data_ptr(), mb["actions"].data_ptr(),
                             mb["rewards"].data_ptr(), mb["dones"].data_ptr(), None)
        L.check(self._lib.glgym_sac_batch(e._h, C.byref(a), e._stream()), "glgym_sac_batch")
        return mb

    def _loss(self, stage, stats_row, *xs):
        global _LOSS_FN
        if _LOSS_FN is None:
            _LOSS_FN = _make_loss_fn()
        e, M = self.collector.env, self.M
        critic = stage == L.SAC_CRITIC

        def call(q1, q2, logp=None):
            nb = self.next_buffers
            lp = nb.logp if critic else logp
            a = L.make_plan_args(L.SacLossArgs, M, stage, 0, q1.data_ptr(), q2.data_ptr(), lp.data_ptr(),
                                 self._q1n.data_ptr() if critic else None, self._q2n.data_ptr() if critic else None,
                                 self.mb["rewards"].data_ptr() if critic else None, self.mb["dones"].data_ptr() if critic else None,
                                 self.alpha_t.data_ptr(), None if critic else self.log_alpha.data_ptr(), self.gamma, self.target_entropy,
                                 self.grad_q1.data_ptr(), self.grad_q2.data_ptr(), None if critic else self.grad_logp.data_ptr(),
                                 self.target_t.data_ptr() if critic else None, None if critic else self.grad_log_alpha_t.data_ptr(),
                                 stats_row.data_ptr(), self.workspace.data_ptr(), L.SAC_LOSS_WS_BYTES)
            L.check(self._lib.glgym_sac_loss(e._h, C.byref(a), e._stream()), "glgym_sac_loss")
            return ((self.grad_q1, self.grad_q2) if critic else (self.grad_q1, self.grad_q2, self.grad_logp)), stats_row[0]

        return _LOSS_FN.apply(call, *xs)

    def refresh_alpha(self):
        with self.torch.no_grad():
            self.torch.exp(self.log_alpha, out=self.alpha_t)

    def critic_step(self, stats_row=None):
        """Next actions and target critics under no_grad, the critic stage of glgym_sac_loss, the critic optimiser's step."""
        t, e, mb, M = self.torch, self.collector.env, self.mb, self.M
        row = stats_row if stats_row is not None else self.critic_stats_t[0]
        with t.no_grad():
            mean_n, ls_n = self.actor(mb["next_observations"])
            nb = self.next_buffers
            sac_rows(e._h, e._stream(), M, mean=mean_n.contiguous(), log_std=ls_n.contiguous(), seed=self.seed, step=1, draw_index=SAC_DRAW0,
                     draw_base=self.draw_t,
                     action=nb.action, logp=nb.logp)
            self._q1n = self.target1(mb["next_observations"], nb.action).reshape(-1).contiguous()
            self._q2n = self.target2(mb["next_observations"], nb.action).reshape(-1).contiguous()
        loss = self._loss(L.SAC_CRITIC, row, self.critic1(mb["observations"], mb["actions"]), self.critic2(mb["observations"], mb["actions"]))
        self.critic_optimizer.zero_grad(set_to_none=False)
        loss.backward()
        self.critic_optimizer.step()
        return loss

    def actor_step(self, stats_row=None):
        """The actor with grad, squashed_sample, the critics on its actions, the actor stage of glgym_sac_loss, the actor optimiser's step and
        the entropy coefficient's."""
        # Runs after critic_step, where SAC.train samples before it and steps the entropy coefficient before the critics: the numbers are
        # the same only as long as nothing between refresh_alpha() and here writes log_alpha, alpha_t, the actor's weights or the draw word.
        e, mb = self.collector.env, self.mb
        row = stats_row if stats_row is not None else self.actor_stats_t[0]
        mean, log_std = self.actor(mb["observations"])
        a_pi, logp_pi = squashed_sample(mean, log_std, handle=e._h, stream=e._stream(), seed=self.seed, step=0, draw_index=SAC_DRAW0, draw_base=self.draw_t,
                                        buffers=self.pi_buffers)
        loss = self._loss(L.SAC_ACTOR, row, self.critic1(mb["observations"], a_pi), self.critic2(mb["observations"], a_pi), logp_pi)
        self.actor_optimizer.zero_grad(set_to_none=False)
        loss.backward()                                       # also into the critics' .grad, zeroed before their next step
        self.actor_optimizer.step()
        if self.ent_optimizer is not None:
            self.log_alpha.grad = self.grad_log_alpha_t       # what the actor-stage launch left
            self.ent_optimizer.step()
        return loss

    def polyak(self):
        """The table holds the parameters' addresses as they were at construction: the critics' and the target critics' parameters must stay
        in place (no .to(), no re-created or re-assigned tensors); in-place updates such as an optimiser's or load_state_dict's are fine."""
        e = self.collector.env
        for q, p, aq, ap in self._polyak_pairs:
            if q.data_ptr() != aq or p.data_ptr() != ap:
                raise RuntimeError("SAC.polyak: a critic or target-critic parameter has moved since construction; build a new SAC")
        for a in self._polyak:
            L.check(self._lib.glgym_polyak(e._h, C.byref(a), e._stream()), "glgym_polyak")

    def update(self, gradient_steps: int = 1):
        G = int(gradient_steps)
        if G < 1:
            raise ValueError("gradient_steps must be >= 1")
        if self.collector.n_valid < 1:
            raise ValueError("SAC.update: the ring holds no transition yet (collect first)")
        if G > self.max_gradient_steps:
            self._alloc_stats(G)
        for g in range(G):
            self.batch()
            self.refresh_alpha()
            self.critic_step(self.critic_stats_t[g])
            self.actor_step(self.actor_stats_t[g])
            self.n_updates += 1
            if self.n_updates % self.target_update_interval == 0:
                self.polyak()
            self.draw_t.add_(1)
        s, c, a = self.stats_t, self.critic_stats_t, self.actor_stats_t
        for k, (src, j) in enumerate(((c, 0), (a, 0), (a, 1), (a, 4), (a, 3), (c, 3), (c, 5), (c, 7))):
            s[:G, k].copy_(src[:G, j])
        return s[:G]

    def learn(self, n_iterations: int, train_freq: int = 1, gradient_steps: int = 1, learning_starts: int = 0):
        """n_iterations times: collect(train_freq) -- uniform actions until learning_starts transitions have been collected -- then
        update(gradient_steps) once they have -> the stats of the last update (None if there was none)."""
        col, out = self.collector, None
        for _ in range(int(n_iterations)):
            col.collect(int(train_freq), explore="uniform" if col.num_timesteps < int(learning_starts) else "policy")
            if col.num_timesteps >= int(learning_starts):
                out = self.update(int(gradient_steps))
        return out
