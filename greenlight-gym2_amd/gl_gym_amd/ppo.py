"""The PPO update on the device (include/glgym.h glgym_ppo_batch / glgym_ppo_loss): what stable_baselines3's PPO.train does around the
two heads -- the shuffle, the minibatch gathers, the advantage normalisation, the clipped-surrogate loss and its gradients with respect to
the heads' outputs.  The heads, their backward pass, the gradient clip and the optimiser stay torch's.

    col = RolloutCollector(env, 64, TorchHeads(pi, vf, log_std), gamma=0.9631)
    ppo = PPO(col, torch.optim.Adam(params, lr=3e-4), n_epochs=8, n_minibatches=4)
    for _ in range(100):
        col.collect()
        stats = ppo.update()                            # [n_epochs, n_minibatches, 8] float64 on the device (PPO.STATS), no synchronisation

The shuffle is a keyed permutation of (seed, draw word, N): it does not depend on the minibatch size or on torch's generator.  The draw
word is a device tensor that advances by one per epoch."""
from __future__ import annotations

import ctypes as C
import math

from . import _lib as L


def _torch():
    import torch
    return torch


class PpoLossBuffers:
    """What one glgym_ppo_loss call writes, for minibatches of up to M rows: grad_mean [M, 6], grad_value [M], grad_log_std [6], inv_std [6],
    stats [8] float64 and the reduction's workspace."""

    def __init__(self, M: int, device):
        t = _torch()
        z = lambda *s, dtype=t.float32: t.zeros(*s, dtype=dtype, device=device)  # noqa: E731
        self.M = int(M)
        self.grad_mean, self.grad_value, self.grad_log_std, self.inv_std = z(M, L.NU), z(M), z(L.NU), z(L.NU)
        self.stats = z(8, dtype=t.float64)
        self.workspace = z(L.PPO_LOSS_WS_BYTES // 8, dtype=t.float64)


def _make_loss_fn():
    t = _torch()

    class _PpoLoss(t.autograd.Function):
        @staticmethod
        def forward(ctx, mean, value, log_std, call):
            mean_c, value_c, log_std_c = mean.detach().contiguous(), value.detach().reshape(-1).contiguous(), log_std.detach().contiguous()
            gm, gv, gl, stats = call(mean_c, value_c, log_std_c)
            ctx.save_for_backward(gm, gv, gl)
            ctx.shapes = (mean.shape, value.shape, log_std.shape)
            return stats[0]

        @staticmethod
        def backward(ctx, grad_output):
            gm, gv, gl = ctx.saved_tensors
            g = grad_output.to(t.float32)
            sm, sv, sl = ctx.shapes
            return (gm * g).reshape(sm), (gv * g).reshape(sv), (gl * g).reshape(sl), None

    return _PpoLoss


_LOSS_FN = None


def ppo_loss(mean, value, log_std, minibatch, *, handle, stream=None, clip_range=0.2, clip_range_vf=None, vf_coef=0.5, ent_coef=0.0,
             buffers=None, stats_out=None):
    """The clipped-surrogate PPO loss of one minibatch as a differentiable scalar (float64, on the device): forward is one glgym_ppo_loss call,
    which also leaves the gradients with respect to mean [M, 6], value [M] or [M, 1] and log_std [6]; backward hands them on times grad_output.

    minibatch: dict with "actions" [M, 6], "log_probs", "advantages", "returns" [M] (float32, contiguous), "values" [M] with clip_range_vf, and
    "adv_stats" (float64 [2]: mean and unbiased standard deviation, glgym_ppo_batch's) or None for unnormalised advantages.
    handle: the library handle of an environment (env._h); stream: a HIP stream as c_void_p (default: torch's current stream).
    buffers: a PpoLossBuffers for at least M rows (default: allocated here); stats_out: a float64 [8] tensor for the stats (default: buffers.stats)."""
    global _LOSS_FN
    t = _torch()
    if _LOSS_FN is None:
        _LOSS_FN = _make_loss_fn()
    if callable(clip_range) or callable(clip_range_vf):
        raise NotImplementedError("ppo_loss: clip schedules are out of scope (a clip range is a number)")
    M = int(mean.shape[0])
    buf = buffers if buffers is not None else PpoLossBuffers(M, mean.device)
    if buf.M < M:
        raise ValueError(f"ppo_loss: buffers hold {buf.M} rows, the minibatch has {M}")
    stats = stats_out if stats_out is not None else buf.stats
    lib = L.load()
    mb = minibatch
    for k in ("actions", "log_probs", "advantages", "returns"):
        if not (mb[k].is_contiguous() and mb[k].dtype == t.float32 and mb[k].shape[0] == M):
            raise ValueError(f"ppo_loss: minibatch[{k!r}] must be contiguous float32 with {M} rows")
    old_v, adv_stats = mb.get("values"), mb.get("adv_stats")

    def call(mean_c, value_c, log_std_c):
        with t.no_grad():
            t.exp(-log_std_c, out=buf.inv_std)
        a = L.make_plan_args(L.PpoLossArgs, M, mean_c.data_ptr(), value_c.data_ptr(), log_std_c.data_ptr(), buf.inv_std.data_ptr(),
                             mb["actions"].data_ptr(), mb["log_probs"].data_ptr(), mb["advantages"].data_ptr(), mb["returns"].data_ptr(),
                             None if old_v is None else old_v.data_ptr(), None if adv_stats is None else adv_stats.data_ptr(),
                             float(clip_range), 0.0 if clip_range_vf is None else float(clip_range_vf), float(vf_coef), float(ent_coef),
                             buf.grad_mean.data_ptr(), buf.grad_value.data_ptr(), buf.grad_log_std.data_ptr(), stats.data_ptr(), None, None,
                             buf.workspace.data_ptr(), L.PPO_LOSS_WS_BYTES)
        s = stream if stream is not None else C.c_void_p(t.cuda.current_stream().cuda_stream)
        L.check(lib.glgym_ppo_loss(handle, C.byref(a), s), "glgym_ppo_loss")
        return buf.grad_mean[:M], buf.grad_value[:M], buf.grad_log_std, stats

    return _LOSS_FN.apply(mean, value, log_std, call)


class PPO:
    """The optimiser phase of PPO over a RolloutCollector's buffer.  collector.policy's pi_module, vf_module and log_std source are what
    `optimizer` trains.  Either n_minibatches (minibatches of ceil(N / n_minibatches) rows) or batch_size; when N is no multiple of the
    minibatch size the last minibatch is smaller, as in stable_baselines3.

    update(): for every epoch, for every minibatch: glgym_ppo_batch (gather + advantage statistics) -> the heads in torch with grad ->
    ppo_loss -> backward -> clip_grad_norm_ -> optimizer.step; then the draw word + 1.  Returns stats_t [n_epochs, n_minibatches, 8]
    (PPO.STATS; float64, on the device).  Never synchronises; everything of its own is allocated in the constructor.
    Out of scope, refused: target_kl (a host decision per minibatch), learning-rate and clip schedules.  Recurrent policies: gl_gym_amd.recurrent_ppo
    (RecurrentCollector, RecurrentPPO)."""

    STATS = L.PPO_STATS

    def __init__(self, collector, optimizer, n_epochs: int = 8, n_minibatches: int = 4, batch_size=None, clip_range: float = 0.2,
                 clip_range_vf=None, normalize_advantage: bool = True, ent_coef: float = 0.0, vf_coef: float = 0.5, max_grad_norm=0.5,
                 seed: int = 0, target_kl=None):
        t = self.torch = _torch()
        if target_kl is not None:
            raise NotImplementedError("PPO: target_kl is out of scope: it needs a host decision per minibatch")
        if callable(clip_range) or callable(clip_range_vf):
            raise NotImplementedError("PPO: clip schedules are out of scope (a clip range is a number)")
        if not (float(clip_range) > 0.0 and math.isfinite(float(clip_range))):
            raise ValueError("clip_range must be > 0 and finite")
        if clip_range_vf is not None and not float(clip_range_vf) > 0.0:
            raise ValueError("clip_range_vf must be > 0, or None")
        self.collector, self.optimizer = collector, optimizer
        self.n_epochs, self.seed = int(n_epochs), int(seed)
        self.clip_range, self.clip_range_vf = float(clip_range), None if clip_range_vf is None else float(clip_range_vf)
        self.normalize_advantage, self.ent_coef, self.vf_coef, self.max_grad_norm = bool(normalize_advantage), float(ent_coef), float(vf_coef), max_grad_norm
        col = collector
        N = self.N = col.T * col.B
        M = self.batch_size = int(batch_size) if batch_size is not None else -(-N // int(n_minibatches))
        if self.n_epochs < 1 or not 1 <= M <= N:
            raise ValueError("n_epochs must be >= 1 and the minibatch size in 1 .. n_steps * num_envs")
        self.sizes = [min(M, N - o) for o in range(0, N, M)]
        if self.normalize_advantage and min(self.sizes) < 2:
            raise ValueError("normalize_advantage needs at least 2 rows in every minibatch (the last one would have 1)")
        dev, D = col.device, col.D
        z = lambda *s, dtype=t.float32: t.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        self.mb = dict(observations=z(M, D), actions=z(M, L.NU), log_probs=z(M), advantages=z(M), returns=z(M), values=z(M))
        self.adv_stats_t = z(2, dtype=t.float64)
        self.batch_ws_t = z(L.PPO_BATCH_WS_BYTES // 8, dtype=t.float64)
        self.loss_buffers = PpoLossBuffers(M, dev)
        self.stats_t = z(self.n_epochs, len(self.sizes), 8, dtype=t.float64)
        self.draw_t = z(1, dtype=t.int64)                     # device word added to the draw index: + 1 per epoch
        self._lib = L.load()
        b = col.buffer
        self._batch_args, self._views = [], []
        for i, m in enumerate(self.sizes):
            self._batch_args.append(L.make_plan_args(
                L.PpoBatchArgs, N, m, i * M, D, self.seed & (2 ** 64 - 1), 0, self.draw_t.data_ptr(), b["observations"].data_ptr(),
                b["actions"].data_ptr(), b["log_probs"].data_ptr(), b["advantages"].data_ptr(), b["returns"].data_ptr(), b["values"].data_ptr(),
                self.mb["observations"].data_ptr(), self.mb["actions"].data_ptr(), self.mb["log_probs"].data_ptr(),
                self.mb["advantages"].data_ptr(), self.mb["returns"].data_ptr(), self.mb["values"].data_ptr(), None,
                self.adv_stats_t.data_ptr() if self.normalize_advantage else None,
                self.batch_ws_t.data_ptr() if self.normalize_advantage else None, L.PPO_BATCH_WS_BYTES))
            v = {k: x[:m] for k, x in self.mb.items()}
            v["adv_stats"] = self.adv_stats_t if self.normalize_advantage else None
            if self.clip_range_vf is None:
                v["values"] = None
            self._views.append(v)
        p = col.policy
        self._params = [q for g in optimizer.param_groups for q in g["params"]]
        self._pi, self._vf, self._log_std = p.pi_module, p.vf_module, p._log_std_src

    def batch(self, i: int):
        """Gather minibatch i of the present epoch's permutation -> its views (the same tensors at every call)."""
        e = self.collector.env
        L.check(self._lib.glgym_ppo_batch(e._h, C.byref(self._batch_args[i]), e._stream()), "glgym_ppo_batch")
        return self._views[i]

    def update(self):
        t, e = self.torch, self.collector.env
        for epoch in range(self.n_epochs):
            for i in range(len(self.sizes)):
                mb = self.batch(i)
                obs = mb["observations"]
                loss = ppo_loss(self._pi(obs), self._vf(obs), self._log_std, mb, handle=e._h, stream=e._stream(), clip_range=self.clip_range,
                                clip_range_vf=self.clip_range_vf, vf_coef=self.vf_coef, ent_coef=self.ent_coef, buffers=self.loss_buffers,
                                stats_out=self.stats_t[epoch, i])
                self.optimizer.zero_grad(set_to_none=False)
                loss.backward()
                if self.max_grad_norm is not None:
                    t.nn.utils.clip_grad_norm_(self._params, self.max_grad_norm)
                self.optimizer.step()
            self.draw_t.add_(1)
        return self.stats_t

    def learn(self, n_iterations: int):
        """collect(); update() n_iterations times -> stats_t of the last update."""
        for _ in range(int(n_iterations)):
            self.collector.collect()
            self.update()
        return self.stats_t
