"""Recurrent PPO on the device (include/glgym.h glgym_lstm_cell / glgym_lstm_cell_grad / glgym_seq_batch): what sb3-contrib's
RecurrentPPO with MlpLstmPolicy adds to gl_gym_amd.collector and gl_gym_amd.ppo -- a hidden state carried along the rollout and zeroed
where an episode starts, the rollout cut into sequences, truncated back-propagation through time over them.  The gate products
(x W_ih^T + b, h W_hh^T), autograd through them, the heads and the optimiser stay torch's; everything between the products is one launch
per LSTM and step.

    lstm = lambda: torch.nn.LSTM(env.obs_dim, 64).to(env.device)
    heads = RecurrentHeads(lstm(), pi_module, vf_module, log_std, lstm_vf=lstm())       # pi_module: [., 64] -> [., 6]; vf_module: [., 64] -> [., 1]
    col = RecurrentCollector(env, 64, heads, seq_len=16, gamma=0.9631)
    ppo = RecurrentPPO(col, torch.optim.Adam(heads.parameters(), lr=2e-5), n_epochs=8, n_minibatches=4)
    stats = ppo.learn(100)

A sequence is a fixed chunk of seq_len steps of one environment; it is not split where an episode starts inside it: the cell's `start`
select does there what sb3-contrib's per-step loop over the episode starts does, so no padding is needed and the gradients are those of
the same truncation length.  States are stored at chunk boundaries only ([T / L][B][H] per state tensor)."""
from __future__ import annotations

import ctypes as C
import math

from . import _lib as L
from .collector import RolloutCollector, TorchHeads
from .ppo import PpoLossBuffers, ppo_loss


def _torch():
    import torch
    return torch


def _stream(stream):
    return stream if stream is not None else C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _cell_call(lib, handle, stream, M, H, gx, gh, c_prev, start, h, c, act):
    a = L.make_plan_args(L.LstmCellArgs, M, H, gx.data_ptr(), gh.data_ptr(), c_prev.data_ptr(), None if start is None else start.data_ptr(),
                         h.data_ptr(), c.data_ptr(), None if act is None else act.data_ptr())
    L.check(lib.glgym_lstm_cell(handle, C.byref(a), stream), "glgym_lstm_cell")


def _make_cell_fn():
    t = _torch()

    class _LstmCell(t.autograd.Function):
        @staticmethod
        def forward(ctx, gx, gh, c_prev, start, handle, stream):
            M, H = c_prev.shape
            gx_c, gh_c, cp_c = gx.detach().contiguous(), gh.detach().contiguous(), c_prev.detach().contiguous()
            h, c = t.empty_like(cp_c), t.empty_like(cp_c)
            need = any(ctx.needs_input_grad[:3])
            act = t.empty(M, L.LSTM_N_ACT * H, dtype=t.float32, device=cp_c.device) if need else None
            _cell_call(L.load(), handle, stream, M, H, gx_c, gh_c, cp_c, start, h, c, act)
            if need:
                ctx.save_for_backward(act, cp_c)
                ctx.start, ctx.call = start, (handle, stream)
            ctx.set_materialize_grads(False)
            return h, c

        @staticmethod
        def backward(ctx, dh, dc):
            act, cp = ctx.saved_tensors
            M, H = cp.shape
            handle, stream = ctx.call
            dh = t.zeros_like(cp) if dh is None else dh.contiguous()
            dc = None if dc is None else dc.contiguous()
            d_gx, d_gh, d_cp = t.empty(M, 4 * H, dtype=t.float32, device=cp.device), t.empty(M, 4 * H, dtype=t.float32, device=cp.device), t.empty_like(cp)
            a = L.make_plan_args(L.LstmCellGradArgs, M, H, dh.data_ptr(), None if dc is None else dc.data_ptr(), act.data_ptr(), cp.data_ptr(),
                                 None if ctx.start is None else ctx.start.data_ptr(), d_gx.data_ptr(), d_gh.data_ptr(), d_cp.data_ptr())
            L.check(L.load().glgym_lstm_cell_grad(handle, C.byref(a), stream), "glgym_lstm_cell_grad")
            return d_gx, d_gh, d_cp, None, None, None

    return _LstmCell


_CELL_FN = None


def lstm_cell(gx, gh, c_prev, start=None, *, handle, stream=None):
    """One LSTM step behind the two gate products, differentiable: (h, c) [M, H] from gx [M, 4H] (x W_ih^T + b_ih + b_hh), gh [M, 4H]
    (h_prev W_hh^T, from the UNMASKED h_prev: the reset commutes with the product), c_prev [M, H] and start (uint8 [M], non-zero where the
    row begins an episode: gh and c_prev are then not read, by a select; or None).  Gates in torch's order i, f, g, o.  Forward is one
    glgym_lstm_cell call, which saves the five activations only when a gradient is required; backward is one glgym_lstm_cell_grad call.
    handle: the library handle of an environment (env._h); stream: a HIP stream as c_void_p (default: torch's current stream)."""
    global _CELL_FN
    t = _torch()
    if _CELL_FN is None:
        _CELL_FN = _make_cell_fn()
    if c_prev.dim() != 2 or gx.shape != (c_prev.shape[0], 4 * c_prev.shape[1]) or gh.shape != gx.shape:
        raise ValueError("lstm_cell: gx and gh must be [M, 4H] and c_prev [M, H]")
    for k, x in (("gx", gx), ("gh", gh), ("c_prev", c_prev)):
        if x.dtype != t.float32:
            raise ValueError(f"lstm_cell: {k} must be float32")
    if start is not None and not (start.dtype == t.uint8 and start.is_contiguous() and start.shape == (c_prev.shape[0],)):
        raise ValueError("lstm_cell: start must be contiguous uint8 [M]")
    return _CELL_FN.apply(gx, gh, c_prev, start, handle, _stream(stream))


def _check_lstm(name, m):
    t = _torch()
    if not isinstance(m, t.nn.LSTM):
        raise TypeError(f"RecurrentHeads: {name} must be a torch.nn.LSTM")
    if m.num_layers != 1:
        raise NotImplementedError(f"RecurrentHeads: {name} has {m.num_layers} layers; multi-layer LSTMs are out of scope")
    if m.bidirectional:
        raise NotImplementedError(f"RecurrentHeads: {name} is bidirectional; that is out of scope")
    if getattr(m, "proj_size", 0):
        raise NotImplementedError(f"RecurrentHeads: {name} has proj_size; projected LSTMs are out of scope")


class RecurrentHeads(TorchHeads):
    """A Gaussian policy and a value function behind single-layer torch.nn.LSTM modules (an sb3-contrib state dict's weight_ih_l0,
    weight_hh_l0, bias_ih_l0, bias_hh_l0 load as they are).  pi_module: [., H] -> [., 6] on the actor LSTM's output.  Three arrangements,
    sb3-contrib's: lstm_vf given -- separate LSTMs, vf_module: [., H_vf] -> [., 1] on the critic LSTM's output (the reference's);
    shared_lstm -- vf_module reads the actor LSTM's output, detached; neither -- vf_module reads the observation.
    Refused: more than one layer, bidirectional, proj_size."""

    def __init__(self, lstm_pi, pi_module, vf_module, log_std, lstm_vf=None, shared_lstm: bool = False):
        _check_lstm("lstm_pi", lstm_pi)
        if lstm_vf is not None:
            _check_lstm("lstm_vf", lstm_vf)
            if shared_lstm:
                raise ValueError("RecurrentHeads: shared_lstm with a critic LSTM of its own: choose one")
        super().__init__(pi_module, vf_module, log_std)
        self.arrangement = "separate" if lstm_vf is not None else "shared" if shared_lstm else "actor_only"
        self.lstms = {"pi": lstm_pi} if lstm_vf is None else {"pi": lstm_pi, "vf": lstm_vf}
        self.in_dim = int(lstm_pi.input_size)
        if lstm_vf is not None and int(lstm_vf.input_size) != self.in_dim:
            raise ValueError("RecurrentHeads: the two LSTMs must read the same observation")

    def parameters(self):
        """Everything an optimiser trains: the LSTMs, the two heads and log_std (if it is a parameter)."""
        t = self.torch
        out = [p for m in self.lstms.values() for p in m.parameters()]
        out += list(self.pi_module.parameters()) + list(self.vf_module.parameters())
        if isinstance(self._log_std_src, t.nn.Parameter):
            out.append(self._log_std_src)
        return out

    def bias(self, name):
        """b_ih + b_hh of an LSTM (differentiable), or None without biases: what the input product folds in."""
        m = self.lstms[name]
        return m.bias_ih_l0 + m.bias_hh_l0 if m.bias else None

    def latent_value(self, latent, obs):
        """What vf_module reads, given {name: LSTM output} and the observation rows behind it."""
        if self.arrangement == "separate":
            return latent["vf"]
        return latent["pi"].detach() if self.arrangement == "shared" else obs

    def sequence(self, name, obs, h0, c0, starts, handle, stream=None):
        """The LSTM `name` over a time-major minibatch: obs [L, S, D], h0 / c0 [S, H], starts uint8 [L, S] -> its outputs [L * S, H] in
        (l, s) order.  One input product over all L * S rows, then L times (h W_hh^T, lstm_cell)."""
        t, m = self.torch, self.lstms[name]
        Ln, S, D = obs.shape
        gx = t.nn.functional.linear(obs.reshape(Ln * S, D), m.weight_ih_l0, self.bias(name)).view(Ln, S, -1)
        h, c, hs = h0, c0, []
        for l in range(Ln):
            gh = t.nn.functional.linear(h, m.weight_hh_l0)
            h, c = lstm_cell(gx[l], gh, c, starts[l], handle=handle, stream=stream)
            hs.append(h)
        return t.cat(hs, dim=0)


class RecurrentCollector(RolloutCollector):
    """RolloutCollector with a recurrent policy (a RecurrentHeads): the same buffer plus buffer["lstm_states"] = {"pi": {"h", "c"}[, "vf":
    {"h", "c"}]}, each [T / L][B][H]: the carried state at the first step of every chunk of seq_len = L steps, stored raw (before the
    reset), as sb3-contrib stores it.  n_steps must be a multiple of seq_len.

    Per step: at a chunk's first step the carried states into their slot; per LSTM two products in torch (into tensors of the collector's
    own) and one glgym_lstm_cell launch with start = episode_starts[k] into the other half of a ping-pong pair; the heads on h; then what
    RolloutCollector does.  The last value takes one more critic-side cell step with start = the last dones, which does not advance the
    carried state.  The states carry over between collect() calls; reset() zeroes them.  collect() allocates nothing of its own and never
    synchronises; the heads' outputs come from torch's caching allocator."""

    def __init__(self, env, n_steps: int, heads, seq_len: int, gamma: float = 0.99, gae_lambda: float = 0.95, seed: int = 0):
        if not isinstance(heads, RecurrentHeads):
            raise TypeError("RecurrentCollector: heads must be a RecurrentHeads")
        if int(seq_len) < 1 or int(n_steps) % int(seq_len) != 0:
            raise ValueError("seq_len must be >= 1 and divide n_steps")
        if heads.in_dim != int(env.obs_dim):
            raise ValueError(f"the LSTMs read {heads.in_dim} columns, the observation has {int(env.obs_dim)}")
        super().__init__(env, n_steps, heads, gamma=gamma, gae_lambda=gae_lambda, seed=seed)
        t = self.torch
        self.L = int(seq_len)
        z = lambda *s: t.zeros(*s, dtype=t.float32, device=self.device)  # noqa: E731
        B, nC = self.B, self.T // self.L
        self.buffer["lstm_states"] = {}
        self._state, self._gates, self._bias = {}, {}, {}
        for name, m in heads.lstms.items():
            H = int(m.hidden_size)
            self.buffer["lstm_states"][name] = dict(h=z(nC, B, H), c=z(nC, B, H))
            self._state[name] = [dict(h=z(B, H), c=z(B, H)), dict(h=z(B, H), c=z(B, H))]       # the carried state is in [0] between calls
            self._gates[name] = (z(B, 4 * H), z(B, 4 * H))
            self._bias[name] = z(4 * H)
        self._cell = L.LstmCellArgs()
        self._cell.struct_size, self._cell.M = C.sizeof(L.LstmCellArgs), B

    def reset(self, seed=None):
        obs = super().reset(seed)
        for pair in self._state.values():
            for s in pair:
                s["h"].zero_()
                s["c"].zero_()
        return obs

    def _step_lstm(self, name, obs, src, dst, start):
        """One step of LSTM `name`: state src -> state dst (dicts of h, c)."""
        m, e, a = self.policy.lstms[name], self.env, self._cell
        t = self.torch
        gx, gh = self._gates[name]
        t.addmm(self._bias[name], obs, m.weight_ih_l0.t(), out=gx)
        t.mm(src["h"], m.weight_hh_l0.t(), out=gh)
        a.H, a.gx, a.gh, a.c_prev, a.start = int(m.hidden_size), gx.data_ptr(), gh.data_ptr(), src["c"].data_ptr(), start.data_ptr()
        a.h, a.c, a.act = dst["h"].data_ptr(), dst["c"].data_ptr(), None
        L.check(self._lib.glgym_lstm_cell(e._h, C.byref(a), e._stream()), "glgym_lstm_cell")

    def _heads(self, latent, obs):
        p = self.policy
        p.mean_t.copy_(p.pi_module(latent["pi"]).reshape(p.mean_t.shape))
        p.value_t.copy_(p.vf_module(p.latent_value(latent, obs)).reshape(p.value_t.shape))

    def collect(self, deterministic: bool = False):
        """-> the buffer of RolloutCollector.collect() plus lstm_states.  The same tensors at every call."""
        t, b, p = self.torch, self.buffer, self.policy
        if self.obs_t is None:
            self.reset()
        with t.no_grad():
            p.refresh()
            for name, m in p.lstms.items():
                if m.bias:
                    t.add(m.bias_ih_l0, m.bias_hh_l0, out=self._bias[name])
            b["episode_starts"][0].copy_(self._last_done)
            obs, cur = self.obs_t, 0
            for k in range(self.T):
                start = b["episode_starts"][k]
                if k % self.L == 0:
                    for name, pair in self._state.items():
                        slot = b["lstm_states"][name]
                        slot["h"][k // self.L].copy_(pair[cur]["h"])
                        slot["c"][k // self.L].copy_(pair[cur]["c"])
                for name, pair in self._state.items():
                    self._step_lstm(name, obs, pair[cur], pair[1 - cur], start)
                cur = 1 - cur
                self._heads({name: pair[cur]["h"] for name, pair in self._state.items()}, obs)
                self.ac_rows(obs, k, slot=k, deterministic=deterministic)
                obs, rew, done = self.env.step_tensor(self.action_env_t)[:3]
                b["rewards"][k].copy_(rew)
                b["dones"][k].copy_(done)
                if k + 1 < self.T:
                    b["episode_starts"][k + 1].copy_(done)
            self.obs_t = obs
            self._last_done.copy_(b["dones"][self.T - 1])
            # the value of the final observation: one more cell step on the critic's side into the idle half, the carried state stays
            crit = {"separate": "vf", "shared": "pi"}.get(p.arrangement)
            if crit is not None:
                pair = self._state[crit]
                self._step_lstm(crit, obs, pair[cur], pair[1 - cur], self._last_done)
                p.value_t.copy_(p.vf_module(pair[1 - cur]["h"]).reshape(p.value_t.shape))
            else:
                p.value_t.copy_(p.vf_module(obs).reshape(p.value_t.shape))
            self.ac_rows(obs, self.T, value_only=True, value_ptr=b["last_values"].data_ptr())
            e = self.env
            L.check(self._lib.glgym_gae(e._h, C.byref(self._gae), e._stream()), "glgym_gae")
            if cur:                                              # an odd n_steps: back into [0], so that a captured collect() can replay
                for pair in self._state.values():
                    pair[0]["h"].copy_(pair[1]["h"])
                    pair[0]["c"].copy_(pair[1]["c"])
            self.draw_base_t.add_(1)
        return b


class RecurrentPPO:
    """The optimiser phase of recurrent PPO over a RecurrentCollector's buffer: PPO over minibatches of whole sequences.  Either
    n_minibatches or batch_size, both in SEQUENCES of collector.L steps (a minibatch of S sequences has L * S rows); the last minibatch is
    smaller when (T / L) * B is no multiple of it.

    update(): for every epoch, for every minibatch: glgym_seq_batch (time-major gather, the states at the sequences' first steps, advantage
    statistics) -> per LSTM one input product over all L * S rows, then L times (h W_hh^T, lstm_cell) -> the heads on the stacked
    [L * S, H] -> ppo_loss on the L * S flat rows -> backward -> clip_grad_norm_ -> optimizer.step; then the draw word + 1.  Returns stats_t
    [n_epochs, n_minibatches, 8] (PPO.STATS; float64, on the device).  Never synchronises.
    Out of scope, refused: target_kl, learning-rate and clip schedules (as PPO)."""

    STATS = L.PPO_STATS

    def __init__(self, collector, optimizer, n_epochs: int = 8, n_minibatches: int = 4, batch_size=None, clip_range: float = 0.2,
                 clip_range_vf=None, normalize_advantage: bool = True, ent_coef: float = 0.0, vf_coef: float = 0.5, max_grad_norm=0.5,
                 seed: int = 0, target_kl=None):
        t = self.torch = _torch()
        if target_kl is not None:
            raise NotImplementedError("RecurrentPPO: target_kl is out of scope: it needs a host decision per minibatch")
        if callable(clip_range) or callable(clip_range_vf):
            raise NotImplementedError("RecurrentPPO: clip schedules are out of scope (a clip range is a number)")
        if not (float(clip_range) > 0.0 and math.isfinite(float(clip_range))):
            raise ValueError("clip_range must be > 0 and finite")
        if clip_range_vf is not None and not float(clip_range_vf) > 0.0:
            raise ValueError("clip_range_vf must be > 0, or None")
        if not hasattr(collector, "L") or not isinstance(getattr(collector, "policy", None), RecurrentHeads):
            raise TypeError("RecurrentPPO: collector must be a RecurrentCollector")
        self.collector, self.optimizer = collector, optimizer
        self.n_epochs, self.seed = int(n_epochs), int(seed)
        self.clip_range, self.clip_range_vf = float(clip_range), None if clip_range_vf is None else float(clip_range_vf)
        self.normalize_advantage, self.ent_coef, self.vf_coef, self.max_grad_norm = bool(normalize_advantage), float(ent_coef), float(vf_coef), max_grad_norm
        col = collector
        Ln, T, B, D = col.L, col.T, col.B, col.D
        N = self.N = (T // Ln) * B
        S = self.batch_size = int(batch_size) if batch_size is not None else -(-N // int(n_minibatches))
        if self.n_epochs < 1 or not 1 <= S <= N:
            raise ValueError("n_epochs must be >= 1 and the minibatch size in 1 .. (n_steps / seq_len) * num_envs sequences")
        self.sizes = [min(S, N - o) for o in range(0, N, S)]
        if self.normalize_advantage and Ln * min(self.sizes) < 2:
            raise ValueError("normalize_advantage needs at least 2 rows in every minibatch (the last one would have 1)")
        dev = col.device
        z = lambda *s, dtype=t.float32: t.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        M = Ln * S
        self.mb = dict(observations=z(M, D), actions=z(M, L.NU), log_probs=z(M), advantages=z(M), returns=z(M), values=z(M),
                       starts=z(M, dtype=t.uint8))
        self.mb_states = {name: dict(h=z(S, st["h"].shape[-1]), c=z(S, st["c"].shape[-1])) for name, st in col.buffer["lstm_states"].items()}
        self.adv_stats_t = z(2, dtype=t.float64)
        self.batch_ws_t = z(L.SEQ_BATCH_WS_BYTES // 8, dtype=t.float64)
        self.loss_buffers = PpoLossBuffers(M, dev)
        self.stats_t = z(self.n_epochs, len(self.sizes), 8, dtype=t.float64)
        self.draw_t = z(1, dtype=t.int64)                     # device word added to the draw index: + 1 per epoch
        self._lib = L.load()
        b = col.buffer
        states = [(b["lstm_states"][n][k], self.mb_states[n][k]) for n in self.mb_states for k in ("h", "c")]
        dims = [int(s.shape[-1]) for s, _ in states] + [0] * (L.SEQ_MAX_STATE - len(states))
        src = [s.data_ptr() for s, _ in states] + [None] * (L.SEQ_MAX_STATE - len(states))
        dst = [o.data_ptr() for _, o in states] + [None] * (L.SEQ_MAX_STATE - len(states))
        self._batch_args, self._views = [], []
        for i, s in enumerate(self.sizes):
            self._batch_args.append(L.make_plan_args(
                L.SeqBatchArgs, T, B, Ln, s, i * S, D, len(states), (C.c_int32 * 4)(*dims), self.seed & (2 ** 64 - 1), 0, self.draw_t.data_ptr(),
                b["observations"].data_ptr(), b["actions"].data_ptr(), b["log_probs"].data_ptr(), b["advantages"].data_ptr(),
                b["returns"].data_ptr(), b["values"].data_ptr(), b["episode_starts"].data_ptr(), (C.c_void_p * 4)(*src),
                self.mb["observations"].data_ptr(), self.mb["actions"].data_ptr(), self.mb["log_probs"].data_ptr(),
                self.mb["advantages"].data_ptr(), self.mb["returns"].data_ptr(), self.mb["values"].data_ptr(), self.mb["starts"].data_ptr(),
                (C.c_void_p * 4)(*dst), None, self.adv_stats_t.data_ptr() if self.normalize_advantage else None,
                self.batch_ws_t.data_ptr() if self.normalize_advantage else None, L.SEQ_BATCH_WS_BYTES))
            v = {k: x[:Ln * s] for k, x in self.mb.items()}                                # flat (l, s) rows: what ppo_loss reads
            v["adv_stats"] = self.adv_stats_t if self.normalize_advantage else None
            if self.clip_range_vf is None:
                v["values"] = None
            v["seq_observations"] = v["observations"].view(Ln, s, D)
            v["seq_starts"] = v["starts"].view(Ln, s)
            v["states"] = {n: {k: x[:s] for k, x in st.items()} for n, st in self.mb_states.items()}
            self._views.append(v)
        self._params = [q for g in optimizer.param_groups for q in g["params"]]

    def batch(self, i: int):
        """Gather minibatch i of the present epoch's permutation -> its views (the same tensors at every call): the flat [L * S] rows of
        PPO.batch plus "seq_observations" [L, S, D], "seq_starts" [L, S] and "states" {name: {"h", "c"} [S, H]}."""
        e = self.collector.env
        L.check(self._lib.glgym_seq_batch(e._h, C.byref(self._batch_args[i]), e._stream()), "glgym_seq_batch")
        return self._views[i]

    def evaluate(self, mb):
        """The heads on a gathered minibatch, with grad -> mean [L * S, 6], value [L * S, 1]."""
        p, e = self.collector.policy, self.collector.env
        latent = {n: p.sequence(n, mb["seq_observations"], mb["states"][n]["h"], mb["states"][n]["c"], mb["seq_starts"], e._h, e._stream())
                  for n in p.lstms}
        return p.pi_module(latent["pi"]), p.vf_module(p.latent_value(latent, mb["observations"]))

    def update(self):
        t, e, p = self.torch, self.collector.env, self.collector.policy
        for epoch in range(self.n_epochs):
            for i in range(len(self.sizes)):
                mb = self.batch(i)
                mean, value = self.evaluate(mb)
                loss = ppo_loss(mean, value, p._log_std_src, mb, handle=e._h, stream=e._stream(), clip_range=self.clip_range,
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
