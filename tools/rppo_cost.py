#!/usr/bin/env python3
"""What recurrent PPO costs, measured on the GPU -> profiles/rppo_cost.txt.

    python tools/rppo_cost.py [--parent-pkg DIR] [--out profiles/rppo_cost.txt]

The set-up of tools/ppo_update_cost.py: fp32, ls5, VecNormalizeGPU(VecMonitorGPU(TomatoVecEnv)), 65 536 environments x 64 steps, sequences
of 16 steps, the nets of examples/train_recurrent_ppo.py (two LSTMs of 64, pi 2 x 256 and vf 2 x 128, silu), 4 minibatches; device
events, warmed up, five alternating repeats with their spreads, no profiler.
(1) Recorded, no bar: glgym_lstm_cell (with act) + glgym_lstm_cell_grad at 1 M rows x 64 units against (i) the same step as torch ops with
    autograd (mask, chunk, sigmoid / tanh, mul / add) and (ii) the pointwise path of torch.nn.LSTMCell (aten::_thnn_fused_lstm_cell and its
    backward, with the reset as two products in front of it, and alone), each as achieved bytes per second of the bytes the library's two calls move (64 + 68 bytes per (row, unit)) against the
    6.3 TB/s a streaming kernel reaches on an MI355X.  If a torch form is faster the report says so.
(2) Recorded: glgym_seq_batch for one epoch against index gathers in torch of the same sequences.
(3) Recorded: one RecurrentPPO.update() epoch and one RecurrentCollector.collect() against a plain-torch restatement of the same loops
    (below; not part of the package), and the share of each that the gate products and the heads are (timed on their own, the update's
    forward and backward).
(4) Requirement, ratio <= 1.05: RolloutCollector.collect(), PPO.update() and 64 plain step_tensor calls against the parent commit's build.
--parent-pkg DIR: the greenlight-gym2_amd directory of a checkout of the PARENT commit with its library built; the other sides of (4) run
in child processes on that build.  Without it they run on this build, the report says so and gives no verdict.
No fallback: without a GPU this fails."""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from collect_cost import B0, GAMMA, N_SAMPLES, N_WARM, T0, alternate, setup, spread, step_loop, timed  # noqa: E402
from ppo_update_cost import nets as ppo_nets  # noqa: E402

SEQ, LSTM, PI_W, VF_W, N_MB, CLIP, LAM = 16, 64, 256, 128, 4, 0.2, 0.9167
CELL_ROWS = 1 << 20
FWD_BYTES, BWD_BYTES = 64, 68                                 # per (row, unit): 9 floats in, 2 + 5 out; 5 + 3 in (act; dh, dc, c_prev), 9 out


def mlp(torch, n_in, width, n_out, dev):
    lin, act = torch.nn.Linear, torch.nn.SiLU
    return torch.nn.Sequential(lin(n_in, width), act(), lin(width, width), act(), lin(width, n_out)).to(dev)


def torch_cell(torch, gx, gh, c_prev, start):
    """The step as torch ops, sb3-contrib's way: the mask as a product."""
    keep = (1.0 - start.to(gx.dtype)).unsqueeze(1)
    i, f, g, o = (gx + keep * gh).chunk(4, dim=1)
    c = torch.sigmoid(f) * (keep * c_prev) + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c), c


def recurrent_stack(torch, base, env, B, T):
    from gl_gym_amd import RecurrentCollector, RecurrentHeads, RecurrentPPO
    D, dev = base.obs_dim, base.device
    torch.manual_seed(0)
    lstm = lambda: torch.nn.LSTM(D, LSTM).to(dev)  # noqa: E731
    log_std = torch.nn.Parameter(torch.zeros(6, device=dev))
    heads = RecurrentHeads(lstm(), mlp(torch, LSTM, PI_W, 6, dev), mlp(torch, LSTM, VF_W, 1, dev), log_std, lstm_vf=lstm())
    col = RecurrentCollector(env, T, heads, seq_len=SEQ, gamma=GAMMA, gae_lambda=LAM, seed=0)
    col.reset(seed=666)
    col.collect()
    opt = torch.optim.Adam(heads.parameters(), lr=2e-5, amsgrad=True)
    ppo = RecurrentPPO(col, opt, n_epochs=1, n_minibatches=N_MB, clip_range=CLIP, ent_coef=0.05434, vf_coef=0.8225, max_grad_norm=0.3, seed=0)
    return heads, col, opt, ppo


class TorchRecurrent:
    """collect() and one update epoch restated in plain torch on the same modules: the cell as torch ops, the sample and the
    log-probability as in examples/device_rollout.py, GAE as its backward loop, minibatches of sequences by torch.randperm and index
    gathers, the loss chain of examples/collect_rollouts.py."""

    def __init__(self, torch, env, heads, B, T, D):
        self.torch, self.env, self.heads, self.B, self.T = torch, env, heads, B, T
        dev = env.device
        e = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
        self.buf = dict(obs=e(T, B, D), act=e(T, B, 6), rew=e(T, B), done=e(T, B), val=e(T, B), logp=e(T, B), start=e(T, B))
        self.state = {n: (torch.zeros(B, LSTM, device=dev), torch.zeros(B, LSTM, device=dev)) for n in heads.lstms}
        self.stored = {n: (e(T // SEQ, B, LSTM), e(T // SEQ, B, LSTM)) for n in heads.lstms}
        self.last_done = torch.ones(B, device=dev)
        self.adv = e(T, B)
        self.obs = env.reset_tensor()

    def step_lstms(self, obs, start, state):
        torch, out = self.torch, {}
        for n, m in self.heads.lstms.items():
            h, c = state[n]
            gx = torch.nn.functional.linear(obs, m.weight_ih_l0, m.bias_ih_l0 + m.bias_hh_l0)
            out[n] = torch_cell(torch, gx, torch.nn.functional.linear(h, m.weight_hh_l0), c, start)
        return out

    def collect(self):
        torch, buf, p = self.torch, self.buf, self.heads
        with torch.no_grad():
            obs, log_std = self.obs, p._log_std_src
            start = self.last_done
            for t in range(self.T):
                if t % SEQ == 0:
                    for n in self.state:
                        self.stored[n][0][t // SEQ].copy_(self.state[n][0]); self.stored[n][1][t // SEQ].copy_(self.state[n][1])
                self.state = self.step_lstms(obs, start, self.state)
                mean, value = p.pi_module(self.state["pi"][0]), p.vf_module(self.state["vf"][0]).squeeze(-1)
                noise = torch.randn_like(mean)
                act = mean + noise * log_std.exp()
                buf["obs"][t].copy_(obs); buf["act"][t].copy_(act); buf["val"][t].copy_(value); buf["start"][t].copy_(start)
                buf["logp"][t].copy_((-0.5 * noise.pow(2) - log_std - 0.9189385).sum(-1))
                obs, rew, done, _ = self.env.step_tensor(act.clamp(-1.0, 1.0))
                buf["rew"][t].copy_(rew); buf["done"][t].copy_(done)
                start = buf["done"][t]
            self.obs, self.last_done = obs, start.clone()
            last_v = p.vf_module(self.step_lstms(obs, start, self.state)["vf"][0]).squeeze(-1)
            adv = torch.zeros(self.B, device=obs.device)
            for t in reversed(range(self.T)):
                nonterm = 1.0 - buf["done"][t]
                delta = buf["rew"][t] + GAMMA * last_v * nonterm - buf["val"][t]
                adv = delta + GAMMA * LAM * nonterm * adv
                self.adv[t] = adv; last_v = buf["val"][t]

    def gather(self, idx):
        """Sequences idx of the [T][B] buffer, time-major, by index gathers."""
        torch, buf, B, T = self.torch, self.buf, self.B, self.T
        rows = ((idx // B) * SEQ)[None, :] * B + torch.arange(SEQ, device=idx.device)[:, None] * B + (idx % B)[None, :]
        flat = rows.reshape(-1)
        out = {k: buf[k].reshape(T * B, -1)[flat] for k in ("obs", "act")}
        out.update({k: buf[k].reshape(-1)[flat] for k in ("logp", "val", "start")})
        out["adv"], out["ret"] = self.adv.reshape(-1)[flat], (self.adv + buf["val"]).reshape(-1)[flat]
        out["states"] = {n: (s[0].reshape(-1, LSTM)[idx], s[1].reshape(-1, LSTM)[idx]) for n, s in self.stored.items()}
        return out

    def update(self, opt, params):
        torch, p, N = self.torch, self.heads, (self.T // SEQ) * self.B
        for idx in torch.randperm(N, device=self.obs.device).chunk(N_MB):
            mb, S = self.gather(idx), len(idx)
            latent = {}
            for n, m in p.lstms.items():
                gx = torch.nn.functional.linear(mb["obs"], m.weight_ih_l0, m.bias_ih_l0 + m.bias_hh_l0).view(SEQ, S, -1)
                (h, c), hs, st = mb["states"][n], [], mb["start"].view(SEQ, S)
                for l in range(SEQ):
                    h, c = torch_cell(torch, gx[l], torch.nn.functional.linear(h, m.weight_hh_l0), c, st[l])
                    hs.append(h)
                latent[n] = torch.cat(hs)
            mean, value, log_std = p.pi_module(latent["pi"]), p.vf_module(latent["vf"]).squeeze(-1), p._log_std_src
            noise = (mb["act"] - mean) / log_std.exp()
            logp = (-0.5 * noise.pow(2) - log_std - 0.9189385).sum(-1)
            ratio = (logp - mb["logp"]).exp()
            a = (mb["adv"] - mb["adv"].mean()) / (mb["adv"].std() + 1e-8)
            loss = -torch.min(ratio * a, ratio.clamp(1 - CLIP, 1 + CLIP) * a).mean() + 0.8225 * (mb["ret"] - value).pow(2).mean() \
                - 0.05434 * (0.5 + 0.9189385 + log_std).sum()
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, 0.3)
            opt.step()


def parent_stack(pkg, B, T):
    torch, make = setup(pkg)
    from gl_gym_amd import PPO, RolloutCollector, TorchHeads
    base, env = make(B)
    pi, vf, log_std = ppo_nets(torch, base.obs_dim, base.device)
    col = RolloutCollector(env, T, TorchHeads(pi, vf, log_std), gamma=GAMMA, gae_lambda=LAM, seed=0)
    col.reset(seed=666)
    col.collect()
    opt = torch.optim.Adam(list(pi.parameters()) + list(vf.parameters()) + [log_std], lr=3e-4)
    ppo = PPO(col, opt, n_epochs=1, n_minibatches=N_MB, clip_range=CLIP, ent_coef=0.0, vf_coef=0.5, max_grad_norm=None, seed=0)
    return torch, base, col, ppo


def untouched(kind, torch, base, col, ppo, B, T):
    return {"collector": col.collect, "update": ppo.update, "steps": step_loop(torch, base, B, T)}[kind]


def worker(pkg, kind, B, T):
    """RolloutCollector.collect() ("collector"), PPO.update() ("update") or a plain step_tensor loop ("steps") on the build under pkg;
    answers "time" on stdin with one sample."""
    torch, base, col, ppo = parent_stack(pkg, B, T)
    run = untouched(kind, torch, base, col, ppo, B, T)
    for _ in range(N_WARM):
        timed(torch, run)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "time":
            break
        print(f"ms {timed(torch, run):.6f}", flush=True)


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
                timed(torch, self.run)

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
            self.child.wait(timeout=120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", default=None, help="built greenlight-gym2_amd directory of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rppo_cost.txt"))
    ap.add_argument("--n-envs", type=int, default=B0)
    ap.add_argument("--n-steps", type=int, default=T0)
    ap.add_argument("--cell-rows", type=int, default=CELL_ROWS)
    ap.add_argument("--worker", nargs=4, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker[0]), args.worker[1], int(args.worker[2]), int(args.worker[3]))
    B, T = args.n_envs, args.n_steps
    torch, base, col0, ppo0 = parent_stack(ROOT / "greenlight-gym2_amd", B, T)
    if not torch.cuda.is_available():
        sys.exit("rppo_cost.py needs a GPU (no fallback)")
    import ctypes as C
    from gl_gym_amd import _lib as L
    dev = base.device
    where = ("child processes on the parent commit's build (--parent-pkg)" if args.parent_pkg else "THIS build (no --parent-pkg given: no verdict)")
    lines = [f"recurrent PPO on the device: cost on {torch.cuda.get_device_name(0)} (tools/rppo_cost.py)",
             f"fp32 ls5-128, VecNormalizeGPU(VecMonitorGPU(TomatoVecEnv)), {B} environments x {T} steps, sequences of {SEQ}, two LSTMs of {LSTM}, pi 2 x "
             f"{PI_W} and vf 2 x {VF_W} (silu), {N_MB} minibatches; device events, {N_WARM} warm-up windows, {N_SAMPLES} alternating repeats; spread = "
             f"(max - min) / median of a side's repeats; the other side of (4) runs in {where}", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731
    fmt = lambda v, k=1.0, d=3: " ".join(f"{x * k:.{d}f}" for x in v)  # noqa: E731
    med = statistics.median
    lib, h_, st_ = col0.env._lib, col0.env._h, col0.env._stream
    ok = True

    # ---- (1) the cell, forward + backward ---------------------------------------------------------------------------------------------------
    M, H = args.cell_rows, LSTM
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)  # noqa: E731
    gx, gh, cp, dh, dc = r(M, 4 * H), r(M, 4 * H), r(M, H), r(M, H), r(M, H)
    start = (torch.rand(M, device=dev, generator=g) < 0.05).to(torch.uint8)
    e = lambda *s: torch.empty(*s, device=dev)  # noqa: E731
    ho, co, act, d_gx, d_gh, d_cp = e(M, H), e(M, H), e(M, 5 * H), e(M, 4 * H), e(M, 4 * H), e(M, H)
    fa = L.make_plan_args(L.LstmCellArgs, M, H, gx.data_ptr(), gh.data_ptr(), cp.data_ptr(), start.data_ptr(), ho.data_ptr(), co.data_ptr(), act.data_ptr())
    ba = L.make_plan_args(L.LstmCellGradArgs, M, H, dh.data_ptr(), dc.data_ptr(), act.data_ptr(), cp.data_ptr(), start.data_ptr(), d_gx.data_ptr(),
                          d_gh.data_ptr(), d_cp.data_ptr())

    def hip_cell():
        L.check(lib.glgym_lstm_cell(h_, C.byref(fa), st_()), "glgym_lstm_cell")
        L.check(lib.glgym_lstm_cell_grad(h_, C.byref(ba), st_()), "glgym_lstm_cell_grad")

    leaves = [x.clone().requires_grad_() for x in (gx, gh, cp)]

    def th_cell():
        hh, cc = torch_cell(torch, *leaves, start)
        return torch.autograd.grad([hh, cc], leaves, [dh, dc])

    keep = (1.0 - start.float()).unsqueeze(1)
    fused = torch.ops.aten._thnn_fused_lstm_cell          # what torch.nn.LSTMCell dispatches to on the device behind its two products

    def fused_cell():
        """torch.nn.LSTMCell's pointwise path with the reset as sb3-contrib has it: the state times 1 - start."""
        hh, cc, _ = fused(leaves[0], keep * leaves[1], keep * leaves[2])
        return torch.autograd.grad([hh, cc], leaves, [dh, dc])

    def fused_bare():
        """The same path alone: no reset at all."""
        hh, cc, _ = fused(*leaves)
        return torch.autograd.grad([hh, cc], leaves, [dh, dc])

    hip_cell()
    ref = th_cell()
    diff = float((ref[0] - d_gx).abs().max() / ref[0].abs().max())
    diff_f = float((fused_cell()[0] - d_gx).abs().max() / ref[0].abs().max())
    x, y = alternate(torch, hip_cell, lambda: timed(torch, th_cell, 3), 3)
    x2, z = alternate(torch, hip_cell, lambda: timed(torch, fused_cell, 3), 3)
    x3, w = alternate(torch, hip_cell, lambda: timed(torch, fused_bare, 3), 3)
    byts = M * H * (FWD_BYTES + BWD_BYTES)
    tb = lambda ms: byts / (ms * 1e-3) / 1e12  # noqa: E731
    say(f"(1) glgym_lstm_cell (with act) + glgym_lstm_cell_grad, {M} rows x {H}, us        : {fmt(x, 1e3, 1)}   median {med(x) * 1e3:.1f}")
    say(f"    the same step as torch ops with autograd, forward + backward, us              : {fmt(y, 1e3, 1)}   median {med(y) * 1e3:.1f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; {FWD_BYTES} + {BWD_BYTES} bytes per (row, unit): library {tb(med(x)):.2f} TB/s, torch ops "
        f"{tb(med(y)):.2f} TB/s of the same bytes (a streaming kernel reaches about 6.3 TB/s); ratio library / torch ops = {med(x) / med(y):.4f}; "
        f"largest difference of d_gx / largest gradient {diff:.2e}")
    say(f"    torch.nn.LSTMCell's pointwise path (aten::_thnn_fused_lstm_cell and its backward, float32 gates) with the reset as two products "
        f"in front of it, us : {fmt(z, 1e3, 1)}   median {med(z) * 1e3:.1f}   (library alongside: median {med(x2) * 1e3:.1f})")
    say(f"    the same path alone, no reset, us                                             : {fmt(w, 1e3, 1)}   median {med(w) * 1e3:.1f}   "
        f"(library alongside: median {med(x3) * 1e3:.1f})")
    say(f"    spreads {spread(z) * 100:.1f} % / {spread(w) * 100:.1f} %; {tb(med(z)):.2f} / {tb(med(w)):.2f} TB/s of the library's bytes; ratio library / fused with "
        f"reset = {med(x2) / med(z):.4f}, library / fused alone = {med(x3) / med(w):.4f}; largest difference of d_gx (fused with reset) / largest gradient {diff_f:.2e}")
    for name, r_ in (("with the reset as products", med(x2) / med(z)), ("alone (which does not reset the state)", med(x3) / med(w))):
        if r_ > 1.0:
            say(f"    torch's fused pointwise path {name} is FASTER than the library's two calls: ratio {r_:.4f}")
    say()
    del gx, gh, cp, dh, dc, ho, co, act, d_gx, d_gh, d_cp, leaves, ref
    torch.cuda.empty_cache()

    # ---- the recurrent stack on an environment of its own ------------------------------------------------------------------------------------
    _, make = setup(ROOT / "greenlight-gym2_amd")
    rbase, renv = make(B)
    heads, col, opt, ppo = recurrent_stack(torch, rbase, renv, B, T)
    tbase, tenv = make(B)
    tr = TorchRecurrent(torch, tenv, heads, B, T, rbase.obs_dim)
    tr.collect()
    params = heads.parameters()

    # ---- (2) sequence minibatches, one epoch ------------------------------------------------------------------------------------------------
    N = (T // SEQ) * B

    def hip_epoch():
        for i in range(len(ppo.sizes)):
            ppo.batch(i)

    def th_epoch():
        for idx in torch.randperm(N, device=dev).chunk(N_MB):
            tr.gather(idx)

    timed(torch, th_epoch)                                       # the torch sides of (2) and (3) warm up once, as the library's do
    x, y = alternate(torch, hip_epoch, lambda: timed(torch, th_epoch, 3), 3)
    say(f"(2) glgym_seq_batch, one epoch = {N_MB} calls ({N} sequences of {SEQ}, states, statistics), us : {fmt(x, 1e3, 1)}   median {med(x) * 1e3:.1f}")
    say(f"    torch.randperm + index gathers of the same sequences, us                      : {fmt(y, 1e3, 1)}   median {med(y) * 1e3:.1f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio kernel / torch = {med(x) / med(y):.4f} (recorded, no bar)")
    say()

    # ---- (3) update and collect against the torch restatement; the products' share ---------------------------------------------------------
    S = ppo.sizes[0]
    mb = ppo.batch(0)

    M_mb = SEQ * S
    g_all, g_step = torch.ones(M_mb, 4 * LSTM, device=dev), torch.ones(S, 4 * LSTM, device=dev)
    g_pi, g_vf = torch.ones(M_mb, 6, device=dev), torch.ones(M_mb, 1, device=dev)
    lat = torch.zeros(M_mb, LSTM, device=dev, requires_grad=True)
    h_in = torch.zeros(S, LSTM, device=dev, requires_grad=True)

    def products_update(backward=True):
        """What stays torch's in one minibatch, on its own: the gate products and the heads, forward and (backward=True) backward."""
        with torch.set_grad_enabled(backward):
            outs, grads = [], []
            for m in heads.lstms.values():
                outs.append(torch.nn.functional.linear(mb["observations"], m.weight_ih_l0, m.bias_ih_l0))
                grads.append(g_all)
                for _ in range(SEQ):
                    outs.append(torch.nn.functional.linear(h_in, m.weight_hh_l0))
                    grads.append(g_step)
            outs += [heads.pi_module(lat), heads.vf_module(lat)]
            grads += [g_pi, g_vf]
            if backward:
                torch.autograd.backward(outs, grads)

    obs_b = col.obs_t

    def products_collect():
        with torch.no_grad():
            hh = torch.zeros(B, LSTM, device=dev)
            for _ in range(T):
                for m in heads.lstms.values():
                    torch.nn.functional.linear(obs_b, m.weight_ih_l0, m.bias_ih_l0), torch.nn.functional.linear(hh, m.weight_hh_l0)
                heads.pi_module(hh), heads.vf_module(hh)

    timed(torch, lambda: tr.update(opt, params))
    x, y = alternate(torch, ppo.update, lambda: timed(torch, lambda: tr.update(opt, params)))
    timed(torch, products_update)
    pu = med([timed(torch, products_update) for _ in range(N_SAMPLES)]) * len(ppo.sizes)
    pf = med([timed(torch, lambda: products_update(False)) for _ in range(N_SAMPLES)]) * len(ppo.sizes)
    say(f"(3) RecurrentPPO.update(), one epoch x {N_MB} minibatches of {S} sequences, ms        : {fmt(x)}   median {med(x):.3f}")
    say(f"    the plain-torch restatement of the same epoch, ms                             : {fmt(y)}   median {med(y):.3f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio package / torch = {med(x) / med(y):.4f}; the gate products and the heads "
        f"on their own, forward + backward, {pu:.3f} ms an epoch (forward {pf:.3f}) = {pu / med(x) * 100:.0f} % of the package's epoch")
    x, y = alternate(torch, col.collect, lambda: timed(torch, tr.collect))
    pc = med([timed(torch, products_collect) for _ in range(N_SAMPLES)])
    sl = med([timed(torch, step_loop(torch, rbase, B, T)) for _ in range(3)])
    col.reset(seed=666)
    say(f"    RecurrentCollector.collect(), ms                                              : {fmt(x)}   median {med(x):.3f}")
    say(f"    the plain-torch restatement of the same rollout, ms                           : {fmt(y)}   median {med(y):.3f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio package / torch = {med(x) / med(y):.4f}; the gate products and the heads "
        f"{pc:.3f} ms = {pc / med(x) * 100:.0f} %, {T} plain env-steps {sl:.3f} ms = {sl / med(x) * 100:.0f} % of the package's collect()")
    say()
    tbase.close()
    rbase.close()

    # ---- (4) the untouched paths ----------------------------------------------------------------------------------------------------------
    for name, kind in ((f"RolloutCollector.collect() ({B} x {T})", "collector"), (f"PPO.update(), one epoch x {N_MB} minibatches", "update"),
                       (f"a seeded reset and {T} plain step_tensor calls", "steps")):
        mine = untouched(kind, torch, base, col0, ppo0, B, T)
        other = Other(torch, args.parent_pkg, kind, B, T, mine)
        x, y = alternate(torch, mine, other)
        other.close()
        r_d = med(x) / med(y)
        say(f"(4) {name}, this build / the parent commit's, ms: {fmt(x)}  /  {fmt(y)}")
        say(f"    medians {med(x):.3f} / {med(y):.3f} ms; spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio = {r_d:.4f}"
            + (f"   (requirement <= 1.05: {'met' if r_d <= 1.05 else 'NOT MET'})" if args.parent_pkg else ""))
        ok = ok and r_d <= 1.05
    base.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if (not args.parent_pkg or ok) else 1


if __name__ == "__main__":
    sys.exit(main())
