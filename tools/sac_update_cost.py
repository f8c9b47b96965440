#!/usr/bin/env python3
"""What soft actor-critic on the device costs, measured on the GPU -> profiles/sac_update_cost.txt.

    python tools/sac_update_cost.py [--parent-pkg DIR] [--out profiles/sac_update_cost.txt]

The set-up of tools/ppo_update_cost.py: fp32, ls5, VecNormalizeGPU(VecMonitorGPU(TomatoVecEnv)), 65 536 environments, a minibatch of
1 048 576 rows, the nets of examples/train_sac.py (actor 3 x 256, critics 3 x 512, SiLU); device events, warmed up, five alternating
repeats with their spreads, no profiler.
(a) Requirement, not slower: squashed_sample's two launches (glgym_sac_rows + glgym_sac_rows_grad) against torch's rsample / tanh /
    log_prob / correction chain, forward plus backward through autograd, on the same actor outputs.
(b) Requirement, not slower: glgym_sac_loss in both stages (two calls) against the two torch loss chains, forward plus backward.
(c) Recorded: glgym_sac_batch against torch.randint plus the five index gathers on the same ring.
(d) Recorded: glgym_polyak against torch._foreach_mul_ + torch._foreach_add_ on the example's critics.
(e) Requirement, ratio <= 1.05: RolloutCollector.collect(), PPO.update() and a plain 64-step step_tensor loop against the parent commit's build.
(f) Recorded: one SAC.update gradient step against the same step written in torch ops, and the share of it that is the networks (their
    GEMMs, autograd through them and the optimisers: the torch step with every loss replaced by a plain sum).
--parent-pkg DIR: the greenlight-gym2_amd directory of a checkout of the PARENT commit with its library built; the other side of (e) runs
in child processes on that build.  Without it it runs on this build, the report says so and gives no verdict.
No fallback: without a GPU this fails."""
import argparse
import ctypes as C
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "examples"))
from collect_cost import B0, N_SAMPLES, N_WARM, T0, alternate, setup, spread, step_loop, timed  # noqa: E402
from ppo_update_cost import N_MB, CLIP, stack  # noqa: E402

M0, N_SLOTS, GAMMA, TAU, TE = 1 << 20, 4, 0.9631, 0.0135, -6.0
STREAM_TBS = 6.3


def worker(pkg, kind, B, T):
    """RolloutCollector.collect() ("collector"), PPO.update() of one epoch ("ppo") or a plain step_tensor loop ("steps") on the build under
    pkg; answers "time" on stdin with one sample."""
    torch, base, col, pi, vf, log_std, opt = stack(pkg, B, T)
    run = runner(torch, kind, base, col, opt, B, T)
    for _ in range(N_WARM):
        timed(torch, run)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() != "time":
            break
        print(f"ms {timed(torch, run):.6f}", flush=True)


def runner(torch, kind, base, col, opt, B, T):
    if kind == "collector":
        return col.collect
    if kind == "steps":
        return step_loop(torch, base, B, T)
    from gl_gym_amd import PPO
    return PPO(col, opt, n_epochs=1, n_minibatches=N_MB, clip_range=CLIP, ent_coef=0.0, vf_coef=0.5, max_grad_norm=None, seed=0).update


class Other:
    """The other side of (e): a child process on the parent commit's build, or (without --parent-pkg) this build."""

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


def torch_sample(torch, mean, log_std, eps):
    """stable_baselines3's squashed Gaussian from the actor's outputs: rsample, tanh, log_prob, the 1e-6 correction."""
    ls = log_std.clamp(-20.0, 2.0)
    dist = torch.distributions.Normal(mean, ls.exp())
    u = mean + ls.exp() * eps
    a = torch.tanh(u)
    return a, dist.log_prob(u).sum(-1) - torch.log(1 - a.pow(2) + 1e-6).sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", default=None, help="built greenlight-gym2_amd directory of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sac_update_cost.txt"))
    ap.add_argument("--n-envs", type=int, default=B0)
    ap.add_argument("--n-steps", type=int, default=T0)
    ap.add_argument("--batch-size", type=int, default=M0)
    ap.add_argument("--worker", nargs=4, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker[0]), args.worker[1], int(args.worker[2]), int(args.worker[3]))
    B, T, M = args.n_envs, args.n_steps, args.batch_size
    torch, make = setup(ROOT / "greenlight-gym2_amd")
    if not torch.cuda.is_available():
        sys.exit("sac_update_cost.py needs a GPU (no fallback)")
    from gl_gym_amd import SAC, ReplayCollector, _lib as L
    from gl_gym_amd.sac import sac_rows
    from train_sac import Actor, Critic
    where = ("child processes on the parent commit's build (--parent-pkg)" if args.parent_pkg else "THIS build (no --parent-pkg given: no verdict)")
    lines = [f"soft actor-critic on the device: cost on {torch.cuda.get_device_name(0)} (tools/sac_update_cost.py)",
             f"fp32 ls5-128, VecNormalizeGPU(VecMonitorGPU(TomatoVecEnv)), {B} environments, a ring of {N_SLOTS} slots, minibatches of {M} rows, actor "
             f"3 x 256 and critics 3 x 512 with SiLU; device events, {N_WARM} warm-up windows, {N_SAMPLES} alternating repeats; spread = (max - min) / "
             f"median of a side's repeats; the other side of (e) runs in {where}", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731
    fmt = lambda v, k=1.0, d=3: " ".join(f"{x * k:.{d}f}" for x in v)  # noqa: E731
    med = statistics.median
    ok = True

    base, env = make(B)
    dev, D = base.device, base.obs_dim
    torch.manual_seed(0)
    actor, c1, c2 = Actor(D).to(dev), Critic(D).to(dev), Critic(D).to(dev)
    col = ReplayCollector(env, actor, N_SLOTS, seed=0, action_noise_sigma=0.05)
    col.reset(seed=666)
    col.collect(N_SLOTS - 1, explore="uniform")
    a_opt = torch.optim.Adam(actor.parameters(), lr=7e-4, amsgrad=True)
    c_opt = torch.optim.Adam(list(c1.parameters()) + list(c2.parameters()), lr=7e-4, amsgrad=True)
    sac = SAC(col, c1, c2, a_opt, c_opt, batch_size=M, gamma=GAMMA, tau=TAU, target_entropy=TE, seed=0)
    h, stream, lib = env._h, env._stream, env._lib
    rnd = lambda *s: torch.randn(*s, device=dev)  # noqa: E731

    def both(mine, theirs):
        """Five alternating samples of the library side and the torch side, both warmed up, each the mean of five windows."""
        for _ in range(N_WARM):
            timed(torch, theirs)
        return alternate(torch, mine, lambda: timed(torch, theirs, 5), 5)

    # ---- (a) the squashed sample, forward + backward ------------------------------------------------------------------------------------
    mean, log_std = rnd(M, 6), (rnd(M, 6) * 2 - 2).contiguous()
    ga, gl = rnd(M, 6), rnd(M)
    buf = sac.pi_buffers
    ag = L.make_plan_args(L.SacRowsGradArgs, M, ga.data_ptr(), gl.data_ptr(), buf.eps.data_ptr(), buf.std.data_ptr(), buf.tanh.data_ptr(),
                          log_std.data_ptr(), buf.grad_mean.data_ptr(), buf.grad_log_std.data_ptr())

    def hip_sample():
        sac_rows(h, stream(), M, mean=mean, log_std=log_std, seed=1, action=buf.action, logp=buf.logp, eps=buf.eps, std=buf.std, tanh=buf.tanh)
        L.check(lib.glgym_sac_rows_grad(h, C.byref(ag), stream()), "glgym_sac_rows_grad")

    leaves = [mean.clone().requires_grad_(), log_std.clone().requires_grad_()]

    def th_sample():
        a, logp = torch_sample(torch, *leaves, torch.randn_like(mean))
        return torch.autograd.grad((a * ga).sum() + (logp * gl).sum(), leaves)

    x, y = both(hip_sample, th_sample)
    m_x, m_y = med(x), med(y)
    lib_ms = 2 * m_x                                     # a gradient step samples twice (the second time without the backward launch)
    say(f"(a) squashed_sample = glgym_sac_rows + glgym_sac_rows_grad, {M} rows, us             : {fmt(x, 1e3, 1)}   median {m_x * 1e3:.1f}")
    say(f"    torch randn / rsample / tanh / log_prob / correction, forward + backward, us       : {fmt(y, 1e3, 1)}   median {m_y * 1e3:.1f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio kernels / torch = {m_x / m_y:.4f} (requirement, not slower: "
        f"{'met' if m_x <= m_y else 'NOT MET'})")
    say()
    ok = ok and m_x <= m_y

    # ---- (b) the two loss stages ----------------------------------------------------------------------------------------------------------
    q1, q2, q1n, q2n, logp, rew = (rnd(M) for _ in range(6))
    done = (torch.rand(M, device=dev) < 0.1).to(torch.uint8)
    sac.refresh_alpha()
    alpha_t, la = sac.alpha_t, sac.log_alpha.detach()
    stats = torch.zeros(2, 8, dtype=torch.float64, device=dev)
    la_args = [L.make_plan_args(L.SacLossArgs, M, st, 0, q1.data_ptr(), q2.data_ptr(), logp.data_ptr(), q1n.data_ptr(), q2n.data_ptr(), rew.data_ptr(),
                                done.data_ptr(), alpha_t.data_ptr(), la.data_ptr(), GAMMA, TE, sac.grad_q1.data_ptr(), sac.grad_q2.data_ptr(),
                                sac.grad_logp.data_ptr(), sac.target_t.data_ptr() if st == 0 else None, sac.grad_log_alpha_t.data_ptr() if st else None,
                                stats[st].data_ptr(), sac.workspace.data_ptr(), L.SAC_LOSS_WS_BYTES) for st in (0, 1)]

    def hip_loss():
        for a in la_args:
            L.check(lib.glgym_sac_loss(h, C.byref(a), stream()), "glgym_sac_loss")

    lq = [q1.clone().requires_grad_(), q2.clone().requires_grad_()]
    lp = [q1.clone().requires_grad_(), q2.clone().requires_grad_(), logp.clone().requires_grad_()]
    lal = la.clone().requires_grad_()
    donef = done.float()

    def th_loss():
        with torch.no_grad():
            yv = rew + (1 - donef) * GAMMA * (torch.min(q1n, q2n) - alpha_t * logp)
        cl = 0.5 * (torch.nn.functional.mse_loss(lq[0], yv) + torch.nn.functional.mse_loss(lq[1], yv))
        g1 = torch.autograd.grad(cl, lq)
        al = (alpha_t * lp[2] - torch.min(lp[0], lp[1])).mean()
        g2 = torch.autograd.grad(al, lp)
        el = -(lal * (lp[2].detach() + TE)).mean()
        return g1, g2, torch.autograd.grad(el, [lal])

    x, y = both(hip_loss, th_loss)
    m_x, m_y = med(x), med(y)
    lib_ms += m_x
    nbytes = M * (37 + 24)
    say(f"(b) glgym_sac_loss, critic stage + actor stage (two calls), {M} rows, us          : {fmt(x, 1e3, 1)}   median {m_x * 1e3:.1f}")
    say(f"    the torch critic, actor and entropy-coefficient chains, forward + backward, us     : {fmt(y, 1e3, 1)}   median {m_y * 1e3:.1f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio kernels / torch = {m_x / m_y:.4f} (requirement, not slower: "
        f"{'met' if m_x <= m_y else 'NOT MET'}); 37 + 24 bytes a row: {nbytes / (m_x * 1e-3) / 1e12:.2f} TB/s achieved, the finishing launches "
        f"included (a streaming kernel reaches about {STREAM_TBS} TB/s on an MI355X)")
    say()
    ok = ok and m_x <= m_y

    # ---- (c) sampling from the ring ---------------------------------------------------------------------------------------------------------
    ring, S = col.ring, col.S
    flat_obs, flat_act = ring["observations"].reshape(S * B, D), ring["actions"].reshape(S * B, 6)
    flat_rew, flat_done = ring["rewards"].reshape(-1), ring["dones"].reshape(-1)
    head, n_valid = col.head, col.n_valid

    def th_batch():
        idx = torch.randint(0, n_valid * B, (M,), device=dev)
        slot, b = (head + idx // B) % S, idx % B
        row, nxt = slot * B + b, ((slot + 1) % S) * B + b
        return flat_obs[row], flat_obs[nxt], flat_act[row], flat_rew[row], flat_done[row]

    x, y = both(sac.batch, th_batch)
    m_x, m_y = med(x), med(y)
    lib_ms += m_x
    nbytes = M * 2 * (2 * D * 4 + 24 + 4 + 1)
    say(f"(c) glgym_sac_batch, {M} rows of {D} + {D} + 6 + 1 floats and a byte, us              : {fmt(x, 1e3, 1)}   median {m_x * 1e3:.1f}")
    say(f"    torch.randint + the five index gathers, us                                         : {fmt(y, 1e3, 1)}   median {m_y * 1e3:.1f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio kernel / torch = {m_x / m_y:.4f} (recorded, no bar); read + written "
        f"{nbytes / (m_x * 1e-3) / 1e12:.2f} TB/s achieved (streaming: about {STREAM_TBS} TB/s)")
    say()

    # ---- (d) Polyak ---------------------------------------------------------------------------------------------------------------------------
    tp = list(sac.target1.parameters()) + list(sac.target2.parameters())
    sp = [p.detach() for p in list(c1.parameters()) + list(c2.parameters())]

    def th_polyak():
        with torch.no_grad():
            torch._foreach_mul_(tp, 1 - TAU)
            torch._foreach_add_(tp, sp, alpha=TAU)

    x, y = both(sac.polyak, th_polyak)
    m_x, m_y = med(x), med(y)
    lib_ms += m_x
    n_el = sum(p.numel() for p in tp)
    say(f"(d) glgym_polyak, {len(tp)} tensors, {n_el} elements, one launch, us                  : {fmt(x, 1e3, 1)}   median {m_x * 1e3:.1f}")
    say(f"    torch._foreach_mul_ + torch._foreach_add_, us                                      : {fmt(y, 1e3, 1)}   median {m_y * 1e3:.1f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio kernel / torch = {m_x / m_y:.4f} (recorded, no bar)")
    say()

    # ---- (f) one gradient step end to end ---------------------------------------------------------------------------------------------------
    log_alpha = torch.zeros(1, device=dev, requires_grad=True)
    e_opt = torch.optim.Adam([log_alpha], lr=7e-4)
    mse = torch.nn.functional.mse_loss

    def th_step(losses=True):
        obs, nobs, act, r, d = th_batch()
        d = d.float()
        m_, ls_ = actor(obs)
        a_pi, logp_pi = torch_sample(torch, m_, ls_, torch.randn_like(m_)) if losses else (torch.tanh(m_ + ls_), ls_.sum(-1))
        alpha = log_alpha.exp().detach()
        if losses:
            el = -(log_alpha * (logp_pi.detach() + TE)).mean()
            e_opt.zero_grad()
            el.backward()
            e_opt.step()
        with torch.no_grad():
            mn, lsn = actor(nobs)
            a_n, logp_n = torch_sample(torch, mn, lsn, torch.randn_like(mn)) if losses else (torch.tanh(mn + lsn), lsn.sum(-1))
            qn1, qn2 = sac.target1(nobs, a_n), sac.target2(nobs, a_n)
            yv = r + (1 - d) * GAMMA * (torch.min(qn1, qn2) - alpha * logp_n) if losses else qn1 + qn2
        qa, qb = c1(obs, act), c2(obs, act)
        cl = 0.5 * (mse(qa, yv) + mse(qb, yv)) if losses else (qa + qb).sum()
        c_opt.zero_grad()
        cl.backward()
        c_opt.step()
        qa, qb = c1(obs, a_pi), c2(obs, a_pi)
        al = (alpha * logp_pi - torch.min(qa, qb)).mean() if losses else (qa + qb).sum() + logp_pi.sum()
        a_opt.zero_grad()
        al.backward()
        a_opt.step()
        th_polyak()

    for _ in range(N_WARM):
        timed(torch, th_step)
        timed(torch, lambda: th_step(False))
    x, y = alternate(torch, lambda: sac.update(1), lambda: timed(torch, th_step))
    z = [timed(torch, lambda: th_step(False)) for _ in range(N_SAMPLES)]
    m_x, m_y, m_z = med(x), med(y), med(z)
    say(f"(f) SAC.update(1), one gradient step of {M} rows, ms                               : {fmt(x)}   median {m_x:.3f}")
    say(f"    the same step in torch ops (randint, gathers, the chains of (a) and (b), _foreach), ms : {fmt(y)}   median {m_y:.3f}")
    say(f"    the networks alone (the torch step with every loss replaced by a plain sum), ms    : {fmt(z)}   median {m_z:.3f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} % / {spread(z) * 100:.1f} %; ratio SAC.update / torch = {m_x / m_y:.4f} (recorded); "
        f"the step's library launches, from the medians of (a) twice, (b), (c) and (d): {lib_ms:.3f} ms = {lib_ms / m_x * 100:.1f} % of SAC.update's step; "
        f"the networks (their GEMMs, autograd through them, the optimisers) are the other {100 - lib_ms / m_x * 100:.1f} %")
    say()
    base.close()
    del sac, col, env, base
    torch.cuda.empty_cache()

    # ---- (e) the untouched paths ------------------------------------------------------------------------------------------------------------
    t2, base2, col2, pi, vf, ls2, opt2 = stack(ROOT / "greenlight-gym2_amd", B, T)
    for name, kind in ((f"RolloutCollector.collect() ({B} x {T})", "collector"), (f"PPO.update(), one epoch x {N_MB} minibatches", "ppo"),
                       (f"a seeded reset and {T} plain step_tensor calls", "steps")):
        mine = runner(torch, kind, base2, col2, opt2, B, T)
        other = Other(torch, args.parent_pkg, kind, B, T, mine)
        x, y = alternate(torch, mine, other)
        other.close()
        r_e = med(x) / med(y)
        say(f"(e) {name}, this build / the parent commit's, ms: {fmt(x)}  /  {fmt(y)}")
        say(f"    medians {med(x):.3f} / {med(y):.3f} ms; spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio = {r_e:.4f}"
            + (f"   (requirement <= 1.05: {'met' if r_e <= 1.05 else 'NOT MET'})" if args.parent_pkg else ""))
        ok = ok and r_e <= 1.05
    base2.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if (not args.parent_pkg or ok) else 1


if __name__ == "__main__":
    sys.exit(main())
