#!/usr/bin/env python3
"""What the PPO update costs, measured on the GPU -> profiles/ppo_update_cost.txt.

    python tools/ppo_update_cost.py [--parent-pkg DIR] [--out profiles/ppo_update_cost.txt]

The set-up of tools/collect_cost.py: fp32, ls5, VecNormalizeGPU(VecMonitorGPU(TomatoVecEnv)), 65 536 environments x 64 steps = 4.2 M
transitions, 4 minibatches, tanh nets 23-64-64-6 and 23-64-1 (examples/collect_rollouts.py); device events, warmed up, five alternating
repeats with their spreads, no profiler.
(a) Requirement, not slower: glgym_ppo_loss (forward and backward in one call) against the example's torch loss chain, forward plus
    backward, from the heads' outputs to their gradients, on the same minibatch.  Achieved bytes per second: the 92 bytes a row needs
    (mean, action, four scalars in; grad_mean, grad_value out) over the call's time.
(b) Recorded: glgym_ppo_batch for one epoch (4 calls, with the advantage statistics) against torch.randperm plus the six index gathers.
(c) Requirement, not slower (overlapping sample ranges count as on par): one PPO.update() of one epoch against the example's torch update
    loop run from the PARENT commit's package on the same rollout.
(d) Requirement, ratio <= 1.05: RolloutCollector.collect() and a plain 64-step step_tensor loop against the parent commit's build.
--parent-pkg DIR: the greenlight-gym2_amd directory of a checkout of the PARENT commit with its library built; the other sides of (c)
and (d) run in child processes on that build.  Without it they run on this build, the report says so and gives no verdict.
No fallback: without a GPU this fails."""
import argparse
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from collect_cost import B0, GAMMA, HIDDEN, LAM, N_SAMPLES, N_WARM, T0, alternate, setup, spread, step_loop, timed  # noqa: E402

N_MB, CLIP = 4, 0.2
ROW_BYTES = 4 * (6 + 6 + 4 + 6 + 1)


def nets(torch, D, dev):
    """The nets of examples/collect_rollouts.py."""
    torch.manual_seed(0)
    lin, act = torch.nn.Linear, torch.nn.Tanh
    pi = torch.nn.Sequential(lin(D, HIDDEN), act(), lin(HIDDEN, HIDDEN), act(), lin(HIDDEN, 6)).to(dev)
    vf = torch.nn.Sequential(lin(D, HIDDEN), act(), lin(HIDDEN, 1)).to(dev)
    return pi, vf, torch.nn.Parameter(torch.zeros(6, device=dev))


def torch_loss(torch, mean, value, log_std, act, old_logp, adv, ret):
    """The loss chain of examples/collect_rollouts.py from the heads' outputs."""
    noise = (act - mean) / log_std.exp()
    logp = (-0.5 * noise.pow(2) - log_std - 0.9189385).sum(-1)
    ratio = (logp - old_logp).exp()
    a = (adv - adv.mean()) / (adv.std() + 1e-8)
    return -torch.min(ratio * a, ratio.clamp(1 - CLIP, 1 + CLIP) * a).mean() + 0.5 * (ret - value).pow(2).mean()


def torch_update(torch, col, pi, vf, log_std, opt):
    """The optimiser phase of examples/collect_rollouts.py: one epoch over torch.randperm minibatches."""
    buf, N = col.buffer, col.T * col.B
    obs, act = buf["observations"].reshape(N, -1), buf["actions"].reshape(N, 6)
    old_logp, adv, ret = buf["log_probs"].reshape(-1), buf["advantages"].reshape(-1), buf["returns"].reshape(-1)

    def run():
        for idx in torch.randperm(N, device=obs.device).chunk(N_MB):
            loss = torch_loss(torch, pi(obs[idx]), vf(obs[idx]).squeeze(-1), log_std, act[idx], old_logp[idx], adv[idx], ret[idx])
            opt.zero_grad()
            loss.backward()
            opt.step()
    return run


def stack(pkg, B, T):
    torch, make = setup(pkg)
    from gl_gym_amd import RolloutCollector, TorchHeads
    base, env = make(B)
    pi, vf, log_std = nets(torch, base.obs_dim, base.device)
    col = RolloutCollector(env, T, TorchHeads(pi, vf, log_std), gamma=GAMMA, gae_lambda=LAM, seed=0)
    col.reset(seed=666)
    col.collect()
    opt = torch.optim.Adam(list(pi.parameters()) + list(vf.parameters()) + [log_std], lr=3e-4)
    return torch, base, col, pi, vf, log_std, opt


def worker(pkg, kind, B, T):
    """The torch update loop ("update"), RolloutCollector.collect() ("collector") or a plain step_tensor loop ("steps") on the build under
    pkg; answers "time" on stdin with one sample."""
    torch, base, col, pi, vf, log_std, opt = stack(pkg, B, T)
    run = {"update": lambda: torch_update(torch, col, pi, vf, log_std, opt), "collector": lambda: col.collect,
           "steps": lambda: step_loop(torch, base, B, T)}[kind]()
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ppo_update_cost.txt"))
    ap.add_argument("--n-envs", type=int, default=B0)
    ap.add_argument("--n-steps", type=int, default=T0)
    ap.add_argument("--worker", nargs=4, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker[0]), args.worker[1], int(args.worker[2]), int(args.worker[3]))
    B, T = args.n_envs, args.n_steps
    torch, base, col, pi, vf, log_std, opt = stack(ROOT / "greenlight-gym2_amd", B, T)
    if not torch.cuda.is_available():
        sys.exit("ppo_update_cost.py needs a GPU (no fallback)")
    import ctypes as C
    from gl_gym_amd import PPO, _lib as L
    N = B * T
    where = ("child processes on the parent commit's build (--parent-pkg)" if args.parent_pkg else
             "THIS build (no --parent-pkg given: no verdict)")
    lines = [f"the PPO update on the device: cost on {torch.cuda.get_device_name(0)} (tools/ppo_update_cost.py)",
             f"fp32 ls5-128, VecNormalizeGPU(VecMonitorGPU(TomatoVecEnv)), {B} environments x {T} steps = {N} transitions, {N_MB} minibatches, tanh "
             f"nets 23-{HIDDEN}-{HIDDEN}-6 and 23-{HIDDEN}-1; device events, {N_WARM} warm-up windows, {N_SAMPLES} alternating repeats; spread = "
             f"(max - min) / median of a side's repeats; the other side of (c) and (d) runs in {where}", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731
    fmt = lambda v, k=1.0, d=3: " ".join(f"{x * k:.{d}f}" for x in v)  # noqa: E731
    ppo = PPO(col, opt, n_epochs=1, n_minibatches=N_MB, clip_range=CLIP, ent_coef=0.0, vf_coef=0.5, max_grad_norm=None, seed=0)
    env = col.env
    ok = True

    # ---- (a) the loss stage from the heads' outputs to their gradients ------------------------------------------------------------------
    mb = ppo.batch(0)
    M = ppo.sizes[0]
    with torch.no_grad():
        mean, value = pi(mb["observations"]).contiguous(), vf(mb["observations"]).reshape(-1).contiguous()
    lb, ls = ppo.loss_buffers, log_std.detach()
    torch.exp(-ls, out=lb.inv_std)
    a = L.make_plan_args(L.PpoLossArgs, M, mean.data_ptr(), value.data_ptr(), ls.data_ptr(), lb.inv_std.data_ptr(), mb["actions"].data_ptr(),
                         mb["log_probs"].data_ptr(), mb["advantages"].data_ptr(), mb["returns"].data_ptr(), None, ppo.adv_stats_t.data_ptr(),
                         CLIP, 0.0, 0.5, 0.0, lb.grad_mean.data_ptr(), lb.grad_value.data_ptr(), lb.grad_log_std.data_ptr(), lb.stats.data_ptr(),
                         None, None, lb.workspace.data_ptr(), L.PPO_LOSS_WS_BYTES)
    hip_loss = lambda: L.check(env._lib.glgym_ppo_loss(env._h, C.byref(a), env._stream()), "glgym_ppo_loss")  # noqa: E731
    leaves = [mean.clone().requires_grad_(), value.clone().requires_grad_(), ls.clone().requires_grad_()]

    def th_loss():
        loss = torch_loss(torch, *leaves, mb["actions"], mb["log_probs"], mb["advantages"], mb["returns"])
        return torch.autograd.grad(loss, leaves)

    hip_loss()
    g = th_loss()
    diff = float((g[0] - lb.grad_mean[:M]).abs().max() / g[0].abs().max())
    x, y = alternate(torch, hip_loss, lambda: timed(torch, th_loss, 5), 5)
    m_x, m_y = statistics.median(x), statistics.median(y)
    say(f"(a) glgym_ppo_loss, forward + backward, {M} rows, us                          : {fmt(x, 1e3, 1)}   median {m_x * 1e3:.1f}")
    say(f"    the example's torch loss chain, forward + backward, on the same minibatch, us : {fmt(y, 1e3, 1)}   median {m_y * 1e3:.1f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio kernel / torch = {m_x / m_y:.4f} (requirement, not slower: "
        f"{'met' if m_x <= m_y else 'NOT MET'}); {ROW_BYTES} bytes a row: {M * ROW_BYTES / (m_x * 1e-3) / 1e12:.2f} TB/s achieved, the finishing "
        f"launch included (a streaming kernel reaches about 6.3 TB/s on an MI355X); largest difference of a mean gradient / largest gradient {diff:.2e}")
    say()
    ok = ok and m_x <= m_y

    # ---- (b) minibatch assembly, one epoch ----------------------------------------------------------------------------------------------
    buf = col.buffer
    obs, act = buf["observations"].reshape(N, -1), buf["actions"].reshape(N, 6)
    flat = [buf[k].reshape(-1) for k in ("log_probs", "advantages", "returns", "values")]

    def hip_epoch():
        for i in range(len(ppo.sizes)):
            ppo.batch(i)

    def th_epoch():
        for idx in torch.randperm(N, device=obs.device).chunk(N_MB):
            _ = obs[idx], act[idx], flat[0][idx], flat[1][idx], flat[2][idx], flat[3][idx]

    x, y = alternate(torch, hip_epoch, lambda: timed(torch, th_epoch, 5), 5)
    m_x, m_y = statistics.median(x), statistics.median(y)
    say(f"(b) glgym_ppo_batch, one epoch = {N_MB} calls (gathers + advantage statistics), us : {fmt(x, 1e3, 1)}   median {m_x * 1e3:.1f}")
    say(f"    torch.randperm + the six index gathers per minibatch, us                      : {fmt(y, 1e3, 1)}   median {m_y * 1e3:.1f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio kernel / torch = {m_x / m_y:.4f} (recorded, no bar)")
    say()

    # ---- (c) one full update --------------------------------------------------------------------------------------------------------------
    th_run = torch_update(torch, col, pi, vf, log_std, opt)
    other = Other(torch, args.parent_pkg, "update", B, T, th_run)
    x, y = alternate(torch, ppo.update, other)
    other.close()
    m_x, m_y = statistics.median(x), statistics.median(y)
    overlap = max(x) >= min(y) and max(y) >= min(x)
    met = m_x <= m_y or overlap
    say(f"(c) PPO.update(), one epoch x {N_MB} minibatches of {M} rows, ms                : {fmt(x)}   median {m_x:.3f}")
    say(f"    the torch update loop of examples/collect_rollouts.py on the same rollout, ms : {fmt(y)}   median {m_y:.3f}")
    say(f"    spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio PPO.update / torch = {m_x / m_y:.4f}"
        + ("   (the samples of the two sides overlap: on par)" if overlap else "")
        + (f"   (requirement, not slower: {'met' if met else 'NOT MET'})" if args.parent_pkg else ""))
    say()
    ok = ok and met

    # ---- (d) the untouched paths ----------------------------------------------------------------------------------------------------------
    for name, kind, mine in ((f"RolloutCollector.collect() ({B} x {T})", "collector", col.collect),
                             (f"a seeded reset and {T} plain step_tensor calls", "steps", step_loop(torch, base, B, T))):
        other = Other(torch, args.parent_pkg, kind, B, T, mine)
        x, y = alternate(torch, mine, other)
        other.close()
        r_d = statistics.median(x) / statistics.median(y)
        say(f"(d) {name}, this build / the parent commit's, ms: {fmt(x)}  /  {fmt(y)}")
        say(f"    medians {statistics.median(x):.3f} / {statistics.median(y):.3f} ms; spreads {spread(x) * 100:.1f} % / {spread(y) * 100:.1f} %; ratio = {r_d:.4f}"
            + (f"   (requirement <= 1.05: {'met' if r_d <= 1.05 else 'NOT MET'})" if args.parent_pkg else ""))
        ok = ok and r_d <= 1.05
    base.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if (not args.parent_pkg or ok) else 1


if __name__ == "__main__":
    sys.exit(main())
