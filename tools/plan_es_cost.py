#!/usr/bin/env python3
"""What the evolution strategy's stages cost, measured on the GPU -> profiles/plan_es_cost.txt.

    python tools/plan_es_cost.py [--parent-pkg DIR] [--out profiles/plan_es_cost.txt] [--iters 10]

fp32, ls5, pred_horizon = 0 (23 observation columns), the 23 -> 32 -> 6 tanh net (D = 966 parameters, Ht = 161 planes); device events,
warmed up, alternating samples.
(a) Recorded, no requirement: glgym_plan_es_sample, _es_utilities and _es_update (Adam) on their own at 64 greenhouses x 1 024 candidates
    (share="greenhouse") and at 1 x 8 192 (share="all"), each against the same stage written with torch ops in float32 -- randn, the
    mirrored pair, clamp; a stable argsort, a scatter of the ranks, the centred utilities; two batched reductions over the block and the
    optimiser.  es_update reads the population once: its time is also set against that read at the HBM bandwidths of
    MI355X_MICROARCH.md (8.0 TB/s specified, 6.29 TB/s measured with a float4 copy).
(b) Requirement, ratio <= 1.05: one PolicySearch.cem iteration and one Planner.rollout of this build against the parent commit's, on the
    same inputs (their code is unchanged), with each side's run-to-run spread.
(c) Recorded, no requirement: one es() iteration against one cem() iteration at the first shape; and the return of the MEAN policy
    (evaluate(mean), share="all": 1 024 policies on 64 greenhouses) after --iters iterations of each from theta = 0.
--parent-pkg DIR: the greenlight-gym2_amd directory of a checkout of the PARENT commit with its library built; its side of (b) runs in
child processes on that build.  Without it they run on this build, the report says so and gives no verdict.
No fallback: without a GPU this fails."""
import argparse
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
P0, K0, H0 = 64, 1024, 48
K_ALL = 8192
HIDDEN = (32,)
N_SAMPLES, N_WARM = 7, 2
SEASON = 10
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12                          # bytes / s: MI355X_MICROARCH.md, "HBM3E peak BW"
ES = dict(lr=0.03, lr_std=0.1, init_std=0.1, min_std=0.01)
CEM = dict(n_elite=32, init_std=0.5, min_std=0.02, alpha=0.1)


def setup(pkg):
    sys.path.insert(0, str(pkg))
    import torch
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    return torch, TomatoVecEnv, synthetic_weather


def parent_env(torch, TomatoVecEnv, w, P):
    """The P parent environments every side starts from: seeded reset, four steps under the default controller."""
    from gl_gym_amd.baseline import RuleBasedController
    env = TomatoVecEnv(P, weather=w, dtype="float32", season_length=SEASON, pred_horizon=0.0, start_rows=list(range(0, 96 * P, 96)), seed=5,
                       auto_reset=False)
    env.reset_tensor()
    for _ in range(4):
        env.step_tensor(controller=RuleBasedController(), want_obs=True)
    assert (env.scheme, env.n_sub, env.obs_dim) == ("ls5", 128, 23)
    return env


def make_spec(env):
    import numpy as np
    from gl_gym_amd.planner import MLPSpec
    obs0 = env.obs_t.double().cpu().numpy()
    norm = (obs0.mean(axis=0), obs0.var(axis=0) + 1.0, 1e-8, 10.0)
    sizes = (23,) + HIDDEN + (6,)
    scale = [v for l in range(len(sizes) - 1) for v in (1.0 / np.sqrt(sizes[l]), 0.5)]
    return MLPSpec(23, HIDDEN, activation="tanh", squash="clip", scale=scale, obs_norm=norm)


def timed(torch, fn, n=3):
    """Device time of fn() in ms, mean of n windows between events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in ev) / n


def cem_iteration(ps):
    def run():
        ps._draw = 0                                          # the same population every time
        ps.cem(1, CEM["n_elite"], init_std=CEM["init_std"], min_std=CEM["min_std"], alpha=CEM["alpha"], seed=1)
    return run


def worker(pkg, P, K, H, kind, block_file):
    """Planner.rollout(actions_t) (kind "actions") or one PolicySearch.cem iteration (kind "cem") on the build under pkg; answers
    "time" on stdin with one sample."""
    torch, TomatoVecEnv, synthetic_weather = setup(pkg)
    env = parent_env(torch, TomatoVecEnv, synthetic_weather(n_rows=35040), P)
    if kind == "actions":
        block = torch.load(block_file).to(env.device).contiguous()
        plan = env.planner(K, H)
        run = lambda: plan.rollout(actions_t=block)  # noqa: E731
    else:
        search = env.policy_search(K, H, make_spec(env))
        plan, run = search.plan, cem_iteration(search)
    for _ in range(N_WARM):
        timed(torch, run, 1)
    print(f"ready {float(plan.ret_t.sum()):.17g}", flush=True)
    for line in sys.stdin:
        if line.strip() != "time":
            break
        print(f"ms {timed(torch, run):.6f}", flush=True)


class Other:
    """The other side of a comparison: a child process on the parent commit's build, or (without --parent-pkg) this build."""

    def __init__(self, torch, pkg, P, K, H, kind, block, local_run, local_plan):
        self.torch, self.child, self.tmp = torch, None, None
        if pkg:
            self.tmp = tempfile.NamedTemporaryFile(suffix=".pt")
            if block is not None:
                torch.save(block.cpu(), self.tmp.name)
            self.child = subprocess.Popen([sys.executable, __file__, "--worker", str(Path(pkg).resolve()), str(P), str(K), str(H), kind, self.tmp.name],
                                          stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
            ready = self.child.stdout.readline().split()
            assert ready and ready[0] == "ready", "the parent-commit worker did not start"
            self.sum = float(ready[1])
        else:
            self.run = local_run
            for _ in range(N_WARM):
                timed(torch, local_run, 1)
            self.sum = float(local_plan.ret_t.sum())

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
            self.child.wait(timeout=60)


def spread(v):
    return (max(v) - min(v)) / statistics.median(v)


def compare(torch, mine, other, n=3):
    for _ in range(N_WARM):
        timed(torch, mine, 1)
    a, b = [], []
    for _ in range(N_SAMPLES):
        a.append(timed(torch, mine, n))
        b.append(other.sample() if hasattr(other, "sample") else timed(torch, other, n))
    return a, b


def stage_costs(torch, ps, say, label):
    """(a) at the shape of ps: the three kernels through ps's own methods against torch ops on tensors of the same shapes."""
    from gl_gym_amd import _lib as L
    Ht, P, K, M, dev = ps.Ht, ps.P, ps.K, ps.K // 2, ps.env.device
    st = ps._es()
    mean, std = ps.mean_t, ps.std_t
    mean.zero_()
    std.fill_(0.1)
    g = torch.Generator().manual_seed(4)
    st.score_t.copy_(torch.randn(P * K, generator=g, dtype=torch.float64).to(dev))
    st.score_failed_t.copy_((torch.rand(P * K, generator=g) < 0.02).to(torch.uint8).to(dev))
    block = ps.sample_mirrored(mean, std, seed=1, draw_index=0)
    ps._theta = block                                         # the stages on their own: no rollout in between
    ps.utilities()
    mean0, std0 = mean.clone(), std.clone()
    nbytes = Ht * P * K * L.NU * 4
    say(f"{label}: P = {P} rows x K = {K} candidates, Ht = {Ht} planes: the population is {nbytes / 1e6:.1f} MB")
    score, failed = st.score_t.view(P, K), st.score_failed_t.view(P, K)
    ar = torch.arange(K, device=dev, dtype=torch.float32).expand(P, K).contiguous()
    m1, m2 = torch.zeros(Ht, P, 6, device=dev), torch.zeros(Ht, P, 6, device=dev)
    keep = {}

    def hip_sample():
        ps._cem.cur = 1                                       # always into block 0
        ps.sample_mirrored(mean, std, seed=1, draw_index=0)

    def th_sample():
        e = torch.randn(Ht, P, M, 6, device=dev) * std.view(Ht, P, 1, 6)
        m = mean.view(Ht, P, 1, 6)
        keep["block"] = torch.stack(((m + e).clamp_(-1, 1), (m - e).clamp_(-1, 1)), dim=3).view(Ht, P * K, 6)

    def hip_util():
        ps.utilities()

    def th_util():
        adm = (failed == 0) & torch.isfinite(score)
        order = torch.argsort(torch.where(adm, -score, float("inf")), dim=1, stable=True)
        rank = torch.empty_like(ar).scatter_(1, order, ar)
        n = adm.sum(dim=1, keepdim=True)
        u = torch.where(adm, 0.5 - rank.double() / (n - 1).clamp(min=1), -0.5)
        keep["u"] = torch.where(n >= 2, u, 0.0)

    def hip_update():
        st.t = 0
        ps.es_update(mean, std, ES["lr"], ES["lr_std"], 1.0, min_std=ES["min_std"])

    def th_update():
        th = block.view(Ht, P, M, 2, 6)
        d = (th[:, :, :, 0] - th[:, :, :, 1]) * 0.5
        uu = keep["u"].view(P, M, 2).float()
        gr = ((uu[:, :, 0] - uu[:, :, 1]).view(1, P, M, 1) * d).sum(dim=2) / M
        z = d / std.view(Ht, P, 1, 6)
        s = ((uu[:, :, 0] + uu[:, :, 1]).view(1, P, M, 1) * (z * z - 1)).sum(dim=2) / M
        m1.mul_(0.9).add_(gr, alpha=0.1)
        m2.mul_(0.999).addcmul_(gr, gr, value=0.001)
        keep["mean"] = mean + ES["lr"] * (m1 / 0.1) / ((m2 / 0.001).sqrt() + 1e-8)
        keep["std"] = (std * torch.exp(0.5 * ES["lr_std"] * s)).clamp_(ES["min_std"], 1.0)

    th_util()
    hip_util()
    du = float((keep["u"] - st.u_t.view(P, K)).abs().max())
    th_update()
    hip_update()
    dm, ds = float((keep["mean"] - mean).abs().max()), float((keep["std"] - std).abs().max())
    say(f"  torch form against the kernels on the same inputs: largest difference of a utility {du:.1e}, of a new mean {dm:.1e}, of a new std {ds:.1e}")
    out = {}
    for name, hip, th, inner in (("sample", hip_sample, th_sample, 5), ("utilities", hip_util, th_util, 20), ("update", hip_update, th_update, 5)):
        mean.copy_(mean0)
        std.copy_(std0)
        m1.zero_()
        m2.zero_()
        for fn in (hip, th):
            timed(torch, fn, 2)
        a, b = compare(torch, hip, th, inner)
        ma, mb = statistics.median(a), statistics.median(b)
        out[name] = (ma, mb)
        say(f"  glgym_plan_es_{name:9s} us: " + " ".join(f"{v * 1e3:.1f}" for v in a) + f"   median {ma * 1e3:.1f} (spread {spread(a) * 100:.0f} %)")
        say("  the same with torch ops us: " + " ".join(f"{v * 1e3:.1f}" for v in b) + f"   median {mb * 1e3:.1f} (spread {spread(b) * 100:.0f} %)")
        say(f"    ratio kernel / torch = {ma / mb:.3f}" + ("   (the kernel is NOT faster than its torch form)" if ma >= mb else ""))
        keep.pop("block", None)
    t_upd = out["update"][0] * 1e-3
    say(f"  es_update reads the population once: {nbytes / 1e6:.1f} MB in {t_upd * 1e6:.1f} us = {nbytes / t_upd / 1e12:.2f} TB/s; that read alone "
        f"takes {nbytes / HBM_SPEC * 1e6:.1f} us at 8.0 TB/s (specified peak) and {nbytes / HBM_COPY * 1e6:.1f} us at 6.29 TB/s (measured float4 "
        f"copy): the kernel takes {t_upd / (nbytes / HBM_SPEC):.2f} x and {t_upd / (nbytes / HBM_COPY):.2f} x those times"
        + ("  (a block under 256 MB can sit in the Infinity Cache, which the sample before it filled)" if nbytes < 256e6 else ""))
    say()
    mean.copy_(mean0)
    std.copy_(std0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-pkg", default=None, help="built greenlight-gym2_amd directory of the parent commit")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plan_es_cost.txt"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--worker", nargs=6, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(Path(args.worker[0]), *(int(v) for v in args.worker[1:4]), args.worker[4], args.worker[5])
    torch, TomatoVecEnv, synthetic_weather = setup(ROOT / "greenlight-gym2_amd")
    if not torch.cuda.is_available():
        sys.exit("plan_es_cost.py needs a GPU (no fallback)")
    P, K, H = P0, K0, H0
    n = P * K
    where = ("child processes on the parent commit's build (--parent-pkg)" if args.parent_pkg else
             "THIS build (no --parent-pkg given)")
    lines = [f"evolution strategy on the device: cost on {torch.cuda.get_device_name(0)} (tools/plan_es_cost.py)",
             f"fp32 ls5-128, pred_horizon 0 (23 observation columns), net 23 -> 32 -> 6 tanh; device events, {N_WARM} warm-up windows, {N_SAMPLES} "
             f"alternating samples; spread = (max - min) / median of a side's samples; the other side of (b) runs in {where}", ""]
    say = lambda s="": (print(s, flush=True), lines.append(s))  # noqa: E731
    w = synthetic_weather(n_rows=35040)
    env = parent_env(torch, TomatoVecEnv, w, P)
    dev = env.device
    spec = make_spec(env)

    # ---- (a) the stages on their own --------------------------------------------------------------------------------------------------
    say("(a) the three stages against torch ops (float32 randn / argsort + scatter / two reductions + Adam), recorded, no requirement")
    ps = env.policy_search(K, H, spec)
    stage_costs(torch, ps, say, '64 x 1 024, share="greenhouse"')
    one = parent_env(torch, TomatoVecEnv, w, 1)
    ps_all = one.policy_search(K_ALL, 2, make_spec(one), share="all")
    stage_costs(torch, ps_all, say, '1 x 8 192, share="all"')
    del ps_all
    one.close()
    torch.cuda.empty_cache()

    # ---- (c) one es() iteration against one cem() iteration ---------------------------------------------------------------------------
    ps.es(1, **ES)

    def es_iteration():
        ps._draw = 0
        ps.es(1, **ES)

    def cem_same_spread():
        ps._draw = 0
        ps.cem(1, CEM["n_elite"], init_std=ES["init_std"], min_std=ES["min_std"], alpha=CEM["alpha"], seed=1)

    a, b = compare(torch, es_iteration, cem_same_spread)
    say(f"(c) one iteration at (P, K, H) = ({P}, {K}, {H}), {n} children, both from theta = 0 with init_std {ES['init_std']} (the rollout is the "
        f"cost, and it depends on the policies: the wide first population of (b), init_std {CEM['init_std']}, walks the controls to their bounds, "
        f"where the step kernels take extra attempts); recorded, no requirement")
    say("    es()  (sample_mirrored, rollout, utilities, es_update, select), ms: " + " ".join(f"{v:.3f}" for v in a))
    say("    cem() (sample, rollout, elites, refit, select), ms                : " + " ".join(f"{v:.3f}" for v in b))
    say(f"      medians {statistics.median(a):.3f} / {statistics.median(b):.3f} ms; spreads {spread(a) * 100:.1f} % / {spread(b) * 100:.1f} %; "
        f"ratio es / cem = {statistics.median(a) / statistics.median(b):.4f}")
    say()

    # ---- (b) the untouched paths against the parent commit's: requirement <= 1.05 ---------------------------------------------------------
    other = Other(torch, args.parent_pkg, P, K, H, "cem", None, cem_iteration(ps), ps.plan)
    mine = cem_iteration(ps)
    mine()
    my_sum = float(ps.plan.ret_t.sum())
    a, b = compare(torch, mine, other)
    other.close()
    r_cem = statistics.median(a) / statistics.median(b)
    verdict = lambda r: f"   (requirement <= 1.05: {'met' if r <= 1.05 else 'NOT MET'})" if args.parent_pkg else ""  # noqa: E731
    say("(b) one PolicySearch.cem iteration, this build / the parent commit's, ms: " + " ".join(f"{v:.3f}" for v in a) + "  /  " + " ".join(f"{v:.3f}" for v in b))
    say(f"      sum of the {n} returns {my_sum:.17g} / {other.sum:.17g} ({'equal' if my_sum == other.sum else 'DIFFERENT'})")
    say(f"      medians {statistics.median(a):.3f} / {statistics.median(b):.3f} ms; spreads {spread(a) * 100:.1f} % / {spread(b) * 100:.1f} %; "
        f"ratio = {r_cem:.4f}" + verdict(r_cem))
    del ps
    torch.cuda.empty_cache()
    plan = env.planner(K, H)
    g = torch.Generator().manual_seed(3)
    fresh = (torch.rand(H, n, 6, generator=g) * 2 - 1).to(dev).contiguous()
    other = Other(torch, args.parent_pkg, P, K, H, "actions", fresh, lambda: plan.rollout(actions_t=fresh), plan)
    a, b = compare(torch, lambda: plan.rollout(actions_t=fresh), other)
    other.close()
    my_sum = float(plan.ret_t.sum())
    r_plan = statistics.median(a) / statistics.median(b)
    say("    Planner.rollout(actions_t = uniform random actions), this build / the parent commit's, ms: " + " ".join(f"{v:.3f}" for v in a) + "  /  " + " ".join(f"{v:.3f}" for v in b))
    say(f"      sum of the {n} returns {my_sum:.17g} / {other.sum:.17g} ({'equal' if my_sum == other.sum else 'DIFFERENT'})")
    say(f"      medians {statistics.median(a):.3f} / {statistics.median(b):.3f} ms; spreads {spread(a) * 100:.1f} % / {spread(b) * 100:.1f} %; "
        f"ratio = {r_plan:.4f}" + verdict(r_plan))
    say()
    del plan, fresh
    torch.cuda.empty_cache()

    # ---- (c) the mean policy after --iters iterations of each -----------------------------------------------------------------------------
    search = env.policy_search(K, H, spec, share="all")
    base = float(search.evaluate(torch.zeros(search.Ht, 1, 6))[0][:, 0].mean())
    search._draw = 0
    es = search.es(args.iters, seed=1, **ES)
    r_es, b_es = float(search.evaluate(search.mean_t)[0][:, 0].mean()), float(es["best_return"][0])
    search._draw = 0
    cem = search.cem(args.iters, CEM["n_elite"], init_std=CEM["init_std"], min_std=CEM["min_std"], alpha=CEM["alpha"], seed=1)
    b_cem = float(cem["best_return"][0])
    r_cem_mean = float(search.evaluate(search.mean_t)[0][:, 0].mean())
    say(f"(c) share=\"all\": {K} policies on {P} greenhouses, H = {H}, {args.iters} iterations from theta = 0 (which scores {base:.4f}); score = the mean "
        f"return over the greenhouses; recorded, no requirement; one seed")
    say(f"    es  (adam lr {ES['lr']}, lr_std {ES['lr_std']}, init_std {ES['init_std']}): the MEAN policy scores {r_es:.4f}; the last population's best {b_es:.4f}")
    say(f"    cem (n_elite {CEM['n_elite']}, init_std {CEM['init_std']}, alpha {CEM['alpha']}): the MEAN policy scores {r_cem_mean:.4f}; the last population's best {b_cem:.4f}")
    say()
    ok = r_cem <= 1.05 and r_plan <= 1.05
    env.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text("\n".join(lines) + "\n")
    return 0 if (ok or not args.parent_pkg) else 1


if __name__ == "__main__":
    sys.exit(main())
