"""The cross-entropy method's stages on the GPU: glgym_plan_sample, glgym_plan_elites, glgym_plan_refit (include/glgym.h) and
Planner.sample / elites / refit / cem / shift (gl_gym_amd/planner.py), against the NumPy restatements and with the bounds of
tests/test_plan_cem_host.py: words, reserved candidates and elite order exact; sampled actions within np.spacing(np.float32(1)) of the
float64 restatement; the refitted float32 values within one float32 ulp of NumPy's rounded ones.  Returns are compared bit for bit:
a cem() iteration goes through the same entry point as Planner.rollout().  Shapes P = 3, K = 70, H = 3, E = 7 unless stated."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_plan import make_env, rand_actions, same_bits, same_state
from test_plan_cem_host import F32_STEP, MOMENT_SEED, make_returns, moment_checks, np_elites, np_noise, np_refit, np_sample, within_one_f32_ulp

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu


def started(P, dtype="float32"):
    env = make_env(P, dtype)
    env.reset_tensor()
    for k in range(2):
        env.step_tensor(rand_actions((P, 6), 20 + k, env.device))
    return env


def dev(env, a):
    import torch
    return torch.as_tensor(a, device=env.device).contiguous()


# ---- 1. the three kernels against NumPy ------------------------------------------------------------------------------------------
# H = 11: the sample kernel takes the horizon in groups of four steps and carries the noise from group to group -- three groups, the
# last one short; the recurrence (beta = 0.5) and the carried elites are compared over all of them
@pytest.mark.parametrize("P,K,H,E", [(3, 70, 3, 7), (2, 300, 2, 300), (1, 1, 1, 1), (2, 257, 3, 64), (2, 70, 11, 7)])
def test_kernels_match_the_numpy_restatements(P, K, H, E):
    env = started(P)
    plan = env.planner(K, H)
    rng = np.random.default_rng(K)
    mean = rng.uniform(-1.2, 1.2, (H, P, 6)).astype(np.float32)
    std = rng.uniform(0.05, 0.6, (H, P, 6)).astype(np.float32)
    mean_t, std_t = dev(env, mean), dev(env, std)
    seed, draw, base, beta = 0xDEADBEEF12345678, 2 ** 40 + 3, 5, 0.5
    plan.draw_base_t.fill_(base)
    block = plan.sample(mean_t, std_t, beta=beta, seed=seed, draw_index=draw)
    got = block.cpu().numpy()
    exp, exact = np_sample(P, K, H, mean, std, beta, seed, draw + base)
    err = np.abs(got.astype(np.float64) - exp).max()
    print(f"sample P={P} K={K} H={H}: max |action - float64 restatement| = {err:.2e} (bound {F32_STEP:.2e})")
    assert err <= F32_STEP
    assert np.array_equal(got[:, exact], exp[:, exact].astype(np.float32))       # candidate 0: the clipped mean
    assert (np.abs(got) <= 1).all()
    # elites on made-up returns (ties, failures, NaN, infinities) over a real rollout's buffers
    plan.rollout(block)
    ret, failed = make_returns(rng, P, K)
    if K == 1:
        ret[:], failed[:] = 0.5, 0
    elif P > 1:
        failed[(P - 1) * K:] = 1                                                 # the last parent: nothing admissible
        failed[(P - 1) * K + K // 2], ret[(P - 1) * K + K // 2] = 0, 1.0         # ... but one
    plan.ret_t.copy_(dev(env, ret)); plan.failed_t.copy_(dev(env, failed))
    elite_t, n_t = plan.elites(E)
    e_elite, e_n = np_elites(P, K, E, ret, failed)
    assert np.array_equal(elite_t.cpu().numpy(), e_elite) and np.array_equal(n_t.cpu().numpy(), e_n)
    # refit, out of place through the C entry point and in place through the planner
    from gl_gym_amd import _lib as L
    import torch
    mo_t, so_t = torch.full_like(mean_t, 7), torch.full_like(std_t, 7)
    alpha, min_std = 0.25, 0.05
    a = L.make_plan_args(L.PlanRefitArgs, P, K, H, E, block.data_ptr(), plan.elite_k_t.data_ptr(), plan.n_elite_t.data_ptr(), alpha, min_std,
                         mean_t.data_ptr(), std_t.data_ptr(), mo_t.data_ptr(), so_t.data_ptr())
    assert env._lib.glgym_plan_refit(env._h, C.byref(a), env._stream()) == L.OK
    e_mo, e_so, _, _ = np_refit(P, K, H, got, e_elite, e_n, alpha, min_std, mean, std)
    assert within_one_f32_ulp(mo_t.cpu().numpy(), e_mo) and within_one_f32_ulp(so_t.cpu().numpy(), e_so)
    assert (so_t.cpu().numpy()[:, e_n > 0] >= np.float32(min_std)).all()
    if P > 1 and K > 1 and e_n[P - 1] == 1:                                      # one elite: its own sequence, spread at the floor
        assert np.array_equal(mo_t.cpu().numpy()[:, P - 1], (alpha * mean[:, P - 1].astype(np.float64)
                                                               + (1 - alpha) * got[:, (P - 1) * K + K // 2].astype(np.float64)).astype(np.float32))
    # carry: the next population holds the clipped mean and the previous elites, exactly; the rest is sampled as without carry
    carry = min(4, E)
    block2 = plan.sample(mean_t, std_t, beta=beta, seed=seed, draw_index=draw + 1, carry=carry)
    assert block2.data_ptr() != block.data_ptr()
    got2 = block2.cpu().numpy()
    exp2, exact2 = np_sample(P, K, H, mean, std, beta, seed, draw + 1 + base, carry, got, e_elite, e_n)
    assert np.array_equal(got2[:, exact2], exp2[:, exact2].astype(np.float32))
    assert np.abs(got2.astype(np.float64) - exp2).max() <= F32_STEP
    assert exact2.sum() == P + sum(min(carry, K - 1, int(n)) for n in e_n)
    plan.refit(mean_t, std_t, alpha, min_std)                                    # in place = out of place
    assert same_bits(mean_t, mo_t) and same_bits(std_t, so_t)
    env.close()


def test_refit_keeps_a_parent_without_elites_and_clipping_holds():
    P, K, H, E = 3, 70, 3, 7
    env = started(P)
    plan = env.planner(K, H)
    import torch
    mean_t = torch.zeros(H, P, 6, dtype=torch.float32, device=env.device)
    std_t = torch.full((H, P, 6), 10.0, dtype=torch.float32, device=env.device)
    block = plan.sample(mean_t, std_t, seed=9)
    got = block.cpu().numpy()
    exp, _ = np_sample(P, K, H, np.zeros((H, P, 6), np.float32), np.full((H, P, 6), 10, np.float32), 0.0, 9, 0)
    assert (np.abs(got) <= 1).all() and (got == 1).mean() > 0.3 and (got == -1).mean() > 0.3
    assert np.abs(got.astype(np.float64) - exp).max() <= F32_STEP
    plan.rollout(block)
    plan.failed_t[K:2 * K] = 1                                                   # parent 1: no admissible candidate
    elite_t, n_t = plan.elites(E)
    assert n_t.cpu().numpy().tolist() == [E, 0, E] and (elite_t[1] == -1).all()
    plan.refit(mean_t, std_t, 0.0, 0.0)
    assert (mean_t[:, 1] == 0).all() and (std_t[:, 1] == 10).all()               # kept
    e_mo, e_so, _, _ = np_refit(P, K, H, got, elite_t.cpu().numpy(), n_t.cpu().numpy(), 0.0, 0.0, np.zeros((H, P, 6), np.float32),
                                np.full((H, P, 6), 10, np.float32))
    assert within_one_f32_ulp(mean_t.cpu().numpy(), e_mo) and within_one_f32_ulp(std_t.cpu().numpy(), e_so)
    assert float(std_t[:, 0].max()) <= 1.0                                       # alpha = 0: the elites' own spread
    env.close()


def test_sample_moments_and_independent_steps_on_the_device():
    """The host test's moment and beta = 0 checks at K = 4 096 (64 blocks of the sample kernel), same seed, same bounds."""
    import torch
    P, K, beta = 1, 4096, 0.9
    env = started(P)
    std32 = np.float64(np.float32(0.2))
    plan2, plan3 = env.planner(K, 2), env.planner(K, 3)
    z = lambda H, v: torch.full((H, P, 6), v, dtype=torch.float32, device=env.device)  # noqa: E731
    got = plan2.sample(z(2, 0.0), z(2, 0.2), beta=beta, seed=MOMENT_SEED, draw_index=0).cpu().numpy()
    exp, _ = np_sample(P, K, 2, np.zeros((2, P, 6), np.float32), np.full((2, P, 6), 0.2, np.float32), beta, MOMENT_SEED, 0)
    assert np.abs(got.astype(np.float64) - exp).max() <= F32_STEP
    w = moment_checks(got[:, 1:].astype(np.float64) / std32, beta)
    print(f"moments on the device over N = {K - 1}: |mean| {w[0]:.4f}, |var - 1| {w[1]:.4f}, |corr - 0.9| {w[2]:.4f}")
    white = plan3.sample(z(3, 0.0), z(3, 0.2), beta=0.0, seed=MOMENT_SEED, draw_index=1).cpu().numpy()
    coloured = plan3.sample(z(3, 0.0), z(3, 0.2), beta=0.5, seed=MOMENT_SEED, draw_index=1).cpu().numpy()
    assert np.array_equal(white[0], coloured[0]) and not np.array_equal(white[1], coloured[1])     # n_0 = e_0 whatever beta is
    e = np.clip(std32 * np_noise(K, 3, 0.0, MOMENT_SEED, 1), -1, 1)
    e[:, 0] = 0.0
    assert np.abs(white.astype(np.float64) - e).max() <= F32_STEP                # beta = 0: every row is its own e_h
    n = white[:, 1:].astype(np.float64) / std32
    for h in (0, 1):
        d0, d1 = n[h] - n[h].mean(axis=0), n[h + 1] - n[h + 1].mean(axis=0)
        corr = (d0 * d1).mean(axis=0) / np.sqrt((d0 * d0).mean(axis=0) * (d1 * d1).mean(axis=0))
        assert np.abs(corr).max() <= 5 / np.sqrt(K - 1), corr
    env.close()


# ---- 2. one cem() iteration is sample + rollout + select -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_one_cem_iteration_is_sample_rollout_select(dtype):
    P, K, H, E = 3, 70, 3, 7
    env = started(P, dtype)
    plan = env.planner(K, H, gamma=0.99)
    out = plan.cem(1, E, init_std=0.4, min_std=0.05, alpha=0.1, beta=0.3, seed=4)
    block, ret = plan._actions.clone(), plan.ret_t.clone()
    best = {k: out[k].clone() for k in ("best_k", "best_return", "best_action", "best_sequence")}
    zeros, spread = np.zeros((H, P, 6), np.float32), np.full((H, P, 6), 0.4, np.float32)
    exp, exact = np_sample(P, K, H, zeros, spread, 0.3, 4, 0)
    got = block.cpu().numpy()
    assert np.abs(got.astype(np.float64) - exp).max() <= F32_STEP and (got[:, exact] == 0).all()
    other = env.planner(K, H, gamma=0.99)
    ret2 = other.rollout(block)[0]
    assert same_bits(ret2.reshape(-1), ret)                                      # the same entry point on the same block: the same bits
    sel = other.select(sequence=True)
    for k in best:
        assert same_bits(sel[k], best[k]), k
    assert out["elite_k"].shape == (P, E) and out["n_elite"].cpu().numpy().tolist() == [E] * P
    e_elite, e_n = np_elites(P, K, E, ret.cpu().numpy(), plan.failed_t.cpu().numpy())
    assert np.array_equal(out["elite_k"].cpu().numpy(), e_elite)
    assert np.array_equal(out["best_k"].cpu().numpy(), e_elite[:, 0])
    e_mo, e_so, _, _ = np_refit(P, K, H, got, e_elite, e_n, 0.1, 0.05, zeros, spread)
    assert within_one_f32_ulp(out["mean_sequence"].cpu().numpy(), e_mo) and within_one_f32_ulp(out["std_sequence"].cpu().numpy(), e_so)
    # shift: the warm start of the next decision
    m0, s0 = out["mean_sequence"].clone(), out["std_sequence"].clone()
    m1, s1 = plan.shift(0.5)
    assert same_bits(m1[:-1], m0[1:]) and same_bits(s1[:-1], s0[1:]) and (m1[-1] == 0).all() and (s1[-1] == 0.5).all()
    env.close()


# ---- 3. with carried elites the best return never decreases ----------------------------------------------------------------------
@pytest.mark.parametrize("dtype,layout", [("float64", None), ("float32", "one"), ("float32", "quad")])
def test_best_return_never_decreases_with_carry(dtype, layout):
    P, K, H, E = 3, 70, 3, 7
    env = started(P, dtype)
    plan = env.planner(K, H, gamma=0.99)
    if layout:
        plan.set_layout(layout)
    bests, mean_t, std_t = [], None, None
    for it in range(4):
        out = plan.cem(1, E, init_std=0.4, carry=2, beta=0.3, seed=8, mean_t=mean_t, std_t=std_t)
        mean_t, std_t = out["mean_sequence"], out["std_sequence"]
        bests.append(out["best_return"].cpu().numpy().copy())
        if it > 0:                                                               # candidate 1 IS the previous best, re-simulated from the same fork
            assert np.array_equal(plan.ret_t.view(P, K)[:, 1].cpu().numpy().view(np.uint64), bests[it - 1].view(np.uint64))
            assert (bests[it] >= bests[it - 1]).all(), (it, bests)
    assert np.isfinite(np.array(bests)).all()
    whole = env.planner(K, H, gamma=0.99).cem(4, E, init_std=0.4, carry=2, beta=0.3, seed=8)     # the same four populations in one call
    assert np.array_equal(whole["best_return"].cpu().numpy().view(np.uint64), bests[3].view(np.uint64))
    env.close()


# ---- 4. the parent is only read --------------------------------------------------------------------------------------------------
def test_cem_leaves_the_parent_untouched():
    P, K, H, E = 3, 70, 3, 7
    env = started(P)
    plan = env.planner(K, H)
    state0, metrics0, flags0 = env.get_state(), env.metrics(), env.step_flags_t.clone()
    plan.cem(2, E, carry=1, beta=0.5)
    plan.shift(0.5)
    same_state(env.get_state(), state0)
    assert env.metrics() == metrics0 and metrics0["n_env_steps"] == 2 * P
    assert same_bits(env.step_flags_t, flags0)
    env.close()


# ---- 5. graph capture ------------------------------------------------------------------------------------------------------------
def test_cem_replays_from_a_captured_graph():
    import torch
    P, K, H, E = 3, 70, 3, 7
    env = started(P)
    plan = env.planner(K, H, gamma=0.99)

    def decision():
        plan._draw = 0                        # the same draw indices every time: what differs between runs is draw_base_t alone
        return plan.cem(2, E, carry=1, beta=0.5, seed=3)

    def outputs():
        return [plan._actions, plan.ret_t, plan.cem_mean_t, plan.cem_std_t, plan.best_k_t, plan.best_ret_t, plan.best_action_t,
                plan.best_sequence_t, plan.elite_k_t[:P * E], plan.n_elite_t]       # elite_k_t: the [P, E] rows in use

    decision()
    eager = [t.clone() for t in outputs()]
    side = torch.cuda.Stream(device=env.device)
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        decision()
    torch.cuda.current_stream(env.device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        decision()
    outs = outputs()
    for t in outs[1:]:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize(env.device)
    for t, e in zip(outs, eager):
        assert same_bits(t, e)
    # the device word behind draw_base moves: the replay samples another population
    plan.draw_base_t += 2
    graph.replay()
    torch.cuda.synchronize(env.device)
    replayed = [t.clone() for t in outs]
    assert not same_bits(replayed[0], eager[0]) and not same_bits(replayed[1], eager[1])
    decision()                                                                   # eager at the same draw_base: the same bits again
    for t, e in zip(outputs(), replayed):
        assert same_bits(t, e)
    env.close()


# ---- 6. argument checks ----------------------------------------------------------------------------------------------------------
def test_cem_entry_points_refuse_bad_arguments():
    import torch
    from gl_gym_amd import _lib as L
    P, K, H, E = 3, 70, 3, 7
    env = started(P)
    plan = env.planner(K, H)
    out = plan.cem(2, E, carry=1)
    lib, h, st = env._lib, env._h, env._stream()
    mean_t, std_t = out["mean_sequence"], out["std_sequence"]
    cur, oth = plan._cem.blocks[plan._cem.cur], plan._cem.blocks[1 - plan._cem.cur]
    watched = [cur, oth, mean_t, std_t, plan.elite_k_t, plan.n_elite_t]
    before = [t.clone() for t in watched]

    def unchanged():
        torch.cuda.synchronize(env.device)
        return all(same_bits(t, b) for t, b in zip(watched, before))

    smp = lambda: L.make_plan_args(L.PlanSampleArgs, P, K, H, mean_t.data_ptr(), std_t.data_ptr(), 0.5, 1, 0, None, oth.data_ptr(), 1, E,  # noqa: E731
                                   cur.data_ptr(), plan.elite_k_t.data_ptr(), plan.n_elite_t.data_ptr())
    for field, value in (("struct_size", 8), ("beta", 1.0), ("beta", -0.1), ("beta", float("nan")), ("K", 0), ("H", 0), ("carry", -1),
                         ("carry", E + 1), ("prev_actions", oth.data_ptr()), ("prev_n_elite", None), ("mean", None), ("actions", None)):
        a = smp()
        setattr(a, field, value)
        assert lib.glgym_plan_sample(h, C.byref(a), st) == L.EINVAL, field
        assert b"glgym_plan_sample" in lib.glgym_last_error()
    el = lambda: L.make_plan_args(L.PlanElitesArgs, P, K, E, plan.ret_t.data_ptr(), plan.failed_t.data_ptr(), plan.elite_k_t.data_ptr(),  # noqa: E731
                                  plan.n_elite_t.data_ptr())
    for field, value in (("struct_size", 0), ("E", K + 1), ("E", 0), ("K", 0), ("P", 0), ("ret", None), ("n_elite", None)):
        a = el()
        setattr(a, field, value)
        assert lib.glgym_plan_elites(h, C.byref(a), st) == L.EINVAL, field
    rf = lambda: L.make_plan_args(L.PlanRefitArgs, P, K, H, E, cur.data_ptr(), plan.elite_k_t.data_ptr(), plan.n_elite_t.data_ptr(), 0.1,  # noqa: E731
                                  0.05, mean_t.data_ptr(), std_t.data_ptr(), mean_t.data_ptr(), std_t.data_ptr())
    for field, value in (("struct_size", 4), ("alpha", 1.0), ("alpha", -0.5), ("min_std", -1.0), ("min_std", float("nan")), ("E", K + 1),
                         ("E", 0), ("H", 0), ("H", 65536), ("actions", None), ("std_out", None)):
        a = rf()
        setattr(a, field, value)
        assert lib.glgym_plan_refit(h, C.byref(a), st) == L.EINVAL, field
    assert unchanged()
    # the planner's checks mirror them and leave everything as it was
    state = (plan._draw, plan._cem.cur, plan._cem.rolled, plan._cem.ranked)
    for call in (lambda: plan.elites(K + 1), lambda: plan.elites(0), lambda: plan.sample(mean_t, std_t, beta=1.0),
                 lambda: plan.sample(mean_t, std_t, carry=-1), lambda: plan.sample(mean_t, std_t, carry=E + 1),
                 lambda: plan.sample(mean_t[:1], std_t), lambda: plan.sample(mean_t.double(), std_t),
                 lambda: plan.refit(mean_t, std_t, 1.0, 0.05), lambda: plan.refit(mean_t, std_t, 0.1, -1.0),
                 lambda: plan.cem(0, E), lambda: plan.cem(1, K + 1), lambda: plan.cem(1, 0), lambda: plan.cem(1, E, carry=E + 1),
                 lambda: plan.cem(1, E, beta=1.0), lambda: plan.cem(1, E, alpha=1.0), lambda: plan.cem(1, E, min_std=-1.0),
                 lambda: plan.cem(1, E, mean_t=mean_t[:2]), lambda: plan.shift(-1.0)):
        with pytest.raises(ValueError):
            call()
    assert unchanged() and state == (plan._draw, plan._cem.cur, plan._cem.rolled, plan._cem.ranked)
    fresh = env.planner(K, H)
    with pytest.raises(ValueError):
        fresh.shift(0.5)
    with pytest.raises(ValueError):
        fresh.refit(mean_t, std_t, 0.1, 0.05)
    # the good arguments still pass
    assert lib.glgym_plan_sample(h, C.byref(smp()), st) == L.OK and lib.glgym_plan_elites(h, C.byref(el()), st) == L.OK
    assert lib.glgym_plan_refit(h, C.byref(rf()), st) == L.OK
    torch.cuda.synchronize(env.device)
    env.close()


# ---- 7. the example --------------------------------------------------------------------------------------------------------------
def test_mpc_cem_example_runs():
    r = subprocess.run([sys.executable, "examples/mpc_cem.py", "--season", "1", "--candidates", "64", "--horizon", "8", "--iters", "2",
                        "--elites", "8"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"8 greenhouses x 97 steps.*?CEM-MPC episode return ([-\d.e+]+).*?rule-based ([-\d.e+]+)", r.stdout, flags=re.S)
    assert m, r.stdout
    assert np.isfinite(float(m.group(1))) and np.isfinite(float(m.group(2)))
    assert "ODE failures: MPC env 0, rule-based env 0" in r.stdout and "without an admissible candidate: 0" in r.stdout
    assert "nan" not in r.stdout.lower()
