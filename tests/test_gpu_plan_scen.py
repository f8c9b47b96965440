"""Robust planning on the GPU: glgym_plan_scenario, glgym_plan_rollout_scenarios, glgym_plan_aggregate (include/glgym.h) and the
scenario mode of gl_gym_amd/planner.py, against the restatements of tests/test_plan_scen_host.py.

Everything is compared bit for bit: the kernels' crop blocks, expanded action plane and risk scores equal the NumPy / Python
restatements; a scenario rollout equals a loop of plain env-steps of an independently constructed environment whose per-env crop
block is filled from the restatement before every step; a captured graph replays the eager results.  Child batches stay <= 4 096 and
horizons <= 4."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_plan import clone_children_into, make_env, rand_actions, same_bits, same_state, weights
from test_plan_host import np_accumulate
from test_plan_scen_host import AGG_SHAPES, NCROP, aggregate_case, np_scen_crop, py_aggregate, same_f64

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
SEED, DRAW, BASE = 0xDEADBEEF12345678, (7 << 32) | 41, 5


def started(B, dtype, **kw):
    env = make_env(B, dtype, **kw)
    env.reset_tensor()
    for k in range(2):
        env.step_tensor(rand_actions((B, 6), 20 + k, env.device))
    return env


def dev(env, a):
    import torch
    return torch.as_tensor(a, device=env.device).contiguous()


def handle_crop(env):
    """float32 p[128..161] as the handle keeps them on the device."""
    return np.asarray(env.p, dtype=np.float64)[128:162].astype(np.float32)


# ---- 1. the kernels equal the restatements ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("P,K,S", [(2, 3, 5), (3, 7, 4), (1, 1, 1)])       # 84 children: a ragged second wavefront
def test_scenario_kernel_matches_the_restatement(P, K, S, dtype):
    import torch
    from gl_gym_amd import _lib as L
    env = make_env(1, dtype)
    n, ld, scale = P * K * S, P * K * S + 3, 0.2
    p0 = handle_crop(env)
    acts = rand_actions((P * K, 6), 7, env.device)
    base_t = torch.full((1,), BASE, dtype=torch.int64, device=env.device)
    for hold in (0, 1):
        for h in (0, 2):
            crop_t = torch.full((NCROP, ld), 7, dtype=env.tdtype, device=env.device)
            out_t = torch.full((n + 1, 6), 7, dtype=torch.float32, device=env.device)
            a = L.make_plan_args(L.PlanScenarioArgs, P, K, S, ld, h, hold, scale, SEED, DRAW, base_t.data_ptr(), crop_t.data_ptr(),
                                 acts.data_ptr(), out_t.data_ptr())
            assert env._lib.glgym_plan_scenario(env._h, C.byref(a), env._stream()) == L.OK
            exp = np_scen_crop(P, K, S, h, hold, scale, SEED, DRAW + BASE, p0)
            got = crop_t.cpu().numpy()
            assert got[:, :n].dtype == (np.float32 if dtype == "float32" else np.float64)
            assert np.array_equal(got[:, :n], exp.astype(got.dtype)), (hold, h, np.abs(got[:, :n] - exp).max())
            assert np.array_equal(got[:, :n].astype(np.float32).view(np.uint32), exp.view(np.uint32))
            assert (got[:, n:] == 7).all()                                  # nothing past the last child
            assert np.array_equal(out_t[:n].cpu().numpy(), np.repeat(acts.cpu().numpy(), S, axis=0)) and (out_t[n] == 7).all()
    # without an action plane only the crop block is written; without a base word D = draw_index
    crop_t = torch.full((NCROP, ld), 7, dtype=env.tdtype, device=env.device)
    a = L.make_plan_args(L.PlanScenarioArgs, P, K, S, ld, 1, 0, scale, SEED, DRAW, None, crop_t.data_ptr(), None, None)
    assert env._lib.glgym_plan_scenario(env._h, C.byref(a), env._stream()) == L.OK
    assert np.array_equal(crop_t.cpu().numpy()[:, :n].astype(np.float32), np_scen_crop(P, K, S, 1, 0, scale, SEED, DRAW, p0))
    env.close()


@pytest.mark.parametrize("S,m", AGG_SHAPES)
def test_aggregate_kernel_matches_the_python_loop(S, m):
    import torch
    from gl_gym_amd import _lib as L
    env = make_env(1, "float32")
    J = 6
    ret, failed, viol, n_steps, ld = aggregate_case(np.random.default_rng(1000 * S + m), J, S)       # the CPU test's cases
    ldc = J + 2
    rc_t = torch.full((J,), 7.0, dtype=torch.float64, device=env.device)
    fc_t = torch.full((J,), 7, dtype=torch.uint8, device=env.device)
    vc_t = torch.full((3, ldc), 7.0, dtype=torch.float64, device=env.device)
    sc_t = torch.full((J,), 7, dtype=torch.int32, device=env.device)
    ins = [dev(env, v) for v in (ret, failed, viol, n_steps)]
    a = L.make_plan_args(L.PlanAggregateArgs, J, S, m, ld, ldc, *(t.data_ptr() for t in ins), rc_t.data_ptr(), fc_t.data_ptr(),
                         vc_t.data_ptr(), sc_t.data_ptr())
    assert env._lib.glgym_plan_aggregate(env._h, C.byref(a), env._stream()) == L.OK
    e_rc, e_fc, e_vc, e_sc = py_aggregate(J, S, m, ret, failed, viol, n_steps)
    assert same_f64(rc_t.cpu().numpy(), e_rc), (rc_t.cpu().numpy(), e_rc)
    assert np.array_equal(fc_t.cpu().numpy(), e_fc) and e_fc.tolist() == [1, 1, 1, 0, 0, 0]
    vc = vc_t.cpu().numpy()
    assert same_f64(vc[:, :J], e_vc) and (vc[:, J:] == 7).all()
    assert np.array_equal(sc_t.cpu().numpy(), e_sc)
    # the optional outputs left out: the scores alone, the same bits
    rc_t.fill_(7.0)
    a = L.make_plan_args(L.PlanAggregateArgs, J, S, m, ld, ldc, ins[0].data_ptr(), ins[1].data_ptr(), None, None, rc_t.data_ptr(),
                         fc_t.data_ptr(), None, None)
    assert env._lib.glgym_plan_aggregate(env._h, C.byref(a), env._stream()) == L.OK
    assert same_f64(rc_t.cpu().numpy(), e_rc)
    env.close()


# ---- 2. a scenario rollout is a loop of plain env-steps -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,layout,noise", [("float64", None, "step"), ("float64", None, "hold"), ("float32", "one", "step"),
                                                ("float32", "quad", "step")])
def test_scenario_rollout_is_a_loop_of_plain_env_steps(dtype, layout, noise):
    B, K, S, H, gamma, scale, n_tail = 2, 3, 4, 3, 0.99, 0.2, 2
    n = B * K * S
    env = started(B, dtype, uncertainty_scale=scale)
    plan = env.planner(K, H, gamma=gamma, n_scenarios=S, n_tail=n_tail, noise=noise, scenario_seed=SEED)
    assert plan.C == n and plan.J == B * K and plan.noise_scale == scale and plan.crop_T is not None
    if layout:
        plan.set_layout(layout)              # "quad" requested: with a crop block the selector takes the one-lane build all the same
    plan.scenario_base_t.fill_(BASE)
    plan.new_scenarios()                     # scenario draw index 1
    acts = rand_actions((H, B * K, 6), 31, env.device)
    ret, alive, steps, viol, failed = plan.rollout(acts)
    env2 = make_env(n, dtype, uncertainty_scale=scale)
    env2.freeze_crop_noise = True            # the hand-set per-env block is what each step sees
    if layout:
        env2.set_layout(layout)
    clone_children_into(env2, env, K * S)
    p0 = handle_crop(env)
    rs, infos, dones, flags = [], [], [], []
    for h in range(H):
        block = np_scen_crop(B, K, S, h, noise == "hold", scale, SEED, 1 + BASE, p0)
        env2.crop_T[:, :n].copy_(dev(env, block).to(env2.tdtype))
        _, r, d, info = env2.step_tensor(actions_t=acts[h].repeat_interleave(S, dim=0).contiguous(), want_obs=False)
        rs.append(r.double().cpu().numpy().copy())
        infos.append(info[[8, 7, 9]].double().cpu().numpy().copy())
        dones.append(d.cpu().numpy().copy())
        flags.append(env2.step_flags_t.cpu().numpy().copy())
    e_ret, e_viol, e_n, e_alive, e_failed = np_accumulate(weights(gamma, H), np.array(rs), np.array(infos), np.array(dones), np.array(flags))
    got = plan.scenario_returns.cpu().numpy()
    assert got.shape == (B, K, S) and same_f64(got.reshape(-1), e_ret), np.abs(got.reshape(-1) - e_ret).max()
    assert np.array_equal(plan.n_steps_t.cpu().numpy(), e_n) and (e_n == H).all()
    assert np.array_equal(plan.scenario_failed.cpu().numpy().reshape(-1).astype(bool), e_failed)
    assert same_f64(plan.viol_T[:, :n].cpu().numpy(), e_viol)
    assert np.array_equal(plan.alive_t.cpu().numpy().astype(bool), e_alive)
    assert not np.array_equal(got[:, :, 0], got[:, :, 1])                  # the futures really differ
    # the [B, K] outputs are the restated aggregate of those
    e_rc, e_fc, e_vc, e_sc = py_aggregate(B * K, S, n_tail, e_ret, e_failed.astype(np.uint8), e_viol, e_n)
    assert ret.shape == (B, K) and viol.shape == (3, B, K) and alive.shape == steps.shape == failed.shape == (B, K)
    assert same_f64(ret.cpu().numpy().reshape(-1), e_rc)
    assert np.array_equal(failed.cpu().numpy().reshape(-1), e_fc) and not e_fc.any()
    assert same_f64(viol.cpu().numpy().reshape(3, -1), e_vc)
    assert np.array_equal(steps.cpu().numpy().reshape(-1), e_sc)
    assert np.array_equal(alive.cpu().numpy().reshape(-1).astype(bool), e_alive.reshape(B * K, S).all(axis=1))
    # select() scores the aggregated returns
    sel = plan.select()
    assert np.array_equal(sel["best_k"].cpu().numpy(), e_rc.reshape(B, K).argmax(axis=1))
    assert same_f64(sel["best_return"].cpu().numpy(), e_rc.reshape(B, K).max(axis=1))
    with pytest.raises(ValueError):
        plan.rollout(controls_t=acts)
    env.close(); env2.close()


# ---- 3. common random numbers, 4. risk ordering --------------------------------------------------------------------------------------
def test_common_random_numbers_and_risk_ordering():
    B, K, S, H = 2, 4, 5, 3
    env = started(B, "float32", uncertainty_scale=0.2)
    acts = rand_actions((H, B, K, 6), 41, env.device)
    acts[:, :, 2] = acts[:, :, 0]                                          # candidates 0 and 2: the same action sequence
    by_tail = {}
    for n_tail in (1, 2, S):
        plan = env.planner(K, H, n_scenarios=S, n_tail=n_tail, scenario_seed=3)
        by_tail[n_tail] = plan.rollout(acts)[0].cpu().numpy().copy()
        sr = plan.scenario_returns
        assert same_bits(sr[:, 0], sr[:, 2]) and not same_bits(sr[:, 0], sr[:, 1])
        assert same_bits(plan.ret_cand_t.view(B, K)[:, 0], plan.ret_cand_t.view(B, K)[:, 2])
        assert not same_bits(sr[:, :, 0], sr[:, :, 1])                         # the futures really differ
        if n_tail > 1:
            assert same_bits(sr, first)                                    # the same futures whatever the risk measure
        first = sr.clone()
    assert (by_tail[1] <= by_tail[2]).all() and (by_tail[2] <= by_tail[S]).all() and (by_tail[1] < by_tail[S]).any()
    assert np.array_equal(by_tail[1], first.min(dim=2).values.cpu().numpy())
    # noise_scale = 0: all S scenario returns of a candidate are identical
    flat = env.planner(K, H, n_scenarios=S, noise_scale=0.0)
    flat.rollout(acts)
    sr0 = flat.scenario_returns
    assert same_bits(sr0, sr0[:, :, :1].expand(B, K, S)) and not same_bits(sr0[:, 0], sr0[:, 1])
    # noise_scale defaults to the environment's uncertainty_scale; the keyword checks
    assert plan.noise_scale == 0.2 and plan.n_tail == S
    for kw in ({"n_scenarios": 0}, {"n_scenarios": 257}, {"n_scenarios": 4, "n_tail": 5}, {"n_scenarios": 4, "n_tail": 0},
               {"n_scenarios": 4, "noise": "white"}, {"n_scenarios": 4, "noise_scale": -0.1}, {"n_tail": 2}, {"noise_scale": 0.1}):
        with pytest.raises(ValueError):
            env.planner(K, H, **kw)
    with pytest.raises(ValueError):
        env.planner(K, H).new_scenarios()
    env.close()


# ---- 5. the parent is untouched -----------------------------------------------------------------------------------------------------
def test_scenario_cem_leaves_the_parent_untouched():
    B, K, S, H, E = 2, 16, 3, 3, 4
    env = started(B, "float32", uncertainty_scale=0.2)
    plan = env.planner(K, H, n_scenarios=S, n_tail=2)
    state0, metrics0, flags0 = env.get_state(), env.metrics(), env.step_flags_t.clone()
    plan.cem(2, E, carry=1, beta=0.5)
    plan.new_scenarios()
    plan.shift(0.5)
    same_state(env.get_state(), state0)
    assert env.metrics() == metrics0 and metrics0["n_env_steps"] == 2 * B
    assert same_bits(env.step_flags_t, flags0)
    env.close()


# ---- 6. monotone under carry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_best_return_never_decreases_with_carry_on_fixed_scenarios(dtype):
    B, K, S, H, E = 2, 16, 3, 3, 4
    env = started(B, dtype, uncertainty_scale=0.2)
    plan = env.planner(K, H, gamma=0.99, n_scenarios=S, n_tail=2)
    bests, mean_t, std_t = [], None, None
    for it in range(4):
        out = plan.cem(1, E, init_std=0.4, carry=2, beta=0.3, seed=8, mean_t=mean_t, std_t=std_t)
        mean_t, std_t = out["mean_sequence"], out["std_sequence"]
        bests.append(out["best_return"].cpu().numpy().copy())
        if it > 0:                                                          # candidate 1 IS the previous best, on the same futures
            assert same_f64(plan.ret_cand_t.view(B, K)[:, 1].cpu().numpy(), bests[it - 1])
            assert (bests[it] >= bests[it - 1]).all(), (it, bests)
    assert np.isfinite(np.array(bests)).all()
    assert out["elite_k"].shape == (B, E) and same_f64(out["best_return"].cpu().numpy(), plan.ret_cand_t.view(B, K).max(dim=1).values.cpu().numpy())
    # other futures for the same action block
    block = plan._actions.clone()
    plan.rollout(block)
    before = plan.scenario_returns.clone()
    plan.rollout(block)
    assert same_bits(plan.scenario_returns, before)                        # fixed from rollout to rollout ...
    plan.new_scenarios()
    plan.rollout(block)
    assert not same_bits(plan.scenario_returns, before)                    # ... until new_scenarios()
    env.close()


# ---- 7. graph capture ---------------------------------------------------------------------------------------------------------------
def test_scenario_cem_replays_from_a_captured_graph(tmp_path):
    import torch
    B, K, S, H, E = 2, 16, 3, 3, 4
    env = started(B, "float32", uncertainty_scale=0.2)
    plan = env.planner(K, H, gamma=0.99, n_scenarios=S, n_tail=2)

    def decision():
        plan._draw = 0                        # the same draw indices every time; mean_t None resets the distribution
        return plan.cem(2, E, carry=1, beta=0.5, seed=3)

    def outputs():
        return [plan._actions, plan.ret_t, plan.ret_cand_t, plan.failed_cand_t, plan.steps_cand_t, plan.alive_cand_t, plan.viol_cand_T,
                plan.cem_mean_t, plan.cem_std_t, plan.best_k_t, plan.best_ret_t, plan.best_action_t, plan.best_sequence_t,
                plan.elite_k_t[:B * E], plan.n_elite_t]

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
    # the device word behind the scenario draw moves: the replay scores the same populations on other futures
    plan.scenario_base_t += 1
    graph.replay()
    torch.cuda.synchronize(env.device)
    replayed = [t.clone() for t in outs]
    assert not same_bits(replayed[1], eager[1]) and not same_bits(replayed[2], eager[2])
    decision()                                                             # eager at the same base: the same bits again
    for t, e in zip(outputs(), replayed):
        assert same_bits(t, e)
    # the captured work is one chain: every node of the graph but the last has exactly one successor, every one but the first one predecessor
    probe = torch.cuda.CUDAGraph(keep_graph=True)                          # keeps the captured graph so that it can be written out
    probe.enable_debug_mode()
    with torch.cuda.graph(probe):
        decision()
    probe.instantiate()
    dot = tmp_path / "scenario_cem.dot"
    probe.debug_dump(str(dot))
    text = dot.read_text()
    nodes = set(re.findall(r'^"(graph_\w+)"\[', text, flags=re.M))
    edges = re.findall(r'^"(graph_\w+)" -> "(graph_\w+)"', text, flags=re.M)
    assert len(nodes) >= 2 * (3 * H + 6)              # per iteration: sample, fork, H x (prologue, step, accumulate), aggregate, alive, elites, refit
    assert len(edges) == len(nodes) - 1
    src, dst = [a for a, _ in edges], [b for _, b in edges]
    assert len(set(src)) == len(src) and len(set(dst)) == len(dst), "the captured graph has parallel branches"
    assert any("plan_scenario_kernel" in line for line in text.splitlines()) and any("plan_aggregate_kernel" in line for line in text.splitlines())
    env.close()


# ---- 8. n_scenarios=None is today's planner -------------------------------------------------------------------------------------------
def test_without_scenarios_the_planner_is_unchanged():
    B, K, H = 3, 8, 3
    env = started(B, "float32", uncertainty_scale=0.2)
    acts = rand_actions((H, B * K, 6), 51, env.device)
    for crop in ("nominal", "current"):
        a, b = env.planner(K, H, gamma=0.99, crop=crop), env.planner(K, H, gamma=0.99, crop=crop, n_scenarios=None)
        out_a, out_b = a.rollout(acts), b.rollout(acts)
        for x, y in zip(out_a, out_b):
            assert same_bits(x, y)
        sel_a, sel_b = a.select(temperature=0.5, sequence=True), b.select(temperature=0.5, sequence=True)
        assert sel_a.keys() == sel_b.keys()
        for k in sel_a:
            assert same_bits(sel_a[k], sel_b[k]), k
        assert b.S is None and b.C == b.J == B * K and (b.crop_T is None) == (crop == "nominal")
    env.close()


# ---- 9. the example -------------------------------------------------------------------------------------------------------------------
def test_mpc_robust_example_runs():
    r = subprocess.run([sys.executable, "examples/mpc_robust.py", "--season", "0.25", "--candidates", "32", "--scenarios", "4", "--tail", "2",
                        "--horizon", "4", "--iters", "2", "--elites", "8"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"8 greenhouses x 25 steps.*?robust CEM-MPC \(4 scenarios.*?closed-loop return ([-\d.e+]+).*?nominal CEM-MPC.*?closed-loop return "
                  r"([-\d.e+]+)", r.stdout, flags=re.S)
    assert m, r.stdout
    assert np.isfinite(float(m.group(1))) and np.isfinite(float(m.group(2)))
    assert "without an admissible candidate: robust 0, nominal 0" in r.stdout and "nan" not in r.stdout.lower()


# ---- the boundary's argument checks, on a live handle ---------------------------------------------------------------------------------
def test_rollout_scenarios_refuses_what_glgym_step_refuses():
    from gl_gym_amd import _lib as L
    B, K, S, H = 2, 3, 4, 2
    env = started(B, "float32", uncertainty_scale=0.2)
    plan = env.planner(K, H, n_scenarios=S)
    acts = rand_actions((H, B * K, 6), 61, env.device)
    plan.rollout(acts)
    lib, h, st = env._lib, env._h, env._stream()

    def args():
        r = L.make_plan_args(L.PlanRolloutArgs, H, 1.0, plan._step_args(), acts.data_ptr(), None, plan.ret_t.data_ptr(), plan.viol_T.data_ptr(),
                             plan.n_steps_t.data_ptr(), plan.alive_t.data_ptr(), plan.failed_t.data_ptr())
        return L.make_plan_args(L.PlanRolloutScenariosArgs, B, K, S, 0, 0.2, 1, 0, None, plan.stage_t.data_ptr(), r)

    assert lib.glgym_plan_rollout_scenarios(h, C.byref(args()), st) == L.OK
    before = [t.clone() for t in (plan.crop_T, plan.stage_t, plan.ret_t, plan.x_T)]
    a = args()
    a.rollout.step.x = None                                                # glgym_step's own check, in its own words, nothing launched
    assert lib.glgym_plan_rollout_scenarios(h, C.byref(a), st) == L.EINVAL and b"glgym_step" in lib.glgym_last_error()
    for field, value in (("S", 257), ("scale", -1.0), ("K", K + 1)):
        a = args()
        setattr(a, field, value)
        assert lib.glgym_plan_rollout_scenarios(h, C.byref(a), st) == L.EINVAL, field
    import torch
    torch.cuda.synchronize(env.device)
    for t, b in zip((plan.crop_T, plan.stage_t, plan.ret_t, plan.x_T), before):
        assert same_bits(t, b)
    env.close()
