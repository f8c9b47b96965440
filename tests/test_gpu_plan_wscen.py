"""Weather-forecast scenarios on the GPU: glgym_plan_weather (include/glgym.h) and the weather_sigma mode of gl_gym_amd/planner.py, against
the restatement of tests/test_plan_wscen_host.py.

Everything is compared bit for bit: the kernel's windows and child offsets equal the NumPy restatement; a weather-scenario rollout equals
a loop of plain env-steps of an independently constructed environment whose weather table IS the restated window and whose per-env crop
block is filled from the crop restatement before every step; zero sigmas give the planner without them; a captured graph replays the
eager results and follows the parent.  Child batches stay <= 4 096 and horizons <= 7."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from test_gpu_plan import clone_children_into, make_env, rand_actions, same_bits, same_state, weights
from test_gpu_plan_scen import dev, handle_crop, started
from test_plan_host import np_accumulate
from test_plan_scen_host import np_scen_crop, py_aggregate, same_f64
from test_plan_wscen_host import SHAPES, SIGMA, np_wscen, parents, table
from test_plan_wscen_host import same_bits as np_same_bits

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
SEED, DRAW, BASE = 0xDEADBEEF12345678, (7 << 32) | 41, 5
PHI = 0.7


def parent_position(env):
    return env.weather_t.cpu().numpy(), env.w_off_t.cpu().numpy(), env.timestep_t.cpu().numpy()


# ---- 1. the kernel equals the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("P,S,H", SHAPES)
def test_weather_kernel_matches_the_restatement(P, S, H, dtype):
    import torch
    from gl_gym_amd import _lib as L
    env = make_env(1, dtype)
    K, pad = 3, 3
    weather = table(np.dtype(dtype).type)
    assert weather.shape[1] == env.nd
    rows = weather.shape[0]
    w_off, ts = parents(P, rows, H)
    weather_t, w_off_t, ts_t = dev(env, weather), dev(env, w_off), dev(env, ts)
    base_t = torch.full((1,), BASE, dtype=torch.int64, device=env.device)
    n, n_child = P * S * H, P * K * S
    for phi in (0.0, PHI):
        for base in (base_t, None):
            for offsets in (True, False):
                win_t = torch.full((n + pad, env.nd), -7, dtype=env.tdtype, device=env.device)
                child_t = torch.full((n_child + pad,), -7, dtype=torch.int32, device=env.device)
                a = L.make_plan_args(L.PlanWeatherArgs, P, K, S, H, rows, weather_t.data_ptr(), w_off_t.data_ptr(), ts_t.data_ptr(),
                                     (C.c_double * 7)(*SIGMA), phi, SEED, DRAW, base.data_ptr() if base is not None else None, win_t.data_ptr(),
                                     child_t.data_ptr() if offsets else None)
                assert env._lib.glgym_plan_weather(env._h, C.byref(a), env._stream()) == L.OK
                exp, exp_child = np_wscen(P, K, S, H, weather, w_off, ts, SIGMA, phi, SEED, DRAW + (BASE if base is not None else 0))
                got, child = win_t.cpu().numpy(), child_t.cpu().numpy()
                assert np_same_bits(got[:n], exp), (phi, np.abs(got[:n].astype(np.float64) - exp).max())
                assert (got[n:] == -7).all() and (child[n_child:] == -7).all()             # nothing past the end
                assert np.array_equal(child[:n_child], exp_child) if offsets else (child == -7).all()
    env.close()


# ---- 2. a weather-scenario rollout is a loop of plain env-steps ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype,layout", [("float64", None), ("float32", "one")])
def test_weather_scenario_rollout_is_a_loop_of_plain_env_steps(dtype, layout):
    B, K, S, H, gamma, scale, n_tail = 2, 3, 4, 3, 0.99, 0.2, 2
    n = B * K * S
    env = started(B, dtype, uncertainty_scale=scale)
    plan = env.planner(K, H, gamma=gamma, n_scenarios=S, n_tail=n_tail, scenario_seed=SEED, weather_sigma=SIGMA, weather_phi=PHI)
    assert plan.weather_window_t.shape == (B * S * H, env.nd) and plan.weather_window.shape == (B, S, H, env.nd)
    if layout:
        plan.set_layout(layout)
    plan.scenario_base_t.fill_(BASE)
    plan.new_scenarios()                     # scenario draw index 1: the crop and the weather futures move together
    acts = rand_actions((H, B * K, 6), 31, env.device)
    weather0 = env.weather_t.clone()
    ret, alive, steps, viol, failed = plan.rollout(acts)
    # the restated windows and offsets, which the kernel reproduces ...
    w_np, w_off, ts = parent_position(env)
    window, child_off = np_wscen(B, K, S, H, w_np, w_off, ts, SIGMA, PHI, SEED, 1 + BASE)
    assert np_same_bits(plan.weather_window_t.cpu().numpy(), window)
    assert same_bits(env.weather_t, weather0)
    assert not np_same_bits(window.reshape(B, S, H, -1)[:, 0, 1:], window.reshape(B, S, H, -1)[:, 1, 1:])
    # ... are the weather table and the offsets of 24 plain environments
    env2 = make_env(n, dtype, uncertainty_scale=scale)
    env2.freeze_crop_noise = True            # the hand-set per-env block is what each step sees
    if layout:
        env2.set_layout(layout)
    clone_children_into(env2, env, K * S)
    need = env2.N + 1 + env2.Np + 1          # the constructor's row check: pad with rows no child reads
    padded = np.zeros((max(need, len(window)), window.shape[1]), window.dtype)
    padded[:len(window)] = window
    padded[len(window):] = w_np[0]
    env2.weather_data = padded               # (zeroes w_off_t; timestep_t is kept)
    assert np_same_bits(env2.weather_t.cpu().numpy()[:len(window)], window)
    env2.w_off_t.copy_(dev(env, child_off))
    p0 = handle_crop(env)
    rs, infos, dones, flags = [], [], [], []
    for h in range(H):
        block = np_scen_crop(B, K, S, h, False, scale, SEED, 1 + BASE, p0)
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
    assert np.array_equal(failed.cpu().numpy().reshape(-1), e_fc)
    assert same_f64(viol.cpu().numpy().reshape(3, -1), e_vc)
    assert np.array_equal(steps.cpu().numpy().reshape(-1), e_sc)
    assert np.array_equal(alive.cpu().numpy().reshape(-1).astype(bool), e_alive.reshape(B * K, S).all(axis=1))
    env.close(); env2.close()


# ---- 3. zero sigmas change nothing ---------------------------------------------------------------------------------------------------
def test_zero_sigmas_and_none_are_the_planner_without_weather_scenarios():
    B, K, S, H = 2, 4, 3, 3
    env = started(B, "float32", uncertainty_scale=0.2)
    acts = rand_actions((H, B * K, 6), 51, env.device)
    kw = dict(gamma=0.99, n_scenarios=S, n_tail=2, scenario_seed=3)
    plain, none = env.planner(K, H, **kw), env.planner(K, H, weather_sigma=None, **kw)
    zeros = env.planner(K, H, weather_sigma=[0] * 7, weather_phi=PHI, **kw)
    assert plain.weather_window_t is None and none.weather_window_t is None and zeros.weather_window_t is not None
    out_p = [t.clone() for t in plain.rollout(acts)] + [plain.scenario_returns.clone(), plain.viol_T.clone(), plain.n_steps_t.clone()]
    for other in (none, zeros):
        out_o = list(other.rollout(acts)) + [other.scenario_returns, other.viol_T, other.n_steps_t]
        for x, y in zip(out_p, out_o):
            assert same_bits(x, y)
    # the window holds the parents' coming rows, once per scenario
    w_np, w_off, ts = parent_position(env)
    src = w_np[np.clip((w_off + ts)[:, None] + np.arange(H)[None, :], 0, len(w_np) - 1)]
    assert np_same_bits(zeros.weather_window.cpu().numpy(), np.broadcast_to(src[:, None], (B, S, H, env.nd)).copy())
    # without scenarios at all the new arguments are absent too
    a, b = env.planner(K, H, gamma=0.99), env.planner(K, H, gamma=0.99, weather_sigma=None, weather_phi=0.0)
    for x, y in zip(a.rollout(acts), b.rollout(acts)):
        assert same_bits(x, y)
    assert b.S is None and b.weather_window_t is None
    env.close()


# ---- 4. common random numbers ---------------------------------------------------------------------------------------------------------
def test_common_random_numbers_over_weather_futures():
    B, K, S, H = 2, 4, 5, 3
    env = started(B, "float32")
    acts = rand_actions((H, B, K, 6), 41, env.device)
    acts[:, :, 2] = acts[:, :, 0]                                          # candidates 0 and 2: the same action sequence
    plan = env.planner(K, H, n_scenarios=S, noise_scale=0.0, weather_sigma={"iGlob": 0.2, "tOut": 1.5, "vpOut": 0.1, "wind": 0.3, "tSky": 2.0},
                       weather_phi=PHI, scenario_seed=3)                   # weather-only scenarios
    assert plan.weather_sigma == [0.2, 1.5, 0.1, 0.0, 0.3, 2.0, 0.0] and plan.noise_scale == 0.0
    plan.rollout(acts)
    sr = plan.scenario_returns.clone()
    assert same_bits(sr[:, 0], sr[:, 2]) and not same_bits(sr[:, 0], sr[:, 1])
    assert not same_bits(sr[:, :, 0], sr[:, :, 1])                         # the scenarios of one candidate differ
    window = plan.weather_window_t.clone()
    plan.rollout(acts)
    assert same_bits(plan.scenario_returns, sr) and same_bits(plan.weather_window_t, window)       # fixed from rollout to rollout ...
    plan.new_scenarios()
    plan.rollout(acts)
    assert not same_bits(plan.scenario_returns, sr) and not same_bits(plan.weather_window_t, window)      # ... until new_scenarios()
    assert same_bits(plan.weather_window[:, :, 0], window.view(B, S, H, -1)[:, :, 0])       # the present row is a measurement in every future
    env.close()


# ---- 5. the parent is untouched; monotone under carry --------------------------------------------------------------------------------
def test_weather_scenario_cem_leaves_the_parent_untouched():
    B, K, S, H, E = 2, 16, 3, 3, 4
    env = started(B, "float32", uncertainty_scale=0.2)
    plan = env.planner(K, H, gamma=0.99, n_scenarios=S, n_tail=2, weather_sigma=SIGMA, weather_phi=PHI)
    state0, metrics0, flags0, weather0 = env.get_state(), env.metrics(), env.step_flags_t.clone(), env.weather_t.clone()
    rows0, table0 = env.weather_rows, env.weather_t.data_ptr()
    bests, mean_t, std_t = [], None, None
    for it in range(4):
        out = plan.cem(1, E, init_std=0.4, carry=2, beta=0.3, seed=8, mean_t=mean_t, std_t=std_t)
        mean_t, std_t = out["mean_sequence"], out["std_sequence"]
        bests.append(out["best_return"].cpu().numpy().copy())
        if it > 0:                                                          # candidate 1 IS the previous best, on the same futures
            assert same_f64(plan.ret_cand_t.view(B, K)[:, 1].cpu().numpy(), bests[it - 1])
            assert (bests[it] >= bests[it - 1]).all(), (it, bests)
    assert np.isfinite(np.array(bests)).all()
    plan.new_scenarios()
    plan.shift(0.5)
    same_state(env.get_state(), state0)
    assert env.metrics() == metrics0 and metrics0["n_env_steps"] == 2 * B
    assert same_bits(env.step_flags_t, flags0)
    assert same_bits(env.weather_t, weather0) and env.weather_rows == rows0 and env.weather_t.data_ptr() == table0
    env.close()


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------------------
def test_weather_scenario_cem_replays_from_a_captured_graph():
    import torch
    B, K, S, H, E = 2, 16, 3, 3, 4
    env = started(B, "float32", uncertainty_scale=0.2)
    plan = env.planner(K, H, gamma=0.99, n_scenarios=S, n_tail=2, weather_sigma=SIGMA, weather_phi=PHI)

    def decision():
        plan._draw = 0                        # the same draw indices every time; mean_t None resets the distribution
        return plan.cem(2, E, carry=1, beta=0.5, seed=3)

    def outputs():
        return [plan._actions, plan.ret_t, plan.ret_cand_t, plan.failed_cand_t, plan.steps_cand_t, plan.alive_cand_t, plan.viol_cand_T,
                plan.weather_window_t, plan.w_off_t, plan.cem_mean_t, plan.cem_std_t, plan.best_k_t, plan.best_ret_t, plan.best_action_t,
                plan.best_sequence_t, plan.elite_k_t[:B * E], plan.n_elite_t]

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
    assert not same_bits(replayed[1], eager[1]) and not same_bits(replayed[2], eager[2]) and not same_bits(replayed[7], eager[7])
    decision()                                                             # eager at the same base: the same bits again
    for t, e in zip(outputs(), replayed):
        assert same_bits(t, e)
    # the parent advances: the replay reads its new position from device memory
    env.step_tensor(rand_actions((B, 6), 77, env.device))
    graph.replay()
    torch.cuda.synchronize(env.device)
    moved = [t.clone() for t in outs]
    assert not same_bits(moved[7], replayed[7]) and not same_bits(moved[8], replayed[8])
    decision()                                                             # eager from the new parent state
    for t, e in zip(outputs(), moved):
        assert same_bits(t, e)
    w_np, w_off, ts = parent_position(env)
    window, child_off = np_wscen(B, K, S, H, w_np, w_off, ts, SIGMA, PHI, 0, 1)
    assert np_same_bits(moved[7].cpu().numpy(), window) and np.array_equal(moved[8].cpu().numpy(), child_off)
    env.close()


# ---- 7. the keyword checks -------------------------------------------------------------------------------------------------------------
def test_weather_sigma_keyword_checks():
    import torch
    env = started(2, "float32")
    K, H = 4, 3
    torch.cuda.synchronize(env.device)
    before = torch.cuda.memory_allocated(env.device)
    for kw in ({"weather_sigma": SIGMA},                                                       # without n_scenarios
               {"n_scenarios": 4, "weather_sigma": SIGMA[:6]}, {"n_scenarios": 4, "weather_sigma": SIGMA + [0.1]},
               {"n_scenarios": 4, "weather_sigma": [-0.1] + SIGMA[1:]}, {"n_scenarios": 4, "weather_sigma": [float("nan")] + SIGMA[1:]},
               {"n_scenarios": 4, "weather_sigma": [float("inf")] + SIGMA[1:]}, {"n_scenarios": 4, "weather_sigma": {"rain": 0.1}},
               {"n_scenarios": 4, "weather_sigma": 0.2}, {"n_scenarios": 4, "weather_sigma": SIGMA, "weather_phi": 1.0},
               {"n_scenarios": 4, "weather_sigma": SIGMA, "weather_phi": -0.1}):
        with pytest.raises(ValueError):
            env.planner(K, H, **kw)
    assert torch.cuda.memory_allocated(env.device) == before                                   # nothing was allocated
    plan = env.planner(K, H, n_scenarios=1, weather_sigma={"tOut": 1.5})                       # certainty-equivalent MPC on one wrong forecast
    assert plan.weather_sigma == [0.0, 1.5, 0.0, 0.0, 0.0, 0.0, 0.0] and plan.weather_phi == 0.0 and plan.weather_window.shape == (2, 1, H, env.nd)
    ret = plan.rollout(rand_actions((H, 2 * K, 6), 5, env.device))[0]
    assert same_bits(ret.view(-1), plan.ret_t) and torch.isfinite(ret).all()                   # S = 1: the score is the one scenario's return
    env.close()


# ---- 8. the example -------------------------------------------------------------------------------------------------------------------
def test_mpc_forecast_example_runs():
    r = subprocess.run([sys.executable, "examples/mpc_forecast.py", "--season", "0.25", "--candidates", "32", "--scenarios", "4", "--tail", "2",
                        "--horizon", "4", "--iters", "2", "--elites", "8"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"perfect forecast.*?closed-loop return ([-\d.e+]+).*?one wrong forecast.*?closed-loop return ([-\d.e+]+).*?"
                  r"4 forecast scenarios.*?closed-loop return ([-\d.e+]+)", r.stdout, flags=re.S)
    assert m, r.stdout
    assert all(np.isfinite(float(m.group(i))) for i in (1, 2, 3)) and "nan" not in r.stdout.lower()
