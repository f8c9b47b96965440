"""Closed-loop rule-based rollouts on the GPU: glgym_rule_rows, glgym_plan_rollout_rule (include/glgym.h) and gl_gym_amd.planner.RuleSearch.

What can be exact is compared bit for bit: a rollout against a loop over its parts from the same fork, the open-loop replay of its
recorded controls, record = 0 against record = 1, a CEM iteration against a rollout of its population, a captured graph against the
eager call, the parent before and after.  The comparisons with a tolerance are the controller's: RULE_RTOL = 1e-12 / RULE_ATOL = 1e-14
on fp64 handles (tests/envlayer_inputs.py) and 2e-5 absolute on fp32 handles, the fp32 bound of tests/test_gpu_rule_based_configs.py
(the inputs and the stored controls are rounded to float32; the controls lie in [0, 1]).
Child batches stay <= 260 rows and horizons <= 6 steps."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import envlayer_inputs as E
from test_gpu_plan import make_env, same_bits, same_state
from test_gpu_plan_scen import handle_crop
from test_plan_rule_host import CONFIGS, NF, NU, bracket, make_space, mixed_batch, np_decode, theta_of
from test_plan_scen_host import np_scen_crop, py_aggregate, same_f64

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
PAD = 3                                                          # ld = B + PAD
F32_BOUND = 2e-5
# symmetric around the defaults: encode(RuleBasedController()) is theta = 0 and decodes to the defaults exactly
TUNE = {"temp_setpoint_day": (16.5, 22.5), "temp_setpoint_night": (13.5, 19.5), "co2_day": (400.0, 1200.0), "rh_max": (75.0, 95.0),
        "lamps_off": (14.0, 22.0), "tHeatBand": (-1.5, -0.5), "heat_deadzone": (3.0, 7.0)}           # D = 7: Ht = 2, five padding entries


@pytest.fixture(scope="module")
def handles():
    hs = {False: E.Handle(False), True: E.Handle(True)}
    yield hs
    for h in hs.values():
        h.close()


def close(got, ref, f64):
    if f64:
        return np.allclose(got, ref, rtol=E.RULE_RTOL, atol=E.RULE_ATOL)
    return np.abs(got - ref).max() < F32_BOUND


def rule_buffers(hd, X, D, ts, sday, hour=None, doy=None):
    """Guarded inputs of one controller call: row b holds X[b] and reads weather row b mod len(D)."""
    B = len(X)
    ld, rows = B + PAD, len(D)
    w_off = (np.arange(B) % rows - ts).astype(np.int32)
    ins = dict(x=E.Guarded(E.soa(X, ld, hd.T)), weather=E.Guarded(np.asarray(D, dtype=hd.T)), w_off=E.Guarded(w_off),
               timestep=E.Guarded(np.asarray(ts, dtype=np.int32)), start_day=E.Guarded(np.asarray(sday, dtype=np.float32)),
               hour=E.Guarded(np.asarray(hour, dtype=np.float64)) if hour is not None else None,
               doy=E.Guarded(np.asarray(doy, dtype=np.float64)) if doy is not None else None)
    return B, ld, rows, ins


def rule_args(hd, B, ld, rows, ins, ctl):
    p = lambda k: ins[k].ptr if ins[k] is not None else None  # noqa: E731
    return hd.L.RuleArgs(B, ld, p("x"), p("weather"), rows, p("w_off"), p("timestep"), p("start_day"), p("hour"), p("doy"), ctl.ptr)


def read_controls(ctl, B):
    out = ctl.read()
    assert np.all(np.ascontiguousarray(out[:, B:]).view(np.uint8) == 0xFF), "a guard row of the control block was written"
    assert not np.isnan(out[:, :B]).any(), "a NaN (padding, or a row nobody wrote) reached the controls"
    return out[:, :B].T.astype(np.float64)


def run_rows(hd, space, theta, J, S, bufs):
    B, ld, rows, ins = bufs
    ctl, th = E.Guarded(shape=(6, ld), dtype=hd.T), E.Guarded(theta)
    a = hd.L.make_plan_args(hd.L.RuleRowsArgs, J, S, rule_args(hd, B, ld, rows, ins, ctl), space, th.ptr)
    hd.sync()
    rc = hd.lib.glgym_rule_rows(hd.h, C.byref(a), hd.stream())
    hd.sync()
    assert rc == 0, (rc, hd.error())
    th.read()                                                    # its guards
    return read_controls(ctl, B)


def run_based(hd, cfg, bufs):
    B, ld, rows, ins = bufs
    ctl = E.Guarded(shape=(6, ld), dtype=hd.T)
    a = rule_args(hd, B, ld, rows, ins, ctl)
    c = hd.L.RuleCfg(*[float(v) for v in cfg])
    hd.sync()
    rc = hd.lib.glgym_rule_based(hd.h, C.byref(c), C.byref(a), hd.stream())
    hd.sync()
    assert rc == 0, (rc, hd.error())
    return read_controls(ctl, B)


# ---- 1. the rows kernel against the existing kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("name", CONFIGS)
def test_rows_kernel_against_the_existing_kernel(handles, golden, name, f64):
    hd, g = handles[f64], golden("controller_kat_configs")
    values = np.asarray(g[f"{name}_cfg"], dtype=np.float64)
    for B in E.RULE_BATCHES:
        idx = np.arange(B) % len(g["X"])
        bufs = rule_buffers(hd, g["X"][idx], g["D"], g[f"{name}_timestep"][idx], g[f"{name}_start_day"][idx])       # derived clocks
        for fields in (np.arange(NF), np.array([6, 7, 10, 26])):     # all 29 tuned; four, the other 25 (lamp hours among them) from base
            lo, hi = bracket(values, fields, seed=len(fields))
            theta, decoded = theta_of(values, fields, lo, hi, B)
            got = run_rows(hd, make_space(values, fields, lo, hi), theta, B, 0, bufs)
            ref = run_based(hd, decoded, bufs)
            err = np.abs(got - ref).max()
            print(f"{name} B={B} D={len(fields)}: {err:.3g}")
            assert close(got, ref, f64), (name, B, len(fields), err)


# ---- 2. per-row parameters --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_per_row_parameters(handles, golden, f64):
    from gl_gym_amd.baseline import RuleBasedController
    hd, g = handles[f64], golden("controller_kat_configs")
    B, S, J = 130, 3, 44
    rng = np.random.default_rng(44)
    vals, Xm, Dm, hour_m, doy_m = mixed_batch(g)
    n_mixed = len(vals)
    fields = np.array([0, 1, 2, 3, 6])
    lo, hi = np.array([0.0, 0.0, -1.0, 0.0, 15.0]), np.array([24.0, 24.0, 366.0, 366.0, 25.0])
    theta = rng.uniform(-1.0, 1.0, (1, J, NU)).astype(np.float32)
    theta[0, :n_mixed, :5] = (2.0 * (vals[:, fields] - lo) / (hi - lo) - 1.0).astype(np.float32)
    theta[0, :, 5] = np.nan                                      # padding
    row = np.arange(B) // S
    X = np.array(g["X"][np.arange(B) % len(g["X"])])
    X[:, 2] += rng.uniform(-0.5, 0.5, B)                         # no two rows in one state
    D = np.array(g["D"][np.arange(B) % len(g["D"])])
    hour, doy = rng.uniform(0, 24, B), rng.uniform(0, 365, B)
    mixed = row < n_mixed
    X[mixed], D[mixed], hour[mixed], doy[mixed] = Xm[row[mixed]], Dm[row[mixed]], hour_m[row[mixed]], doy_m[row[mixed]]
    X[mixed, 2] += 0.01 * (np.arange(B)[mixed] % S)
    ts, sday = np.arange(B, dtype=np.int32) % 50, np.zeros(B, dtype=np.float32)
    base = vals[0]
    got = run_rows(hd, make_space(base, fields, lo, hi), theta, J, S, rule_buffers(hd, X, D, ts, sday, hour, doy))

    def reference(rows_of):
        cfg = np_decode(base, fields, lo, hi, theta, 1, J)[rows_of]
        Xr, Dr = E.rounded(X, f64), E.rounded(D, f64)
        return np.array([RuleBasedController(**dict(zip(hd.L.RULE_FIELDS, cfg[b]))).predict(Xr[b:b + 1], Dr[b:b + 1], hour[b:b + 1], doy[b:b + 1])[0]
                         for b in range(B)])

    ref = reference(row)
    assert close(got, ref, f64), np.abs(got - ref).max()
    assert {bool(v > 0) for v in ref[mixed, 4]} == {False, True}     # the lamp comparisons went both ways inside one wavefront
    wrong = reference(np.minimum(np.arange(B), J - 1))               # had row b read theta row b, not b / 3
    assert np.abs(got - wrong).max() > 1e-3


# ---- helpers of the rollout tests ---------------------------------------------------------------------------------------------------
def started(B, dtype, n=2, **kw):
    from gl_gym_amd.baseline import RuleBasedController
    env = make_env(B, dtype, **kw)
    env.reset_tensor()
    for _ in range(n):
        env.step_tensor(controller=RuleBasedController(), want_obs=False)
    return env


def rand_theta(rs, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(rs.Ht, rs.J, 6, generator=g) * 2 - 1).to(device=rs.env.device, dtype=torch.float32).contiguous()


CHILD = ("ret_t", "viol_T", "n_steps_t", "alive_t", "failed_t", "x_T", "u_T", "timestep_t")


def snapshot(p):
    return {k: getattr(p, k).clone() for k in CHILD}


def assert_same_children(a, b, keys=CHILD):
    for k in keys:
        assert same_bits(a[k], b[k]), k


def parts_loop(rs, theta_t):
    """From a fresh fork: H x (glgym_rule_rows -> glgym_step with that control plane -> glgym_plan_accumulate), called one by one.
    -> (the children afterwards, the control planes [H, C, 6])."""
    import torch
    from gl_gym_amd import _lib as L
    p, e = rs.plan, rs.env
    lib, h, st = e._lib, e._h, e._stream()
    p.fork()
    plane = torch.zeros(6, p.ld, dtype=e.tdtype, device=e.device)
    w, planes = 1.0, []
    for _ in range(rs.H):
        rule = L.RuleArgs(p.C, p.ld, p.x_T.data_ptr(), e.weather_t.data_ptr(), e.weather_rows, p.w_off_t.data_ptr(), p.timestep_t.data_ptr(),
                          p.start_day_t.data_ptr(), None, None, plane.data_ptr())
        a = L.make_plan_args(L.RuleRowsArgs, p.J, 0, rule, rs._space, theta_t.data_ptr())
        assert lib.glgym_rule_rows(h, C.byref(a), st) == L.OK, lib.glgym_last_error()
        planes.append(plane[:, :p.C].t().clone())
        s = p._step_args()
        s.control = plane.data_ptr()
        assert lib.glgym_step(h, C.byref(s), st) == L.OK, lib.glgym_last_error()
        acc = L.make_plan_args(L.PlanAccumulateArgs, p.C, p.ld, w, p.reward_t.data_ptr(), p.info_T.data_ptr(), p.done_t.data_ptr(),
                               p.step_flags_t.data_ptr(), p.ret_t.data_ptr(), p.viol_T.data_ptr(), p.n_steps_t.data_ptr(), p.alive_t.data_ptr(),
                               p.failed_t.data_ptr())
        assert lib.glgym_plan_accumulate(h, C.byref(acc), st) == L.OK
        w = w * p.gamma
    return snapshot(p), torch.stack(planes)


# ---- 3. a rollout equals its parts, 4. open-loop replay ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("B,K,H", [(2, 5, 4), (5, 13, 3)])       # C = 65: the second wavefront holds one child
def test_a_rollout_equals_its_parts_and_replays_open_loop(B, K, H, dtype):
    env = started(B, dtype)
    rs = env.rule_search(K, H, tune=TUNE, gamma=0.97)
    assert (rs.D, rs.Ht, rs.C) == (7, 2, B * K)
    theta = rand_theta(rs, 5)
    out = [t.clone() for t in rs.rollout(theta, record=True)]
    rolled, controls = snapshot(rs.plan), rs.controls.clone()
    assert rs.controls_T.shape == (H, 6, rs.plan.ld) and controls.shape == (H, B * K, 6)
    parts, planes = parts_loop(rs, theta)
    assert_same_children(rolled, parts)
    assert same_bits(controls.contiguous(), planes)
    ret, alive, steps, viol, failed = out
    assert ret.shape == (B, K) and viol.shape == (3, B, K) and int(steps.min()) == H and bool(alive.all()) and not bool(failed.any())
    assert all(len(np.unique(r)) > K // 2 for r in ret.cpu().numpy())        # the candidate controllers earn returns of their own
    # record = 0: one plane, the same children
    rs.rollout(theta)
    assert_same_children(snapshot(rs.plan), rolled)
    assert same_bits(rs._plane_T[0, :, :rs.C].t().contiguous(), planes[-1])
    # the recorded controls, replayed open-loop by the planner as it was
    plan = env.planner(K, H, gamma=0.97)
    replay = plan.rollout(controls_t=controls)
    for a, b in zip(replay, out):
        assert same_bits(a, b)
    assert_same_children(snapshot(plan), rolled)
    env.close()


# ---- 5. clocks and feedback ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_clocks_and_feedback(dtype):
    from gl_gym_amd.baseline import RuleBasedController
    B, K, H = 3, 2, 2
    c = RuleBasedController()
    env = make_env(B, dtype)
    env.reset_tensor()
    env.x_T[2, 1] += 1.5                                         # air temperature: three greenhouses in three states, whatever start
    env.x_T[2, 2] -= 1.0                                         # row each one drew
    for _ in range(3):                                           # three step_tensor(controller=c) steps of the parent
        env.step_tensor(controller=c, want_obs=False)
    rs = env.rule_search(K, H, tune=TUNE, base=c)
    theta = rs.theta_of(c)
    assert (theta == 0).all()                                    # TUNE is symmetric around the defaults: they decode exactly
    rs.rollout(theta, record=True)
    first = rs.controls[0].double().cpu().numpy()                # [C, 6]
    ref = env.rule_based_controls(c).double().cpu().numpy()      # [B, 6]
    assert close(first, np.repeat(ref, K, axis=0), dtype == "float64"), np.abs(first - np.repeat(ref, K, axis=0)).max()
    # greenhouses in different states (three start rows) get different controls from the same theta, and the controls follow the state
    assert np.abs(first[0] - first[K]).max() > 1e-6 and np.abs(first[K] - first[2 * K]).max() > 1e-6
    second = rs.controls[1].double().cpu().numpy()
    assert np.abs(second - first).max() > 1e-9
    env.close()


# ---- 6. season end inside the horizon ---------------------------------------------------------------------------------------------------
def test_season_end_inside_the_horizon():
    B, K, H = 2, 5, 6
    env = started(B, "float32")
    env.timestep_t.fill_(env.N - 2)                              # two steps from the last step
    rs = env.rule_search(K, H, tune=TUNE, gamma=0.97)
    theta = rand_theta(rs, 6)
    ret, alive, steps, viol, failed = rs.rollout(theta)
    rolled = snapshot(rs.plan)
    n = steps.cpu().numpy()
    assert not bool(alive.any()) and (n == n[0, 0]).all() and 1 <= n[0, 0] < H, n
    parts, _ = parts_loop(rs, theta)
    assert_same_children(rolled, parts)
    short = env.rule_search(K, int(n[0, 0]), tune=TUNE, gamma=0.97)      # the step that reports done was the last one counted
    assert same_bits(short.rollout(theta)[0], ret) and not bool(short.plan.alive_t.any())
    env.close()


# ---- 7. scenarios ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", ["step", "hold"])
def test_scenarios(noise):
    B, K, S, H, scale, seed = 2, 4, 3, 3, 0.2, 0xDEADBEEF12345678
    env = started(B, "float32")
    kw = dict(n_scenarios=S, noise=noise, noise_scale=scale, scenario_seed=seed, gamma=0.97)
    rs = env.rule_search(K, H, tune=TUNE, n_tail=1, **kw)
    rs.new_scenarios()                                           # scenario draw index 1
    theta = rand_theta(rs, 7)
    theta[:, 1] = theta[:, 0]                                    # candidates 0 and 1 of greenhouse 0: the same controller
    ret, alive, steps, viol, failed = [t.clone() for t in rs.rollout(theta)]
    p = rs.plan
    n = B * K * S
    assert p.C == n and rs.scenario_returns.shape == (B, K, S)
    # the crop blocks are glgym_plan_scenario's: the last step's is still in the children's buffer
    exp = np_scen_crop(B, K, S, H - 1, noise == "hold", scale, seed, 1, handle_crop(env))
    assert np.array_equal(p.crop_T[:, :n].cpu().numpy().view(np.uint32), exp.view(np.uint32))
    import torch
    from gl_gym_amd import _lib as L
    crop_t = torch.full_like(p.crop_T, 7.0)
    a = L.make_plan_args(L.PlanScenarioArgs, B, K, S, p.ld, H - 1, 1 if noise == "hold" else 0, scale, seed, 1, p.scenario_base_t.data_ptr(),
                         crop_t.data_ptr(), None, None)
    assert env._lib.glgym_plan_scenario(env._h, C.byref(a), env._stream()) == L.OK
    assert same_bits(crop_t[:, :n], p.crop_T[:, :n])
    sr, sf = rs.scenario_returns.cpu().numpy(), rs.scenario_failed.cpu().numpy()
    assert same_f64(sr[0, 0], sr[0, 1]) and not np.array_equal(sr[0, 0], sr[0, 2])
    assert not np.array_equal(sr[:, :, 0], sr[:, :, 1])          # the futures really differ
    vi, ns = p.viol_T[:, :n].cpu().numpy(), p.n_steps_t.cpu().numpy()
    for n_tail, got in ((1, (ret, steps, viol, failed)), (S, None)):
        if got is None:
            other = env.rule_search(K, H, tune=TUNE, n_tail=n_tail, **kw)
            other.new_scenarios()
            o = other.rollout(theta)
            got = (o[0], o[2], o[3], o[4])
            assert same_bits(other.scenario_returns, rs.scenario_returns)
        e_rc, e_fc, e_vc, e_sc = py_aggregate(B * K, S, n_tail, sr.reshape(-1), sf.reshape(-1), vi, ns)
        assert same_f64(got[0].cpu().numpy().reshape(-1), e_rc) and np.array_equal(got[3].cpu().numpy().reshape(-1), e_fc)
        assert same_f64(got[2].cpu().numpy().reshape(3, -1), e_vc) and np.array_equal(got[1].cpu().numpy().reshape(-1), e_sc)
    assert not bool(failed.any()) and bool(alive.all())
    # weather windows with sigma = 0 hold the parents' own rows: the same returns
    windows = env.rule_search(K, H, tune=TUNE, n_tail=1, weather_sigma=[0.0] * 7, weather_phi=0.5, **kw)
    windows.new_scenarios()
    windows.rollout(theta)
    assert same_bits(windows.scenario_returns, rs.scenario_returns) and windows.plan.weather_window is not None
    env.close()


# ---- 8. the cross-entropy method -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_cem(dtype):
    import torch
    B, K, H, E_, n_iter = 3, 8, 3, 3, 3
    env = started(B, dtype)
    rs = env.rule_search(K, H, tune=TUNE, gamma=0.97)
    out = rs.cem(1, E_, init_std=0.4, carry=1, seed=9)
    block, ret = rs._theta.clone(), rs.plan.ret_t.clone()
    other = env.rule_search(K, H, tune=TUNE, gamma=0.97)
    assert same_bits(other.rollout(block)[0].reshape(-1), ret)   # an iteration's returns are rollout() of the sampled block
    cand0 = block.view(rs.Ht, B, K, 6)[:, :, 0]
    assert (cand0 == 0).all()                                    # candidate 0 is the clipped mean: encode(base) = 0
    assert float(block.abs().max()) <= 1.0 and float(block.view(rs.Ht, B, K, 6)[:, :, 1:].abs().max()) > 0
    sel = other.select()
    for k in ("best_k", "best_return", "best_theta"):
        assert same_bits(sel[k], out[k]), k
    # stage by stage with one carried elite: the best return never decreases, the carried elite keeps its score
    stages = env.rule_search(K, H, tune=TUNE, gamma=0.97)
    stages.mean_t.zero_()
    stages.std_t.fill_(0.4)
    bests = []
    for it in range(n_iter):
        pop = stages.sample(stages.mean_t, stages.std_t, seed=9, draw_index=it, carry=1)
        stages.rollout(pop)
        stages.elites(E_)
        stages.refit(stages.mean_t, stages.std_t, 0.1, 0.05)
        bests.append(stages.select()["best_return"].cpu().numpy().copy())
        if it > 0:                                               # candidate 1 IS the previous best, rolled out from the same fork
            assert np.array_equal(stages.plan.ret_t.view(B, K)[:, 1].cpu().numpy().view(np.uint64), bests[it - 1].view(np.uint64))
            assert (bests[it] >= bests[it - 1]).all(), (it, bests)
    whole = env.rule_search(K, H, tune=TUNE, gamma=0.97).cem(n_iter, E_, init_std=0.4, carry=1, seed=9)
    assert np.array_equal(whole["best_return"].cpu().numpy().view(np.uint64), bests[-1].view(np.uint64)) and np.isfinite(bests).all()
    # best_theta decodes to best_params, and a controller comes out of it
    dec = rs.decode(out["best_theta"].view(B, rs.Ht, 6).permute(1, 0, 2))
    for name in TUNE:
        assert same_bits(dec[name].contiguous(), out["best_params"][name].contiguous()), name
        v = out["best_params"][name].cpu().numpy()
        assert (v >= TUNE[name][0]).all() and (v <= TUNE[name][1]).all()
    ctrl = rs.best_controller(1)
    assert ctrl.co2_day == float(out["best_params"]["co2_day"][1]) and ctrl.lamps_on == 0
    assert out["mean"].shape == out["std"].shape == (rs.Ht, B, 6) and out["elite_k"].shape == (B, E_)
    assert float(out["std"].min()) >= 0.05 and torch.isfinite(out["mean"]).all()
    env.close()


def test_cem_replays_from_a_captured_graph():
    import torch
    B, K, H, E_ = 3, 8, 3, 3
    env = started(B, "float32")
    rs = env.rule_search(K, H, tune=TUNE, gamma=0.97)

    def decision():
        rs._draw = 0                          # the same draw indices every time: what differs between runs is draw_base_t alone
        return rs.cem(2, E_, carry=1, seed=3)

    def outputs():
        return [rs._theta, rs.plan.ret_t, rs.mean_t, rs.std_t, rs.plan.best_k_t, rs.plan.best_ret_t, rs.best_theta_t, rs._params_T,
                rs.elite_k_t[:B * E_], rs.n_elite_t]

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
    rs.plan.draw_base_t += 2                  # the device word behind draw_base moves: the replay samples another population
    graph.replay()
    torch.cuda.synchronize(env.device)
    replayed = [t.clone() for t in outs]
    assert not same_bits(replayed[0], eager[0]) and not same_bits(replayed[1], eager[1])
    decision()                                # eager at the same draw_base: the same bits again
    for t, e in zip(outputs(), replayed):
        assert same_bits(t, e)
    env.close()


# ---- 9. the parent is only read ---------------------------------------------------------------------------------------------------------------
def test_cem_leaves_the_parent_untouched():
    B, K, H = 3, 8, 3
    env = started(B, "float32", uncertainty_scale=0.2)           # the parent has a crop block of its own
    rs = env.rule_search(K, H, tune=TUNE, n_scenarios=2)
    state0, metrics0, flags0, crop0 = env.get_state(), env.metrics(), env.step_flags_t.clone(), env.crop_T.clone()
    rs.cem(2, 3, carry=1)
    rs.rollout(rand_theta(rs, 1), record=True)
    same_state(env.get_state(), state0)
    assert env.metrics() == metrics0 and metrics0["n_env_steps"] == 2 * B
    assert same_bits(env.step_flags_t, flags0) and same_bits(env.crop_T, crop0)
    env.close()


# ---- the boundary's checks on a live handle -------------------------------------------------------------------------------------------
def test_rollout_rule_refuses_what_glgym_step_refuses_and_python_checks_its_arguments():
    import torch
    from gl_gym_amd import _lib as L
    from gl_gym_amd.baseline import RuleBasedController
    B, K, H = 2, 3, 2
    env = started(B, "float32")
    rs = env.rule_search(K, H, tune=TUNE)
    theta = rand_theta(rs, 2)
    rs.rollout(theta)
    p = rs.plan
    lib, h, st = env._lib, env._h, env._stream()

    def args():
        r = L.make_plan_args(L.PlanRolloutArgs, H, 1.0, p._step_args(), None, rs._plane_T.data_ptr(), p.ret_t.data_ptr(), p.viol_T.data_ptr(),
                             p.n_steps_t.data_ptr(), p.alive_t.data_ptr(), p.failed_t.data_ptr())
        return L.make_plan_args(L.PlanRolloutRuleArgs, 0, r, rs._space, theta.data_ptr(), p.start_day_t.data_ptr(), p.J, 0, 0, 0, 0, 0.0, 0, 0, None)

    p.fork()
    assert lib.glgym_plan_rollout_rule(h, C.byref(args()), st) == L.OK
    before = [t.clone() for t in (rs._plane_T, p.ret_t, p.x_T, p.timestep_t)]
    a = args()
    a.rollout.step.x = None                                      # glgym_step's own check, in its own words, nothing launched
    assert lib.glgym_plan_rollout_rule(h, C.byref(a), st) == L.EINVAL and b"glgym_step" in lib.glgym_last_error()
    assert lib.glgym_set_integrator(h, L.INTEGRATORS["bdf"]) == L.OK       # a BDF glgym_evalF setting on explicit steps
    assert lib.glgym_plan_rollout_rule(h, C.byref(args()), st) == L.EINVAL and b"glgym_step" in lib.glgym_last_error()
    assert lib.glgym_set_integrator(h, L.INTEGRATORS["explicit"]) == L.OK
    a = args()
    a.space.base.co2Band = 0.0                                   # an untuned band that glgym_rule_based would refuse
    assert lib.glgym_plan_rollout_rule(h, C.byref(a), st) == L.EINVAL and b"zero proportional band" in lib.glgym_last_error()
    torch.cuda.synchronize(env.device)
    for t, b in zip((rs._plane_T, p.ret_t, p.x_T, p.timestep_t), before):
        assert same_bits(t, b)
    with pytest.raises(ValueError, match="values"):
        rs.rollout(theta[:1])
    with pytest.raises(ValueError, match="unknown"):
        env.rule_search(K, H, tune={"temp_setpoint_noon": (1, 2)})
    with pytest.raises(ValueError, match="at least one"):
        env.rule_search(K, H, tune={})
    with pytest.raises(ValueError, match="outside"):
        rs.encode(RuleBasedController(co2_day=5000))
    with pytest.raises(TypeError):
        env.rule_search(K, H, tune=TUNE, crop="current")
    env.close()
    slow = make_env(2, "float32", dt=300.0, pred_horizon=0.25)   # the 300 s steps of the reference's run-time experiment
    with pytest.raises(ValueError, match="450"):
        slow.rule_search(K, H, tune=TUNE)
    slow.close()


# ---- 10. the example ---------------------------------------------------------------------------------------------------------------------------
def test_tune_rule_based_example_runs():
    r = subprocess.run([sys.executable, "examples/tune_rule_based.py", "--envs", "2", "--candidates", "8", "--horizon", "4", "--iters", "2",
                        "--elites", "3", "--carry", "1"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    m = re.search(r"default controller: return over the horizon ([-\d.e+]+).*?tuned controller  : return over the horizon ([-\d.e+]+)", r.stdout,
                  flags=re.S)
    assert m, r.stdout
    assert np.isfinite(float(m.group(1))) and np.isfinite(float(m.group(2))) and float(m.group(2)) >= float(m.group(1))
    assert "temp_setpoint_day" in r.stdout and "without an admissible candidate: 0" in r.stdout and "nan" not in r.stdout.lower()
