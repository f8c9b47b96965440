"""GPU tests of the BDF env-step (glgym_set_step_integrator / TomatoVecEnv(integrator="bdf")): the same bits as glgym_evalF's BDF on the
same inputs, the action path against the reference env's semantics, the hold-outs free-running, the failure contract, switching, graph
capture and the env seams."""
import ctypes as C

import numpy as np
import pytest

from conftest import judge_rollout
from test_gpu_holdout import PLAIN_BOUND, make_env, rollout
from test_make_env import cfg_dir  # noqa: F401  (fixture: a config directory in the reference's layout)

pytestmark = pytest.mark.gpu


def gl(dtype="float64", tol=1e-6, **kw):
    from gl_gym_amd import GreenLight
    m = GreenLight(28, 6, 10, 208, 900.0, dtype=dtype, integrator="bdf", rtol=tol, atol=tol, **kw)
    return m


def env_step(m, x, u_prev, w, control=None, action=None, crop=None, timestep=None, step_bdf=True, dtype="float64"):
    """One glgym_step of B environments (environment b on weather row b) on a GreenLight handle; -> dict of host arrays."""
    import torch
    from gl_gym_amd import _lib as L
    if step_bdf:
        L.check(m._lib.glgym_set_step_integrator(m.handle, 1))
    B = x.shape[0]
    T = torch.float64 if dtype == "float64" else torch.float32
    dev = torch.device("cuda:0")
    t = dict(dtype=T, device=dev)
    X = torch.as_tensor(x.T.copy(), **t).contiguous(); Uu = torch.as_tensor(u_prev.T.copy(), **t).contiguous()
    Ctl = torch.as_tensor(control.T.copy(), **t).contiguous() if control is not None else None
    Act = torch.as_tensor(action, dtype=torch.float32, device=dev).contiguous() if action is not None else None
    Wt = torch.as_tensor(w, **t).contiguous()
    Cr = torch.as_tensor(crop.T.copy(), **t).contiguous() if crop is not None else None
    w_off = torch.arange(B, dtype=torch.int32, device=dev)
    ts = torch.as_tensor(np.zeros(B) if timestep is None else timestep, dtype=torch.int32, device=dev)
    rew = torch.zeros(B, **t); info = torch.zeros(11, B, **t); done = torch.zeros(B, dtype=torch.uint8, device=dev)
    met = torch.zeros(L.METRIC_REPLICAS, L.METRIC_STRIDE, dtype=torch.float32, device=dev)
    flags = torch.zeros(B, dtype=torch.int32, device=dev)
    a = L.make_step_args(B, B, X.data_ptr(), Uu.data_ptr(), Act.data_ptr() if Act is not None else None,
                         Ctl.data_ptr() if Ctl is not None else None, Wt.data_ptr(), Wt.shape[0], w_off.data_ptr(), ts.data_ptr(),
                         Cr.data_ptr() if Cr is not None else None, 96, rew.data_ptr(), info.data_ptr(), done.data_ptr(), met.data_ptr(),
                         flags.data_ptr())
    rc = m._lib.glgym_step(m.handle, C.byref(a), None)
    torch.cuda.synchronize()
    h = lambda v: v.cpu().numpy().copy()  # noqa: E731
    return dict(rc=rc, x=h(X.T).astype(np.float64), u=h(Uu.T), reward=h(rew), info=h(info.T), done=h(done), ts=h(ts), flags=h(flags),
                metrics=met.double().sum(dim=0).cpu().numpy())


def exact_time(x0, ts, dt=900.0):
    per = dt / 86400.0
    t0 = x0[:, 27] - ts * per
    t0[np.abs(t0) < 5e-4] = 0.0
    return t0 + (ts + 1.0) * per


def test_same_bits_as_evalf(golden):
    from gl_gym_amd import _lib as L
    for name in ("holdout_gl2010_random", "step_tight"):
        g = golden(name)
        if name == "step_tight":
            X, U, W = g["X"][:64], g["U"][:64], g["D"][:64]
        else:
            X, U, W = g["X"][:64], g["U"][:64], g["weather"][:64]
        m = gl()
        ref = m.evalF_batch(X, U, W)
        steps = m.solver_stats()["steps"]
        r = env_step(m, X, np.zeros_like(U), W, control=U)
        assert r["rc"] == L.OK
        assert np.array_equal(r["x"][:, :27], ref[:, :27]), name
        assert np.array_equal(r["x"][:, 27], exact_time(X, np.zeros(64)))
        assert np.array_equal(r["u"], U)
        assert np.array_equal(r["flags"], L.SF_BDF | (steps << 16)) and steps.min() >= 1
        assert r["metrics"][3] == 0 and r["metrics"][7] == 64 and r["metrics"][L.METRIC_BDF] == steps.sum()
        assert np.all(r["metrics"][8:14] == 0)
        m.close()
        # fp32 handle: the integration in fp64 from the float32 inputs, stored in float32
        x32, u32, w32 = (np.float32(v) for v in (X, U, W))
        m32 = gl("float32")
        ref32 = np.float32(m32.evalF_batch(np.float64(x32), np.float64(u32), np.float64(w32)))
        r32 = env_step(m32, np.float64(x32), np.zeros_like(U), np.float64(w32), control=np.float64(u32), dtype="float32")
        assert np.array_equal(np.float32(r32["x"][:, :27]), ref32[:, :27]), name
        m32.close()
    # per-env crop blocks against evalF with per-row p (row 0 keeps the handle's block)
    g = golden("holdout_gl2010_noisy")
    X, U, W, Pc = g["X"][0, :48], g["U"][0, :48], g["weather"][:48], g["P_crop"][0, :48].astype(np.float64)
    from gl_gym_amd.parameters import init_default_params
    p0 = np.asarray(init_default_params(208), dtype=np.float64)      # the handle's block
    Pc[0] = p0[128:162]
    P = np.repeat(p0[None], 48, axis=0)
    P[:, 128:162] = Pc
    m = gl()
    ref = m.evalF_batch(X, U, W, P)
    r = env_step(m, X, np.zeros_like(U), W, control=U, crop=Pc)
    assert r["rc"] == L.OK and np.array_equal(r["x"][:, :27], ref[:, :27])
    m.close()


def _vec(g, integrator="bdf", **kw):
    from gl_gym_amd.tomato_env import TomatoVecEnv
    return TomatoVecEnv(1, weather=g["weather"], params=g["p"], dtype="float64", season_length=1, start_rows=[0], start_days=[0.0],
                        auto_reset=False, integrator=integrator, **kw)


@pytest.mark.parametrize("drive", ["actions", "rule_based"])
def test_env_step_against_the_reference_env_over_device_evalf(golden, drive):
    """97 steps (a whole 1-day episode) of one env, teacher-forced: the reference env restated (OracleTomatoEnv) with the device's
    evalF-BDF as its evalF.  drive = "actions": step() with refenv_1day's actions, the applied control also against the explicit env's
    bit for bit.  drive = "rule_based": step_rule_based() -- the controller on the device, then the raw-control env-step (verified mode
    in the explicit path) -- with the oracle env's step_raw_control given the control the device applied."""
    from oracle.gl_env_oracle import OracleReward, OracleTomatoEnv
    from gl_gym_amd._lib import INFO_KEYS
    from gl_gym_amd.baseline import RuleBasedController
    g = golden("refenv_1day")
    acts = g["ra_actions"][:97]
    ctrl = RuleBasedController()
    env, exp = _vec(g), _vec(g, integrator="explicit")
    env.reset(); exp.reset()
    p64 = np.asarray(env.p, dtype=np.float64)
    m = gl()
    o = OracleTomatoEnv(g["weather"], g["p"], season_length=1, dt=900.0, train_days=(0,), start_day=0)
    o._evalF = lambda x, u, d, p: m.evalF_batch(np.asarray(x)[None], np.asarray(u)[None], np.asarray(d)[None], p64[None])[0]
    o.reset(seed=0)
    o.p = p64
    o.reward = OracleReward(o)
    x_prev = env.x[0].double().cpu().numpy()
    o.x = x_prev.copy()
    u_seen = []
    for k in range(len(acts)):
        o.x, o.x_prev = x_prev.copy(), x_prev.copy()
        if drive == "actions":
            exp.x_T[:, 0] = env.x_T[:, 0]; exp.u_T[:, 0] = env.u_T[:, 0]; exp.timestep_t.copy_(env.timestep_t)
            obs, r, d, infos = env.step(acts[k][None])
            exp.step(acts[k][None])
            u_dev = env.u[0].double().cpu().numpy()
            assert np.array_equal(u_dev, exp.u[0].double().cpu().numpy()), k           # action_to_control bit for bit
            o_obs, o_r, o_term, o_info = o.step(acts[k])
        else:
            obs, r, d, infos = env.step_rule_based(ctrl)
            u_dev = env.u[0].double().cpu().numpy()
            assert np.array_equal(u_dev, env.ctrl_T[:, 0].double().cpu().numpy()), k   # the raw control, applied unclipped
            o_obs, o_r, o_term, o_info = o.step_raw_control(u_dev)
        u_seen.append(u_dev)
        x_dev = env.x[0].double().cpu().numpy()
        assert np.array_equal(u_dev, o.u) and np.array_equal(x_dev[:27], np.asarray(o.x)[:27]), k
        assert bool(d[0]) == bool(o_term) and int(env.timestep_t[0]) == o.timestep == k + 1
        r_dev = float(env.reward_t[0])                        # (the SB3 path hands rewards out as float32)
        assert abs(r_dev - o_r) <= 1e-12 * max(abs(o_r), 1.0), (k, r_dev, o_r)
        for q, key in enumerate(INFO_KEYS):
            assert abs(infos[0][key] - o_info[key]) <= 1e-12 * max(abs(o_info[key]), 1e-3), (k, key)
        np.testing.assert_allclose(obs[0], np.float32(o_obs), rtol=2e-6, atol=2e-6)
        assert infos[0]["integration"] & 2048
        x_prev = x_dev
    assert env.solver_metrics()["bdf_steps"] > 0 and env.metrics()["n_env_steps"] == len(acts)
    assert env.metrics()["n_ode_fail"] == 0 and bool(d[0])                               # the episode ended on its last step
    if drive == "rule_based":                                                        # the controller did switch (bang-bang)
        assert np.abs(np.diff(np.array(u_seen), axis=0)).max() > 0.5
    for h in (env, exp, m):
        h.close()


def _bdf_holdout(g, name, dtype, tol=1e-6):
    if name == "holdout_runtime_dt300":
        U = g["U"].astype(np.float64)
        XR = np.vstack([g["X"], g["X_last"][None]]) if (len(U) % 3) else g["X"]
        env = make_env(g, dtype, "quad", 0, "parity", 300.0, 10, params=g["p"], pred_horizon=0, integrator="bdf", rtol=tol, atol=tol)
        X = rollout(env, len(U), controls=U, x0=g["x0"], keep_every=3)
        if len(U) % 3:
            X = np.vstack([X, env.x[0].double().cpu().numpy()[None]])
    elif name == "holdout_gl2010_rulebased":
        U, XR = g["U"], g["X"]
        env = make_env(g, dtype, "quad", 0, "parity", 900.0, 10, params=g["p"], pred_horizon=0, integrator="bdf", rtol=tol, atol=tol)
        X = rollout(env, len(U), controls=U)
    else:
        acts, XR = g["actions"], g["X"]
        env = make_env(g, dtype, "quad", 0, "parity", 900.0, 10, integrator="bdf", rtol=tol, atol=tol)
        X = rollout(env, len(acts), actions=acts)
    m = env.metrics()
    env.close()
    return judge_rollout(X, XR)[0], m


@pytest.mark.parametrize("name", ["holdout_gl2010_random", "holdout_gl2010_rulebased", "holdout_runtime_dt300"])
def test_holdouts_free_running(golden, name):
    g = golden(name)
    band = float(g["bdf_free"].max())
    e64, m64 = _bdf_holdout(g, name, "float64")
    e32, m32 = _bdf_holdout(g, name, "float32")
    e64t, m64t = _bdf_holdout(g, name, "float64", 1e-8)
    print(f"{name} BDF env-steps: fp64 {e64:.2e} ({e64 / band:.2f} x the BDF-1e-6 free-running band {band:.2e}), fp32 {e32:.2e}, "
          f"fp64 at 1e-8 {e64t:.2e} ({e64t / e64:.3f} x)")
    for m in (m64, m32, m64t):
        assert m["n_ode_fail"] == 0 and m["n_env_steps"] > 0
    assert e64 <= 1.25 * band
    assert e32 <= max(1.25 * band, PLAIN_BOUND[name]["parity"][1])
    assert e64t <= 0.2 * e64


def test_failure_contract(golden):
    from gl_gym_amd import _lib as L
    g = golden("holdout_gl2010_random")
    X, U, W = g["X"][:64], g["U"][:64], g["weather"][:64]
    up = np.full_like(U, 0.25)
    m = gl(max_steps=5)
    r = env_step(m, X, up, W, control=U)
    assert r["rc"] == L.OK and np.all(r["done"] == 1) and np.array_equal(r["x"], X) and np.array_equal(r["u"], U)
    assert np.all(r["ts"] == 1) and np.all(r["flags"] == (L.SF_FAILED | L.SF_BDF | (5 << 16)))
    assert r["metrics"][3] == 64 and r["metrics"][2] == 64
    assert np.all(r["info"][:, 1] == 0)                                        # no gains
    m.close()
    m = gl()
    clean = env_step(m, X, up, W, control=U)
    Xb = X.copy(); Xb[9, 4] = np.nan
    bad = env_step(m, Xb, up, W, control=U)
    keep = np.arange(64) != 9
    assert bad["rc"] == L.OK and bad["done"][9] == 1 and bad["flags"][9] == (L.SF_FAILED | L.SF_BDF)
    assert np.array_equal(bad["x"][9], Xb[9], equal_nan=True)
    for k in ("x", "u", "reward", "info", "done", "ts", "flags"):
        assert np.array_equal(bad[k][keep], clean[k][keep]), k
    m.close()


def test_switching(golden):
    from gl_gym_amd import GreenLight
    from gl_gym_amd import _lib as L
    g = golden("refenv_1day")
    acts = g["ra_actions"][:3]

    def run(env):
        env.reset()
        out = [env.step(a[None]) for a in acts]
        return env.x_T.cpu().numpy().copy(), np.array([o[1] for o in out]), env.step_flags_t.cpu().numpy().copy()
    a = _vec(g, integrator="explicit")
    b = _vec(g, integrator="explicit")
    b.set_integrator("bdf")
    assert b.integrator == "bdf"
    run(b)
    b.set_integrator("explicit")
    ra, rb = run(a), run(b)
    assert all(np.array_equal(p, q) for p, q in zip(ra, rb))
    assert (b.scheme, b.n_sub, b.window) == (a.scheme, a.n_sub, a.window)
    a.close(); b.close()
    # evalF-only BDF still refuses env-steps; ODE_pipe refuses BDF env-steps
    gh = golden("holdout_gl2010_random")
    X, U, W = gh["X"][:4], gh["U"][:4], gh["weather"][:4]
    m = gl()
    r = env_step(m, X, U, W, control=U, step_bdf=False)
    assert r["rc"] == L.EINVAL and b"glgym_evalF only" in m._lib.glgym_last_error()
    m.close()
    mp = GreenLight(28, 6, 14, 208, 900.0, variant="ode_pipe")
    Wp = np.hstack([W, np.zeros((4, 4))])
    r = env_step(mp, X, U, Wp, control=U)
    assert r["rc"] == L.EINVAL and np.array_equal(r["x"], X)
    mp.close()


def test_graph_capture_and_seams(golden):
    import torch
    from gl_gym_amd.tomato_env import TomatoEnv, TomatoVecEnv
    from gl_gym_amd.vector_env import TomatoVectorEnv
    g = golden("refenv_1day")
    acts = torch.as_tensor(g["ra_actions"][:3], dtype=torch.float32, device="cuda:0")
    B = 8
    kw = dict(weather=g["weather"], params=g["p"], dtype="float64", season_length=1, auto_reset=True, integrator="bdf")
    eager, graphed = TomatoVecEnv(B, **kw), TomatoVecEnv(B, **kw)
    eager.reset_tensor(); graphed.reset_tensor()
    replay = graphed.capture_step_graph()
    for k in range(3):
        a = acts[k][None].expand(B, 6).contiguous()
        e = eager.step_tensor(a)
        r = replay(a)
        torch.cuda.synchronize()
        for p, q in zip(e, r):
            assert torch.equal(p, q), k
        assert torch.equal(eager.x_T, graphed.x_T) and torch.equal(eager.step_flags_t, graphed.step_flags_t)
    eager.close(); graphed.close()
    env = TomatoEnv(weather=g["weather"], params=g["p"], season_length=1, integrator="bdf", rtol=1e-7)
    env.reset()
    obs, r, term, trunc, info = env.step(np.zeros(6, dtype=np.float32))
    assert np.isfinite(obs).all() and np.isfinite(r) and env.vec.integrator == "bdf" and env.vec.rtol == 1e-7
    env.close()
    venv = TomatoVectorEnv(4, weather=g["weather"], params=g["p"], season_length=1, integrator="bdf")
    venv.reset(seed=0)
    obs, r, term, trunc, infos = venv.step(np.zeros((4, 6), dtype=np.float32))
    assert np.isfinite(obs).all() and np.isfinite(r).all()
    venv.close()


def test_make_vec_env_seam(cfg_dir):
    """The reference's make_vec_env call (gl_gym/RL/utils.py:44-69) with integrator="bdf" forwarded to every env."""
    from gl_gym_amd import _lib as L
    from gl_gym_amd.make_env import load_env_params, make_vec_env
    base, spec = load_env_params("TomatoEnv", str(cfg_dir))
    env = make_vec_env("TomatoEnv", base, spec, seed=666, n_envs=16, dtype="float64", integrator="bdf", rtol=1e-7, atol=1e-7)
    assert env.venv.integrator == "bdf" and (env.venv.rtol, env.venv.atol) == (1e-7, 1e-7)
    obs = env.reset()
    for _ in range(3):
        obs, rew, done, infos = env.step(np.zeros((16, 6), np.float32))
    assert np.isfinite(obs).all() and np.isfinite(rew).all()
    assert all(infos[i]["integration"] & L.SF_BDF for i in range(16))
    assert env.venv.metrics()["n_ode_fail"] == 0 and env.venv.solver_metrics()["bdf_steps"] > 0
    env.close()
