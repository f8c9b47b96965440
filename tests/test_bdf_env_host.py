"""CPU tests of the BDF env-step (glgym_set_step_integrator, GLGYM_SF_BDF, GLGYM_METRIC_BDF): the binding agrees with the header and
the library, the env classes validate their integrator arguments without a device, and the host instantiation of
csrc/gl_bdf_env.hpp's env-step (a team of one lane, tests/bdfhost/envstep_host.cpp) reproduces the reference env's step semantics over
the oracle's BDF at the same tolerance."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from gl_gym_amd import _lib
    if not _lib.LIB_PATH.exists():
        g.build()
    return _lib


def test_step_integrator_abi_is_declared_bound_and_versioned(lib):
    hdr = (ROOT / "include" / "glgym.h").read_text()
    assert re.search(r"\bint glgym_set_step_integrator\s*\(glgym_handle h, int integrator\);", hdr)
    assert lib.PROTOTYPES["glgym_set_step_integrator"] == (C.c_int, [C.c_void_p, C.c_int])
    L = lib.load()
    assert L.glgym_set_step_integrator.argtypes == [C.c_void_p, C.c_int]
    assert int(re.search(r"#define GLGYM_SF_BDF (\d+)", hdr).group(1)) == lib.SF_BDF == 1 << 11
    assert int(re.search(r"#define GLGYM_METRIC_BDF (\d+)", hdr).group(1)) == lib.METRIC_BDF == lib.NMETRIC == 14
    assert lib.METRIC_BDF + len(lib.BDF_METRIC_KEYS) <= lib.METRIC_STRIDE
    assert int(re.search(r"#define GLGYM_NMETRIC (\d+)", hdr).group(1)) == 14
    assert lib.ABI_VERSION == 7 == L.glgym_abi_version()
    assert L.glgym_set_step_integrator(None, 1) == lib.EINVAL
    assert L.glgym_set_step_integrator(None, 0) == lib.EINVAL


BAD = [dict(integrator="rk45"), dict(integrator="BDF"), dict(integrator="bdf", rtol=0.0), dict(integrator="bdf", atol=-1e-6),
       dict(rtol=float("nan")), dict(atol=float("inf")), dict(integrator="bdf", max_steps=0), dict(max_steps=2.5),
       dict(integrator="bdf", model_variant="ode_pipe")]


@pytest.mark.parametrize("kw", BAD)
def test_vec_env_validates_integrator_arguments_before_the_device(kw):
    from gl_gym_amd.tomato_env import TomatoVecEnv
    with pytest.raises(ValueError):
        TomatoVecEnv(4, **kw)


@pytest.mark.parametrize("kw", BAD)
def test_single_env_validates_integrator_arguments_before_the_device(kw):
    from gl_gym_amd.tomato_env import TomatoEnv
    with pytest.raises(ValueError):
        TomatoEnv(**kw)


@pytest.fixture(scope="module")
def envstep(tmp_path_factory):
    so = tmp_path_factory.mktemp("envstep") / "libenvstep.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           f"-I{ROOT / 'tests' / 'bdfhost'}", "-o", str(so), str(ROOT / "tests" / "bdfhost" / "envstep_host.cpp")])
    L = C.CDLL(str(so))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    L.envstep_host.argtypes = [dp, dp, C.POINTER(C.c_float), dp, dp, C.c_int, C.c_int, C.c_int, ip, C.c_int, dp, C.c_double, C.c_double,
                               C.c_double, C.c_int, dp, dp, C.POINTER(C.c_uint8), ip, ip]
    return L


def test_host_env_row_against_the_oracle_env_over_bdf(envstep, oracle, golden):
    """refenv_1day's ra_* (actions) and rb_* (raw controls) sequences, 97 steps each, teacher-forced on the host function's own states:
    applied controls, the one-step state against gl_oracle's BDF at the same tolerance, reward / info against OracleReward on the host
    function's new state, done and timestep."""
    from oracle.gl_env_oracle import OracleReward, OracleTomatoEnv
    from gl_gym_amd._lib import INFO_KEYS
    g = golden("refenv_1day")
    W = np.ascontiguousarray(g["weather"], dtype=np.float64)
    N = int(g["N"])
    tol, dt = 1e-6, 900.0
    dp = C.POINTER(C.c_double)
    for tag in ("ra", "rb"):
        env = OracleTomatoEnv(W, g["p"], season_length=1, dt=dt)
        env._evalF = lambda x, u, d, p: oracle.bdf(x, u, d, np.asarray(p, dtype=np.float64), dt, tol, tol)[0]
        env.reset(seed=0)
        # the library promotes the float32 parameter block to double once (glgym_create); with a float32 block numpy would compute
        # OracleReward's scale in float32 (3e-8 relative), so the oracle gets the same promoted block
        p64 = np.ascontiguousarray(env.p, dtype=np.float64)
        env.p = p64
        env.reward = OracleReward(env)
        x = np.ascontiguousarray(g[f"{tag}_x"][0], dtype=np.float64)
        u = np.zeros(6)
        ts = C.c_int(0)
        H, R = [], []
        n_steps = len(g[f"{tag}_u"])
        assert n_steps == N + 1
        for k in range(n_steps):
            x_prev, u_prev = x.copy(), u.copy()
            act = np.ascontiguousarray(g["ra_actions"][k], dtype=np.float32) if tag == "ra" else None
            ctl = None if tag == "ra" else np.ascontiguousarray(g["rb_u"][k], dtype=np.float64)
            rew, info = C.c_double(), np.zeros(11)
            done, flags, st = C.c_uint8(), C.c_int(), np.zeros(5, dtype=np.int32)
            envstep.envstep_host(x.ctypes.data_as(dp), u.ctypes.data_as(dp),
                                 act.ctypes.data_as(C.POINTER(C.c_float)) if act is not None else None,
                                 ctl.ctypes.data_as(dp) if ctl is not None else None, W.ctypes.data_as(dp), len(W), W.shape[1], 0,
                                 C.byref(ts), N, p64.ctypes.data_as(dp), dt, tol, tol, 10000, C.byref(rew), info.ctypes.data_as(dp),
                                 C.byref(done), C.byref(flags), st.ctypes.data_as(C.POINTER(C.c_int)))
            # the oracle env from the same state and control
            env.x, env.x_prev, env.u, env.timestep = x_prev.copy(), x_prev.copy(), u_prev.copy(), k
            _, _, term, _ = env.step(act) if tag == "ra" else env.step_raw_control(ctl)
            assert np.array_equal(u, env.u), (tag, k, u, env.u)
            H.append(x.copy()); R.append(np.asarray(env.x, dtype=np.float64).copy())
            assert bool(done.value) == bool(term) == (k >= N) and ts.value == env.timestep == k + 1
            assert flags.value == 2048 | (int(st[0]) << 16) and st[0] >= 1
            # reward and info of the reference's GreenhouseReward on the host function's own new state
            env.x, env.x_prev = x.copy(), x_prev.copy()
            env.obs = env._get_obs()
            r_ref = env.reward.compute_reward()
            i_ref = env.reward.info()
            assert abs(rew.value - r_ref) <= 1e-12 * max(abs(r_ref), 1.0), (tag, k, rew.value, r_ref)
            for q, key in enumerate(INFO_KEYS):
                ref = float(i_ref[key])
                assert abs(info[q] - ref) <= 1e-12 * max(abs(ref), 1e-3), (tag, k, key, info[q], ref)
        e = oracle.scaled_rel_err(np.array(H), np.array(R))
        print(f"refenv_1day {tag}: one-step state difference host env row vs oracle env over gl_oracle_bdf {e:.2e}")
        assert e <= 5e-5
