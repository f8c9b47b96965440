"""Cases, inputs and references of the step-kernel build census (tests/test_gpu_step_builds.py) and its host checks
(tests/test_step_build_inputs_host.py).  Importable without a GPU.

The cases: one per build csrc/gl_step_select.hpp lists -- 53 one-lane-per-environment fp32 builds, 28 four-lanes-per-environment ones --
each with the recipe that reaches it at a small batch through the C ABI.  The lists are restated here on purpose: a build added to
the header has no case until it is added here as well, and tests/test_step_build_inputs_host.py fails until then.

The inputs: 65 environments, every one different.  Even rows are tests/test_gpu_fuzz.py's random tuples, far off equilibrium (the
stability control refines them), odd rows the calm tuples of tests/golden/step_tight.npz (mostly the nominal sub-step count), so that
every wavefront holds refined and nominal lanes side by side.  Every row has its own weather row (through w_off), its own timestep and the
clock x[27] that goes with it; a few rows of the first wavefront and the last row start at timestep >= N: `done` fires there.

The references: oracle.gl_oracle.rk_sc_guarded on the inputs as the handle's dtype stores them and on the control the kernel applied,
cached by what the reference depends on (never per build); the reference project's reward restated (oracle.gl_env_oracle.OracleReward) on
the kernel's own returned state, so that the integrator's error is not in it; envlayer_inputs.obs_reference for observation rows."""
import collections
import hashlib
from multiprocessing.pool import ThreadPool
from pathlib import Path

import numpy as np

import envlayer_inputs as E

GOLDEN = Path(__file__).resolve().parent / "golden"
RK4, RK2, RK3, LS5 = 0, 1, 2, 3
ONE_LANE, QUAD, QUAD_PAIR = 0, 1, 2
FAMILY_NAME = {ONE_LANE: "one", QUAD: "quad", QUAD_PAIR: "pair"}
# scheme -> (GLGYM_SCHEME_*, nominal n_sub, the oracle's order, the scheme's window): tests/test_gpu_storm.py SCHEMES, test_gpu_fuzz.py
SCHEMES = {"ls5": (LS5, 128, 5, 2), "rk4": (RK4, 240, 4, 4), "rk3": (RK3, 270, 3, 3), "rk2": (RK2, 336, 2, 4)}
# csrc/gl_step_select.hpp GL_STEP_ONE_LANE_BUILDS: (CROP, DEF, PIPE, EPI, OCC); PIPE with RK4 only
ONE_LANE_BUILDS = [(0, 0, 0, 0, 1), (0, 1, 0, 0, 1), (1, 0, 0, 0, 1), (1, 1, 0, 0, 1), (0, 1, 0, 0, 2),
                   (0, 0, 0, 8, 1), (0, 1, 0, 8, 1), (1, 0, 0, 8, 1), (1, 1, 0, 8, 1), (0, 1, 0, 8, 2),
                   (0, 0, 0, 24, 1), (0, 1, 0, 24, 1), (0, 1, 0, 24, 2),
                   (0, 0, 1, 0, 1)]
# GL_STEP_QUAD_BUILDS: (F64, DEF, PIPE, CROP, PAIR)
QUAD_BUILDS = [(1, 0, 1, 0, 0), (1, 0, 1, 1, 0), (1, 0, 1, 0, 1), (0, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 0, 0, 1), (0, 1, 0, 0, 1)]
ENTRY = {0: "step", 8: "step_obs", 24: "step_obs_reset"}
FUSED = {0: 0, 8: 1, 24: 2}

N_ENV, LD, BATCHES = 65, 80, (65, 1)
DT, N_TERMINAL = 900.0, 96
NP_FORECAST = 3
OBS_DIM = 23 + 5 * NP_FORECAST
DONE_ROWS = (3, 17, 40, 64)                 # timestep >= N: three in the first wavefront, and the last row
CLIP_HIGH_ROW, CLIP_LOW_ROW = 9, 12          # action rows that clip at the upper / lower limit in every control
NAN_ROW = 5
SEED = 20261020

# build = (family, f64, crop, def, pipe, sch, epi, occ), the row tests/stepselecthost exports and glgym_last_step_build returns
Case = collections.namedtuple("Case", "id build scheme f64 layout occupancy params crop pipe nd entry raw ladder_parallel lanes")


def _case(build, scheme):
    family, f64, crop, deflt, pipe, sch, epi, occ = build
    bits = [FAMILY_NAME[family], "f64" if f64 else "f32"] + (["crop"] if crop else []) + (["def"] if deflt else []) + \
           (["pipe"] if pipe else []) + [scheme] + ([f"epi{epi}", f"occ{occ}"] if family == ONE_LANE else [])
    runs_pipe = bool(pipe and family == ONE_LANE)       # the fp64 quad builds have ODE_pipe compiled in; it is selected at run time
    return Case(id="-".join(bits), build=build, scheme=scheme, f64=bool(f64), layout=1 if family == ONE_LANE else 2, occupancy=occ,
                params="default" if deflt else "handle", crop=bool(crop), pipe=runs_pipe, nd=14 if runs_pipe else 10, entry=ENTRY[epi],
                raw=family == QUAD_PAIR, ladder_parallel=1 if family == QUAD_PAIR else 0, lanes={ONE_LANE: 1, QUAD: 4, QUAD_PAIR: 8}[family])


def cases():
    out = []
    for scheme, (sch, _, _, _) in SCHEMES.items():
        for crop, deflt, pipe, epi, occ in ONE_LANE_BUILDS:
            if not pipe or sch == RK4:
                out.append(_case((ONE_LANE, 0, crop, deflt, pipe, sch, epi, occ), scheme))
        for f64, deflt, pipe, crop, pair in QUAD_BUILDS:
            out.append(_case((QUAD_PAIR if pair else QUAD, f64, crop, deflt, pipe, sch, 0, 1), scheme))
    return out


CASES = cases()
BY_BUILD = {c.build: c for c in CASES}


def verified_twin(c):
    """The builds that also run once with raw controls (a verified step under GLGYM_VERIFY_AUTO) and the sequential ladder."""
    if c.build[0] == QUAD:
        return True
    return c.build[0] == ONE_LANE and c.build[1:5] == (0, 0, 1, 0) and c.build[6] == 0


def grid(c, B):
    return -(-c.lanes * B // 64)


def select_inputs(c, B, n_simd, raw=None):
    """The row tests/stepselecthost's stepselect_batch takes (StepSelectIn's fields in order) for what the recipe sets."""
    raw = c.raw if raw is None else raw
    return [int(c.f64), SCHEMES[c.scheme][0], int(c.pipe), int(c.crop), int(c.params == "default"), c.layout, c.occupancy, B, n_simd,
            int(raw), c.ladder_parallel, int(c.entry != "step"), OBS_DIM if c.entry != "step" else 0, int(c.entry == "step_obs_reset"), 0]


def stepselect_host(build_dir):
    """csrc/gl_step_select.hpp compiled with g++ (tests/stepselecthost/stepselecthost.cpp) into build_dir -> the ctypes library."""
    import ctypes as C
    import subprocess
    root = Path(__file__).resolve().parent.parent
    so = Path(build_dir) / "libstepselecthost.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", f"-I{root / 'greenlight-gym2_amd' / 'csrc'}", "-o", str(so),
                           str(root / "tests" / "stepselecthost" / "stepselecthost.cpp")])
    lib = C.CDLL(str(so))
    lib.stepselect_batch.argtypes, lib.stepselect_batch.restype = [C.c_int, C.c_void_p, C.c_void_p], None
    lib.stepselect_builds.argtypes, lib.stepselect_builds.restype = [C.c_void_p, C.c_int], C.c_int
    lib.evalfselect_batch.argtypes, lib.evalfselect_batch.restype = [C.c_int, C.c_void_p, C.c_void_p], None
    lib.evalfselect_builds.argtypes, lib.evalfselect_builds.restype = [C.c_void_p, C.c_int], C.c_int
    return lib


# ---- parameters --------------------------------------------------------------------------------------------------------------------
def params(kind):
    """The handle's parameter block as glgym_create receives it (float64 of the float32 block)."""
    from gl_gym_amd.parameters import init_default_params
    if kind == "default":
        return np.ascontiguousarray(init_default_params(208), dtype=np.float64)
    from test_gpu_step_reset import handle_params
    return np.ascontiguousarray(handle_params(), dtype=np.float64)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
_golden = lambda name: np.load(GOLDEN / f"{name}.npz", allow_pickle=False)      # noqa: E731
_base = {}


def base():
    """The 65 rows in float64, before any rounding to the handle's dtype: X [65, 28], U (raw controls) [65, 6], D [65, 10],
    CROP [65, 34], timestep, w_off, u_prev, action, start_day, episode."""
    if _base:
        return _base
    from test_gpu_fuzz import _tuples
    Xf, Uf, Df, Pf = _tuples(N_ENV, _golden)
    g = _golden("step_tight")
    p0 = params("default")
    X, U, D, CROP = (np.zeros((N_ENV, n)) for n in (28, 6, 10, 34))
    for i in range(N_ENV):
        if i % 2 == 0:
            X[i], U[i], D[i], CROP[i] = Xf[i], Uf[i], Df[i], Pf[i][128:162]
        else:
            X[i], U[i], D[i], CROP[i] = g["X"][i // 2], g["U"][i // 2], g["D"][i // 2], p0[128:162]
    rng = np.random.default_rng(SEED)
    ts = rng.permutation(90)[:N_ENV].astype(np.int32)                # every row its own timestep
    ts[list(DONE_ROWS)] = (N_TERMINAL, N_TERMINAL + 1, 150, N_TERMINAL)
    X[:, 27] = ts * DT / 86400.0                                     # the clock that goes with it: the kernels' exact x[27] applies
    u_prev = rng.uniform(0, 1, (N_ENV, 6))
    action = rng.uniform(-1, 1, (N_ENV, 6)).astype(np.float32)
    u_prev[CLIP_HIGH_ROW], action[CLIP_HIGH_ROW] = 0.97, 1.0
    u_prev[CLIP_LOW_ROW], action[CLIP_LOW_ROW] = 0.02, -1.0
    _base.update(X=X, U=U, D=D, CROP=CROP, timestep=ts, w_off=(np.arange(N_ENV) - ts).astype(np.int32), u_prev=u_prev, action=action,
                 start_day=rng.uniform(0, 364, N_ENV).astype(np.float32), episode=rng.integers(0, 50, N_ENV).astype(np.int32),
                 start_rows=np.array([2, 11, 30, 47, 63], dtype=np.int32),
                 start_days=np.array([10.5, 100.25, 200.0, 300.75, 59.0], dtype=np.float32))
    return _base


def weather_table(nd):
    """Row i is environment i's weather row; ODE_pipe rows get columns 10..13 as tests/test_gpu_step_reset.py weather(nd) builds them."""
    D = base()["D"]
    if nd == 10:
        return D.copy()
    from test_gpu_step_reset import weather
    w = np.zeros((N_ENV, nd))
    w[:, :10] = D
    w[:, 10:] = weather(nd)[:N_ENV, 10:]
    return w


def host_inputs(c, raw=None):
    """What a case's launch reads, as the handle's dtype stores it and widened again (float64 arrays; action stays float32)."""
    raw = c.raw if raw is None else raw
    b = base()
    r = lambda a: E.rounded(a, c.f64)                                # noqa: E731
    return dict(x=r(b["X"]), u_prev=r(b["u_prev"]), action=None if raw else b["action"], control=r(b["U"]) if raw else None,
                weather=r(weather_table(c.nd)), crop=r(b["CROP"]) if c.crop else None, timestep=b["timestep"], w_off=b["w_off"],
                start_day=b["start_day"], episode=b["episode"], start_rows=b["start_rows"], start_days=b["start_days"], p=params(c.params))


# ---- references --------------------------------------------------------------------------------------------------------------------
def applied_control(u_prev, action, f64, du=0.1):
    """clip(u_prev + float32(action) * float32(du), 0, 1) in the handle's dtype (tomato_env.py:109-113, held in float32 there)."""
    T = np.float64 if f64 else np.float32
    inc = np.asarray(action, dtype=np.float32) * np.float32(du)
    return np.clip(np.asarray(u_prev).astype(T) + inc.astype(T), T(0), T(1)).astype(np.float64)


_state_cache = {}
N_ORACLE_CALLS = [0]


def state_reference(x, u, d, p, crop, scheme, pipe, verify):
    """rk_sc_guarded row by row -> (x_next [B, 28], retries [B], refined sub-steps [B], failed [B]).  Cached by content: whatever
    builds share storage dtype, scheme, parameter block, crop blocks, ODE variant, verify mode and applied control share the result."""
    from oracle import gl_oracle as O
    _, n_sub, order, window = SCHEMES[scheme]
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, u, d, p) + (() if crop is None else (crop,))]
    key = hashlib.sha1(b"".join(a.tobytes() for a in arrays)).hexdigest(), scheme, bool(pipe), bool(verify), crop is None
    if key not in _state_cache:
        B = len(x)
        O.lib()                                                      # built and bound before the threads start

        def row(i):
            pi = p
            if crop is not None:
                pi = p.copy()
                pi[128:162] = crop[i]
            return O.rk_sc_guarded(x[i], u[i], d[i], pi, DT, n_sub, order, window, pipe=pipe, verify=verify)

        with ThreadPool(8) as pool:                                  # (the oracle is C behind ctypes: the calls run side by side)
            res = pool.map(row, range(B))
        N_ORACLE_CALLS[0] += B
        _state_cache[key] = (np.array([r[0] for r in res]), np.array([r[1] for r in res], dtype=int),
                             np.array([r[2] for r in res], dtype=int), np.array([r[3] for r in res], dtype=bool))
    return _state_cache[key]


def state_error(got, ref, scale_from):
    """tests/test_gpu_fuzz.py's metric per row: max over the states of |got - ref| / max(|ref|, column max of |X|)."""
    scale = np.maximum(np.abs(scale_from).max(axis=0), 1e-3)
    return np.max(np.abs(got - ref) / np.maximum(np.abs(ref), scale), axis=1)


def exact_clock(timestep):
    """x[27] after the step, in float64 (the kernels round it to the handle's dtype): (timestep + 1) * dt / 86400."""
    return (np.asarray(timestep, dtype=np.float64) + 1.0) * (DT / 86400.0)


class _RewardEnv:
    pass


def reward_reference(x_prev, x_new, u, p):
    """OracleReward row by row at the kernel's own state and control -> (reward [B], info [B, 11] in GLGYM_NINFO order, the reward's
    profit range max_profit - min_profit)."""
    from oracle.gl_env_oracle import INFO_KEYS, OracleReward, co2_dens_to_ppm, vapor_pres_to_rh
    env = _RewardEnv()
    env.p, env.dt = np.asarray(p, dtype=np.float64), DT
    rw = OracleReward(env)
    B = len(x_new)
    reward, info = np.zeros(B), np.zeros((B, 11))
    for i in range(B):
        env.x, env.x_prev, env.u = x_new[i], x_prev[i], u[i]
        env.obs = np.array([co2_dens_to_ppm(x_new[i, 2], x_new[i, 0] * 1e-6), x_new[i, 2], vapor_pres_to_rh(x_new[i, 2], x_new[i, 15])])
        reward[i] = rw.compute_reward()
        d = rw.info()
        info[i] = [d[k] for k in INFO_KEYS]
    return reward, info, float(rw.max_profit - rw.min_profit)


def reward_error(reward, info, ref_reward, ref_info, profit_range):
    """tests/test_gpu_parity.py test_step_kernel_matches_env_oracle's metrics -> (worst |d reward|, worst |d info| / max(1, |info|),
    worst |d reward| with the kernel's own revenue).  Kept apart: in fp32 the info rows carry the CO2 violation in ppm, whose rounding
    (1e-4 at 1 000 ppm) would hide the reward's.  The third figure takes the reference's revenue from the kernel's revenue row (the
    reward is linear in it) instead of from the stored fruit dry matter: in fp32 the stored difference is quantised at 0.03 mg m-2,
    1e-4 of reward, which hides the reward's arithmetic in the first figure; the revenue row itself is held by the second."""
    own = ref_reward + (info[:, 1] - ref_info[:, 1]) / profit_range
    return (float(np.max(np.abs(reward - ref_reward))), float(np.max(np.abs(info - ref_info) / np.maximum(1.0, np.abs(ref_info)))),
            float(np.max(np.abs(reward - own))))


def done_reference(timestep):
    return (np.asarray(timestep) >= N_TERMINAL).astype(np.uint8)
