"""Inputs and references for the env-layer kernel tests (tests/test_gpu_obs_kernel.py, test_gpu_reset_kernel.py,
test_gpu_crop_noise.py, test_gpu_rule_based_configs.py) and their host checks (tests/test_envlayer_inputs_host.py).

The references are vectorised fp64 NumPy restatements of the reference project's Python text -- observations.py:59-182 with the clocks
of tomato_env.py:126-128, utils.py init_state, and the counter layouts include/glgym.h documents -- not of the kernels.  The crop-noise
and controller references are the suite's own (test_controller_and_noise.expected_crop_noise, gl_gym_amd.baseline).  The builders are
seeded; every environment of a batch gets its own state, controls, weather window, timestep and start day, and the first environments
of a batch are placed on the edges the kernels have a branch or a clamp for (OBS_KINDS).

Device side: SoA inputs are allocated with ld > B and NaN in the padding columns, every buffer a kernel writes is a `Guarded` one --
GUARD bytes of 0xFF in front and behind, and 0xFF (a NaN in both float formats, -1 as an integer) wherever the test did not put data."""
import ctypes as C

import numpy as np

from test_controller_and_noise import expected_crop_noise, philox4x32_10  # noqa: F401  (re-exported)

# ---------------------------------------------------------------------------------------------------------------------------
# observations
# ---------------------------------------------------------------------------------------------------------------------------
# GLGYM_OBS_* ids in include/glgym.h order: indoor climate (4), crop (3), controls (6), weather (5), time (5), forecast (5 Np)
MODULE_WIDTH = (4, 3, 6, 5, 5)
MODULE_LISTS = {
    "default": [0, 1, 2, 3, 4, 5],
    "permuted": [0, 5, 4, 2, 1, 3],            # tests/test_gpu_step_obs.py LAYOUTS["permuted"]
    "no_forecast": [0, 4, 3, 1, 2],
    "forecast_only": [5],
    "crop_only": [1],                          # dim = 3
    "time_climate": [4, 0],                    # dim = 9
}
# pass-through columns inside each module: copied from an input, so float32(input) bit for bit; the others are computed
_PASS = {0: (False, True, False, True), 1: (True,) * 3, 2: (True,) * 6, 3: (True, True, False, False, True),
         4: (True, False, False, False, False)}
OBS_RTOL = OBS_ATOL = 3e-6                     # computed columns: the bound of tests/test_gpu_refenv.py

OBS_BATCHES = (1, 15, 16, 17, 31, 33, 100)
OBS_NP = (0, 1, 3, 127, 128)
OBS_ROWS = 400                                 # rows of the builders' weather table
# what env b of a batch is placed on (b >= len: "generic")
OBS_KINDS = ("generic", "ts0", "ts1", "last_row", "straddle", "beyond", "negative", "day_whole", "year_whole", "year_cross")


def obs_layout(modules, Np):
    """-> ({module id: first column}, row width) of a module list."""
    off, dim = {}, 0
    for m in modules:
        off[m] = dim
        dim += 5 * Np if m == 5 else MODULE_WIDTH[m]
    return off, dim


def obs_passthrough(modules, Np):
    """-> bool [dim]: True where the column is a copy of an input."""
    off, dim = obs_layout(modules, Np)
    mask = np.zeros(dim, dtype=bool)
    for m, o in off.items():
        mask[o:o + (5 * Np if m == 5 else MODULE_WIDTH[m])] = True if m == 5 else _PASS[m]
    return mask


def obs_reference(x, u, weather, w_off, timestep, start_day, Np, modules, dt):
    """Observation rows [B, dim] in float64.  x [B, 28], u [B, 6], weather [rows, >= 5]; timestep is the value AFTER the step's
    increment (0 = freshly reset).  The reference shows the pre-increment row and timestep k = max(timestep - 1, 0) (tomato_env.py
    computes the observation before `self.timestep += 1`) with clocks that the step has already advanced, here in closed form from
    float32(start_day); the forecast is raw columns 0..4 of rows k + 1 .. k + Np.  Row indices clamp to [0, rows - 1] one by one --
    the project's documented behaviour (glgym_obs_args), where the reference would raise."""
    from gl_gym_amd.utils import co2dens2ppm, vaporPres2rh
    x, u, weather = (np.asarray(a, dtype=np.float64) for a in (x, u, weather))
    w_off, ts = np.asarray(w_off, dtype=np.int64), np.asarray(timestep, dtype=np.int64)
    B, rows = len(ts), weather.shape[0]
    k = np.maximum(ts - 1, 0)
    d = weather[np.clip(w_off + k, 0, rows - 1)]
    t_air = x[:, 2]
    doy = np.asarray(start_day, dtype=np.float32).astype(np.float64) + ts * ((dt / 86400.0) % 365)
    hod = (ts * (dt / 3600.0)) % 24.0
    a_doy, a_hod = 2 * np.pi * doy / 365.0, 2 * np.pi * hod / 24.0
    block = {
        0: np.stack([co2dens2ppm(t_air, x[:, 0] * 1e-6), t_air, vaporPres2rh(t_air, x[:, 15]), x[:, 9]], axis=1),
        1: x[:, [21, 25, 26]],
        2: u,
        3: np.stack([d[:, 0], d[:, 1], vaporPres2rh(d[:, 1], d[:, 2]), co2dens2ppm(d[:, 1], d[:, 3] * 1e-6), d[:, 4]], axis=1),
        4: np.stack([k.astype(np.float64), np.sin(a_doy), np.cos(a_doy), np.sin(a_hod), np.cos(a_hod)], axis=1),
        5: weather[np.clip((w_off + k)[:, None] + 1 + np.arange(Np)[None, :], 0, rows - 1)][:, :, :5].reshape(B, 5 * Np),
    }
    return np.concatenate([block[m] for m in modules], axis=1)


def obs_weather(rows=OBS_ROWS):
    from gl_gym_amd.utils import synthetic_weather
    w = synthetic_weather(n_rows=rows, seed=77)
    w[:, 0] += np.arange(rows) * 1e-3          # no two rows alike, nights included
    return w


def obs_case(B, Np, dt=900.0, seed=0, kinds=OBS_KINDS):
    """One batch of observation inputs: dict x [B, 28], u [B, 6], weather [OBS_ROWS, 10], w_off, timestep [B] int32, start_day [B]
    float32, kind [B] (names of OBS_KINDS).  Env b < len(kinds) is of kind kinds[b]; a kind the forecast length cannot show
    ("straddle" needs Np >= 3) falls back to "generic".  The first shown row of every env is drawn without replacement, so that no
    two rows of any module list are equal."""
    rng = np.random.default_rng([seed, B, Np])
    w = obs_weather()
    rows = w.shape[0]
    per_day = int(round(86400.0 / dt))
    x = np.tile(init_like(w[0]), (B, 1)) * (1 + 0.05 * rng.standard_normal((B, 28)))
    x[:, 2] = rng.uniform(10, 30, B)
    sat = 610.78 * np.exp(17.2694 * x[:, 2] / (x[:, 2] + 238.3))
    x[:, 15] = rng.uniform(0.4, 1.15, B) * sat                       # some rows above saturation: the RH clip
    x[:, 0] = rng.uniform(400, 2000, B)
    u = rng.uniform(0, 1, (B, 6))
    base = rng.permutation(rows - 2 - Np)[:B] if B <= rows - 2 - Np else None
    assert base is not None
    ts = rng.integers(2, 900, B)
    sday = rng.uniform(0, 364, B).astype(np.float32)
    kind = []
    for b in range(B):
        kd = kinds[b] if b < len(kinds) else "generic"
        if kd == "straddle" and Np < 3:
            kd = "generic"
        if kd == "ts0":
            ts[b] = 0
        elif kd == "ts1":
            ts[b] = 1
        elif kd == "last_row":
            base[b] = rows - 1
        elif kd == "straddle":
            base[b] = rows - 1 - (Np + 1) // 2
        elif kd == "beyond":
            base[b] = rows + 7
        elif kd == "negative":
            base[b] = -2
        elif kd == "day_whole":
            ts[b] = per_day                                          # hour-of-day revolution = 1 exactly
        elif kd == "year_whole":
            ts[b], sday[b] = per_day, 364.0                          # day-of-year revolution = 1 exactly
        elif kd == "year_cross":
            ts[b], sday[b] = per_day // 2, 364.75
        kind.append(kd)
    w_off = base - np.maximum(ts - 1, 0)
    return dict(x=x, u=u, weather=w, w_off=w_off.astype(np.int32), timestep=ts.astype(np.int32), start_day=sday, kind=np.array(kind))


def init_like(d0):
    from gl_gym_amd.utils import init_state
    return init_state(d0)


def assert_rows_distinct(ref):
    r = np.ascontiguousarray(ref)
    assert len(np.unique(r, axis=0)) == len(r), "two expected rows are equal: a row written to the wrong place could pass"


def mask_of(kind, B, seed=5):
    """The masks of the masked-mode tests -> uint8 [B]."""
    m = np.zeros(B, dtype=np.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind == "corners":
        m[[i for i in (0, 15, 16, B - 1) if i < B]] = 1
    elif kind == "random":
        m[:] = np.random.default_rng([seed, B]).uniform(size=B) < 0.4
    elif kind == "strip_off":                   # everything but one whole 16-row strip (the second)
        m[:] = 1
        m[16:32] = 0
    else:
        assert kind == "zeros"
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# reset
# ---------------------------------------------------------------------------------------------------------------------------
RESET_BATCHES = (1, 255, 256, 257, 1000)
RESET_N_STARTS = (1, 3, 7, 1000)
RESET_SEEDS = (0, 4242, 0x9E3779B97F4A7C15)    # the last one has a non-zero high word
RESET_EPISODES = (0, 1, 12345)
RESET_ROWS = 300
RESET_COMPUTED = (11, 12, 13, 15, 16)          # entries of init_state that go through a sum of products or exp


def reset_draw(b, episode, seed, n_starts):
    """Start-table entry of env b's episode (glgym_reset_args): counter {b, episode, 0x5eed, 0}, key {seed low, seed high}."""
    return philox4x32_10([b, episode, 0x5eed, 0], [seed & 0xFFFFFFFF, seed >> 32])[0] % n_starts


def reset_reference(weather, w_off, episode, seed, start_rows=None, start_days=None, start_day=None):
    """Every env of the batch reset -> dict x [B, 28] float64, w_off, start_day, episode (None where the input was None).
    With a start table env b takes entry reset_draw(b, episode[b], seed, n_starts) and its episode count goes up by one; without,
    it keeps the w_off found.  x = init_state(weather[clamp(w_off)]); controls 0 and timestep 0 are the caller's to assert."""
    from gl_gym_amd.utils import init_state
    weather = np.asarray(weather, dtype=np.float64)
    w_off = np.array(w_off, dtype=np.int64)
    B, rows = len(w_off), weather.shape[0]
    ep = None if episode is None else np.array(episode, dtype=np.int64)
    sd = None if start_day is None else np.array(start_day, dtype=np.float32)
    if start_rows is not None and len(start_rows) > 0:
        j = np.array([reset_draw(b, 0 if ep is None else int(ep[b]), seed, len(start_rows)) for b in range(B)])
        w_off = np.asarray(start_rows, dtype=np.int64)[j]
        if sd is not None and start_days is not None:
            sd = np.asarray(start_days, dtype=np.float32)[j]
        if ep is not None:
            ep = ep + 1
    x = np.array([init_state(weather[min(max(int(r), 0), rows - 1)]) for r in w_off])
    return dict(x=x, w_off=w_off, start_day=sd, episode=ep)


def init_state_computed_ld(d0):
    """The entries RESET_COMPUTED of init_state in numpy.longdouble."""
    L = np.longdouble
    t_air, t_so = L(16.5), L(d0[6])
    vp = L(90) / L(100) * (L(610.78) * np.exp(L(17.2694) * t_air / (t_air + L(238.3))))
    return np.array([L(0.25) * (L(3) * t_air + t_so), L(0.25) * (L(2) * t_air + L(2) * t_so), L(0.25) * (t_air + L(3) * t_so), vp, vp])


def init_state_spread(weather):
    """Largest relative difference between init_state in float64 and in longdouble over the rows of `weather`, per entry of
    RESET_COMPUTED -- what the reference's own arithmetic leaves open."""
    from gl_gym_amd.utils import init_state
    worst = np.zeros(len(RESET_COMPUTED))
    for d0 in np.asarray(weather, dtype=np.float64):
        ld = init_state_computed_ld(d0)
        f64 = init_state(d0)[list(RESET_COMPUTED)]
        worst = np.maximum(worst, np.abs((ld - f64) / ld).astype(np.float64))
    return worst


def reset_weather(rows=RESET_ROWS):
    from gl_gym_amd.utils import synthetic_weather
    return synthetic_weather(n_rows=rows, seed=78)


def reset_start_table(n_starts, rows=RESET_ROWS, seed=3):
    """-> (start_rows int32 [n], start_days float32 [n]); with n >= 3 the first entry lies in front of the table and the last behind."""
    rng = np.random.default_rng([seed, n_starts])
    sr = rng.integers(0, rows, n_starts).astype(np.int32)
    if n_starts >= 3:
        sr[0], sr[-1] = -4, rows + 10
    return sr, rng.uniform(0, 364, n_starts).astype(np.float32)


def reset_case(B, rows=RESET_ROWS, seed=0):
    """Pre-reset contents of a batch: x [B, 28], u [B, 6] (random, recognisable), timestep, w_off (some outside the table), start_day,
    episode (RESET_EPISODES in turn)."""
    rng = np.random.default_rng([seed, B])
    w_off = rng.integers(0, rows, B).astype(np.int32)
    w_off[0] = -3
    if B > 2:
        w_off[B - 1], w_off[B // 2] = rows, rows + 1234
    return dict(x=rng.uniform(1, 2, (B, 28)), u=rng.uniform(0.1, 0.9, (B, 6)), timestep=rng.integers(1, 900, B).astype(np.int32),
                w_off=w_off, start_day=rng.uniform(0, 364, B).astype(np.float32),
                episode=np.array([RESET_EPISODES[b % 3] for b in range(B)], dtype=np.int32))


def reset_mask(kind, B, seed=6):
    m = np.zeros(B, dtype=np.uint8)
    if kind == "corners":
        m[[i for i in (0, 255, 256, B - 1) if i < B]] = 1
    else:
        assert kind == "random"
        m[:] = np.random.default_rng([seed, B]).uniform(size=B) < 0.5
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# crop noise
# ---------------------------------------------------------------------------------------------------------------------------
NOISE_BATCHES = (1, 255, 256, 257, 1000)
NOISE_SEEDS = (4242, 0x9E3779B97F4A7C15)
NOISE_DRAWS = (0, 1, 2 ** 32 + 5, 2 ** 40)
NOISE_SCALES = (0.0, 0.2, 1.0)
NOISE_PAD = 7
_noise_cache = {}


def crop_p0():
    from gl_gym_amd.parameters import init_default_params
    return np.asarray(init_default_params(208), dtype=np.float32)[128:162].copy()


def crop_noise_reference(B, scale, seed, draw):
    """expected_crop_noise for the first B envs; the definition is per env, so one evaluation at the largest batch serves all."""
    key = (float(scale), int(seed), int(draw))
    assert B <= max(NOISE_BATCHES)
    if key not in _noise_cache:
        _noise_cache[key] = expected_crop_noise(crop_p0(), max(NOISE_BATCHES), scale, seed, draw)
    return _noise_cache[key][:, :B]


# ---------------------------------------------------------------------------------------------------------------------------
# rule-based controller
# ---------------------------------------------------------------------------------------------------------------------------
RULE_BATCHES = (1, 255, 257)
RULE_BANDS = ("vent_heat_Pband", "vent_rh_Pband", "vent_cold_Pband", "thScrPband", "thScrRhPband", "tHeatBand", "co2Band")
RULE_RTOL, RULE_ATOL = 1e-12, 1e-14            # tests/test_controller_and_noise.py


def rule_config(g, name):
    """Constructor arguments of config `name` of tests/golden/controller_kat_configs.npz."""
    return {str(k): float(v) for k, v in zip(g["fields"], g[f"{name}_cfg"])}


def rule_clocks(g, name, hour_explicit, doy_explicit):
    """-> (hour [64], doy [64], expected U [64, 6]) of one of the four clock combinations."""
    return (g[f"{name}_hour" if hour_explicit else f"{name}_hour_d"], g[f"{name}_doy" if doy_explicit else f"{name}_doy_d"],
            g[f"{name}_U_hd"][0 if hour_explicit else 1, 0 if doy_explicit else 1])


# ---------------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------------
GUARD = 256                                    # bytes in front of and behind every buffer; keeps the payload 16-byte aligned


def rounded(a, f64):
    """The array as a handle of that dtype stores it, widened again."""
    a = np.asarray(a, dtype=np.float64)
    return a if f64 else a.astype(np.float32).astype(np.float64)


def soa(a, ld, dtype):
    """[B, n] -> SoA [n, ld] of `dtype` with NaN in the padding columns."""
    a = np.asarray(a)
    out = np.full((a.shape[1], ld), np.nan, dtype=dtype)
    out[:, :a.shape[0]] = a.T
    return out


class Guarded:
    """A device buffer with GUARD bytes of 0xFF in front and behind.  Made from a host array, or from shape + dtype alone: then the
    payload is 0xFF as well (NaN as float32 / float64, -1 as int32, 255 as uint8)."""

    def __init__(self, arr=None, *, shape=None, dtype=None):
        import torch
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            shape, dtype, payload = arr.shape, arr.dtype, arr.reshape(-1).view(np.uint8)
        else:
            payload = np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, 0xFF, dtype=np.uint8)
        self.shape, self.dtype, self.n = tuple(shape), np.dtype(dtype), payload.size
        g = np.full(GUARD, 0xFF, dtype=np.uint8)
        self.t = torch.from_numpy(np.concatenate([g, payload, g])).to("cuda:0")
        self.ptr = self.t.data_ptr() + GUARD
        assert self.ptr % 16 == 0

    def read(self):
        """The payload; asserts that both guards still hold their pattern."""
        h = self.t.cpu().numpy()
        assert np.all(h[:GUARD] == 0xFF), "the guard in front of the buffer was written"
        assert np.all(h[GUARD + self.n:] == 0xFF) and h.size == self.n + 2 * GUARD, "the guard behind the buffer was written"
        return h[GUARD:GUARD + self.n].copy().view(self.dtype).reshape(self.shape)

    def untouched(self):
        return bool(np.all(self.read().reshape(-1).view(np.uint8) == 0xFF))


def bits(a):
    """Integer view for bit-for-bit comparisons (NaN payloads included)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


class Handle:
    """A raw glgym handle, as tests/test_gpu_vecnorm.py makes its own.  nd: columns of a weather row (default the model's 10; up to 16,
    14 being the rows of GLGYM_ODE_PIPE).  params: the parameter block [208] (default: the default block)."""

    def __init__(self, f64, dt=900.0, nd=None, params=None):
        import torch
        from gl_gym_amd import _lib as L
        from gl_gym_amd.parameters import init_default_params
        assert torch.cuda.is_available()
        self.t, self.L, self.f64, self.dt = torch, L, f64, dt
        self.T = np.float64 if f64 else np.float32
        self.lib, self.h = L.load(), C.c_void_p()
        self.nd = L.ND if nd is None else int(nd)
        p = np.ascontiguousarray(init_default_params(L.NP) if params is None else params, dtype=np.float64)
        L.check(self.lib.glgym_create(L.NX, L.NU, self.nd, L.NP, dt, p.ctypes.data_as(L._DP), L.F64 if f64 else L.F32, 4, 0,
                                      C.byref(self.h)), "glgym_create")

    def stream(self):
        return C.c_void_p(self.t.cuda.current_stream().cuda_stream)

    def sync(self):
        self.t.cuda.synchronize()

    def error(self):
        return self.lib.glgym_last_error().decode()

    def close(self):
        self.lib.glgym_destroy(self.h)
