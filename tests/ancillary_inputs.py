"""Input builders shared by tests/test_gpu_vecnorm.py, tests/test_gpu_weather.py and tests/test_vecnorm_weather_inputs_host.py
(a plain module, not a conftest): seeded observation / reward batches and ill-conditioned columns for ``glgym_vecnorm``, raw
weather tables and the host composition of ``gl_gym_amd.utils`` for ``glgym_weather``.  Everything here is numpy on the
host; the host test asserts that these inputs are fair to the kernels before the GPU tests hold the kernels to them."""
from __future__ import annotations

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------------
# VecNormalize
# ---------------------------------------------------------------------------------------------------------------------------
# (rtol, atol) of tests/test_gpu_env_api.py::test_vecnormalize_on_device_matches_sb3_algorithm -- the project's own
VN_TOL = {"obs": (1e-5, 2e-5), "reward": (1e-5, 1e-6), "mean": (1e-9, 1e-9), "var": (1e-7, 1e-9), "returns": (1e-9, 1e-12)}
VN_COUNT_ATOL = 1e-6

# (B, dim): the path of glgym_vecnorm each pair reaches (64-row moment strips up to 1 024 blocks, 16-row apply strips up to
# 8 192 blocks, the moments kernel's 8-row unrolled loop, col_threads = dim rounded up to a wave and capped at 1 024)
VN_SHAPES = [
    (1, 1),          # one row, one column: no unrolled pass, tail of one; batch variance 0
    (7, 3),          # B < 8: tail only
    (8, 3),          # exactly one unrolled pass, empty tail
    (9, 3),          # one unrolled pass + tail of one
    (63, 64),        # one short strip (7 passes + tail 7); dim = exactly one wave
    (64, 65),        # one full strip, no tail; dim one past a wave (second wave has one live lane)
    (65, 63),        # second block holds ONE row; dim one short of a wave
    (255, 263),      # the env's row width; last moments block 63 rows, last apply block 15
    (257, 263),      # five moment blocks, the last with one row; 17 apply blocks, the last with one row
    (1000, 503),     # 16 moment blocks = one per replica, last strip 40 rows (5 passes, no tail)
    (65, 1023),      # col_threads 1 024 with one idle lane
    (65, 1024),      # col_threads 1 024 exactly
    (65, 1025),      # column loop: thread 0 owns columns 0 and 1 024
    (33, 2050),      # column loop: three trips for threads 0 and 1
    (65601, 3),      # 1 024 moment blocks x 65-row strips (8 passes + tail 1); blocks 1 010..1 023 are empty
    (131089, 2),     # 8 192 apply blocks x 17-row strips, blocks 7 712.. empty; 129-row moment strips, blocks 1 017.. empty
]
VN_MODE_SHAPES = [(257, 263), (65, 1025)]
VN_N_CALLS = 3


def vn_clip_obs(B):
    """A single outlier among B rows normalises to at most sqrt(B - 1): small batches get a clip they can reach."""
    return 10.0 if B >= 255 else 1.0


def vn_batch(B, dim, call, seed=20240611):
    """Raw float32 observations [B, dim], float64 rewards [B] and done flags [B] of one call.  Columns span seven decades
    of scale with offsets of a few spreads; about one value in 250 is an outlier of 15 to 60 spreads (either sign), so that
    normalised values land beyond +-clip_obs; rewards carry outliers for clip_reward; done marks lane 0, a wave's last
    and first lane and the last row where they exist."""
    cols = np.random.default_rng([seed, dim])                   # column scales are the shape's, not the call's
    scale = 10.0 ** cols.uniform(-3.0, 4.0, dim)
    offset = scale * cols.uniform(-5.0, 5.0, dim)
    rng = np.random.default_rng([seed, B, dim, call])
    z = rng.standard_normal((B, dim))
    out = rng.random((B, dim)) < 0.004
    z = np.where(out, rng.uniform(15.0, 60.0, (B, dim)) * rng.choice([-1.0, 1.0], (B, dim)), z)
    drift = 0.3 * call                                          # the running mean moves between the calls
    obs = (offset + scale * (z + drift)).astype(np.float32)
    reward = 5.0 * rng.standard_normal(B) - 1.0
    big = rng.random(B) < 0.02
    reward = np.where(big, reward * 400.0, reward)
    done = rng.random(B) < 0.05
    for k in (0, 63, 64, B - 1):
        if k < B:
            done[k] = True
    if B > 2:
        done[1] = False
    return obs, reward, done


def vn_eval_stats(dim, epsilon=1e-8):
    """Loaded statistics for the training = 0 call whose scale is exactly 1/2: mean whole numbers, var + epsilon == 4.0
    (asserted by the host test), so that mean +- 2 * clip normalises to exactly +-clip."""
    rng = np.random.default_rng([77, dim])
    mean = rng.integers(100, 200, dim).astype(np.float64) * rng.choice([-1.0, 1.0], dim)    # mean +- 20 stays away from zero
    var = np.full(dim, 4.0 - epsilon)
    return mean, var, 12345.0


def vn_eval_batch(B, dim, clip, seed=5):
    """Rows for ``vn_eval_stats``: N(mean, 2) with, in rows 0..5 of every column, the values that normalise to exactly
    +clip, -clip, and their float32 neighbours on either side."""
    mean, _, _ = vn_eval_stats(dim)
    rng = np.random.default_rng([seed, B, dim])
    obs = (mean + 2.0 * rng.standard_normal((B, dim)) * 3.0).astype(np.float32)
    hi, lo = (mean + 2.0 * clip).astype(np.float32), (mean - 2.0 * clip).astype(np.float32)
    inf = np.float32(np.inf)
    rows = [hi, lo, np.nextafter(hi, inf), np.nextafter(hi, -inf), np.nextafter(lo, inf), np.nextafter(lo, -inf)]
    for r, v in enumerate(rows[:B]):
        obs[r] = v
    return obs


# ---- ill-conditioned columns: |mean| / spread up to 1e7 and a constant column ------------------------------------------
ILL_BATCHES = (65536, 4096)
ILL_COLUMNS = [(5.5338e4, 8e-3), (35040.0, 3e-3), (1e5, 0.1), (1e6, 1.0), (123456.789, 0.0), (730.0, 1e-4), (0.0, 1.0),
               (21.5, 2.0)]
ILL_CONST_COL = 4


def ill_batch(B, seed=31):
    rng = np.random.default_rng([seed, B])
    cols = [np.float32(m) + np.zeros(B, np.float32) if s == 0.0 else (m + s * rng.standard_normal(B)).astype(np.float32)
            for m, s in ILL_COLUMNS]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def two_pass_moments(obs):
    """Column mean and variance (population, like np.var) by the two-pass formula in np.longdouble."""
    x = np.asarray(obs, dtype=np.longdouble)
    m = x.sum(axis=0) / x.shape[0]
    v = np.square(x - m).sum(axis=0) / x.shape[0]
    return m, v


def ill_warm_stats(obs):
    """The columns' exact statistics (two-pass, longdouble, rounded to fp64) with ten batches' worth of count."""
    m, v = two_pass_moments(obs)
    return m.astype(np.float64), v.astype(np.float64), 10.0 * obs.shape[0]


def tol_ratio(got, want, rtol, atol):
    """max |got - want| / (atol + rtol |want|): <= 1 is what np.testing.assert_allclose(rtol, atol) accepts."""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    return float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want)))) if got.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------------
# Weather pipeline
# ---------------------------------------------------------------------------------------------------------------------------
W_INTERVALS = (300.0, 600.0, 900.0, 1800.0, 3600.0)            # ramp lengths int(3600 / dt) = 12, 6, 4, 2, 1
W_N_RAW = (3, 4, 5, 24, 25, 26, 255, 256, 257, 289, 577, 1999)
W_STARTS = ("midnight", "before_midnight", "midday", "odd", "day100")
W_RADIATION = ("clear", "night", "always", "dropouts", "pulses", "edges")
W_STRESS = ("flat_runs", "zigzag", "jump", "monotone_equal", "cross_zero")
DAY = 86400.0


def _start_time(kind, dt):
    return {"midnight": 20 * DAY, "before_midnight": 20 * DAY - dt, "midday": 20 * DAY + 43200.0, "odd": 12345.0,
            "day100": 100 * DAY + 150.0}[kind]


def weather_cases(dt):
    """The cases of one raw interval: every (radiation, start) pair, with n_raw and the grid (uniform / jittered) cycling so
    that each n_raw meets both grids.  -> list of dicts for ``weather_raw``."""
    di = W_INTERVALS.index(dt)
    cases = []
    for ri, rad in enumerate(W_RADIATION):
        for si, start in enumerate(W_STARTS):
            idx = ri * len(W_STARTS) + si
            cases.append(dict(dt=dt, n=W_N_RAW[(idx + 5 * di) % len(W_N_RAW)], start=start, rad=rad,
                              jitter=bool((idx + idx // len(W_N_RAW) + di) % 2), idx=idx,
                              stress=tuple(W_STRESS[(idx + di + j) % len(W_STRESS)] for j in range(3))))
    return cases


def case_id(c):
    return f"dt{int(c['dt'])}-n{c['n']}-{c['start']}-{c['rad']}-{'jit' if c['jitter'] else 'uni'}"


def n_out_list(n):
    return sorted({1, 2, n, 3 * n + 1, max(n // 3, 1)})


def _stress_series(kind, n, rng, lo, hi):
    """PCHIP stress data in [lo, hi]: the cases of the slope kernel (m0 == 0 runs, sign changes at every knot, one huge
    secant among small ones, equal neighbours inside a monotone run, values through zero)."""
    k = np.arange(n)
    mid, amp = 0.5 * (lo + hi), 0.5 * (hi - lo)
    if kind == "flat_runs":
        y = mid + amp * 0.8 * np.repeat(rng.uniform(-1, 1, n // 3 + 1), 3)[:n]
    elif kind == "zigzag":
        y = mid + amp * 0.5 * np.where(k % 2 == 0, 1.0, -1.0) * rng.uniform(0.2, 1.0, n)
    elif kind == "jump":
        y = np.full(n, lo + 0.01 * amp) + 1e-3 * amp * rng.random(n)
        y[n // 2:] = hi - 0.01 * amp - 1e-3 * amp * rng.random(n - n // 2)
    elif kind == "monotone_equal":
        inc = rng.uniform(0.1, 1.0, n)
        inc[rng.random(n) < 0.2] = 0.0
        inc[0] = 0.0
        if n > 2:
            inc[2] = 0.0                                        # equal neighbours next to the end-point formula too
        y = np.cumsum(inc)
        y = lo + 0.05 * amp + (y / max(y[-1], 1e-30)) * 1.9 * amp
    else:                                                       # cross_zero: a slow wave about zero plus noise
        c = 0.0 if lo < 0.0 < hi else mid
        y = c + min(abs(hi - c), abs(c - lo)) * (0.7 * np.sin(0.37 * k + rng.uniform(0, 6)) + 0.2 * rng.uniform(-1, 1, n))
    return np.clip(y, lo, hi)


def weather_raw(c, seed=9):
    """-> (time, i_glob, t_out, rh, wind, t_sky), float64 [n] each."""
    dt, n = c["dt"], c["n"]
    rng = np.random.default_rng([seed, int(dt), n, c["idx"], int(c["jitter"])])
    k = np.arange(n, dtype=np.float64)
    if c["jitter"]:
        j = rng.uniform(-0.27, 0.27, n)
        j[0], j[-1] = 0.02, -0.02          # mean(diff) a little BELOW dt: 3600 / mean stays just above the even ramp length
        time = np.sort(_start_time(c["start"], dt) + dt * (k + j))
    else:
        time = _start_time(c["start"], dt) + dt * k
    tod = np.mod(time, DAY)
    sun = np.maximum(np.sin(2 * np.pi * (tod - 6 * 3600.0) / DAY), 0.0)
    clear = np.where(sun > 0, 3.0 + 800.0 * sun, 0.0)
    n_tr = int(3600.0 / dt)
    rad = c["rad"]
    if rad == "clear":
        g = clear
    elif rad == "night":
        g = np.zeros(n)
    elif rad == "always":
        g = 40.0 + 300.0 * np.abs(np.sin(2 * np.pi * tod / DAY))
    elif rad == "dropouts":                 # single dark samples in daylight: repeated sunsets, overlapping ramps
        g = np.where(rng.random(n) < 0.12, 0.0, 40.0 + clear)
    elif rad == "pulses":
        g = np.where(rng.random(n) < 0.08, rng.uniform(5.0, 900.0, n), 0.0)
    else:                                   # edges: sunrise inside the first ramp length of samples, sunset inside the last
        g = 30.0 + 500.0 * rng.random(n)
        a = max(1, min(n_tr - 1, n // 3))
        g[:a] = 0.0
        g[n - a:] = 0.0
    t_out = _stress_series(c["stress"][0], n, rng, -30.0, 45.0)
    wind = _stress_series(c["stress"][1], n, rng, -4.0, 4.0e6 if c["stress"][1] == "jump" else 25.0)
    t_sky = _stress_series(c["stress"][2], n, rng, -60.0, 30.0)
    rh = rng.uniform(30.0, 100.0, n)
    return tuple(np.ascontiguousarray(v, dtype=np.float64) for v in (time, g, t_out, rh, wind, t_sky))


def ramp_length(time):
    dt = np.mean(np.diff(time - time[0]))
    return int(3600 / dt), 3600 / dt


def weather_knots(time, i_glob, t_out, rh, wind, t_sky, co2_ppm=400):
    """The ten converted columns on the raw grid, [n, 10]: gl_gym_amd.utils.weather_from_raw before its resample."""
    from gl_gym_amd import utils as U
    time = np.asarray(time, dtype=np.float64)
    dt = np.mean(np.diff(time - time[0]))
    w = np.zeros((len(time), 10))
    w[:, 0] = i_glob
    w[:, 1] = t_out
    w[:, 2] = U.vaporDens2pres(w[:, 1], U.rh2vaporDens(w[:, 1], np.asarray(rh, dtype=np.float64)))
    w[:, 3] = U.co2ppm2dens(w[:, 1], co2_ppm) * 1e6
    w[:, 4] = wind
    w[:, 5] = t_sky
    w[:, 6] = U.soilTempNl(time)
    w[:, 7] = U.daily_light_sum(time, w[:, 0])
    w[:, 8], w[:, 9] = U.compute_is_day(w[:, 0], dt)
    return w


def weather_host(time, knots, n_out):
    """weather_from_raw's resample with n_out given rather than derived -> (table [n_out, 10], iGlob before its clean-up)."""
    from scipy.interpolate import PchipInterpolator
    out = PchipInterpolator(time, knots)(np.linspace(time[0], time[-1], n_out))
    raw0 = out[:, 0].copy()
    out[:, 0][out[:, 0] < 1e-10] = 0
    return out, raw0
