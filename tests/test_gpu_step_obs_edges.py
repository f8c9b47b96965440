"""The observation epilogue of the step kernel (csrc/glgym.hip step_kernel, `if constexpr (OBS)`) at the shapes where it can go wrong:
glgym_step_obs and glgym_step_obs_reset through the C ABI, into an observation buffer of the test's own.

Every scenario runs two environments with the same seed.  R, the reference, is stepped by the plain glgym_step and observed by glgym_obs
(obs_kernel, full mode), then -- where the step auto-resets -- reset by glgym_reset over `done` and observed again in masked mode with
the terminal rows saved.  E is stepped by glgym_step_obs / glgym_step_obs_reset: the kernel with the epilogue.  Compared for equality of
bits: the observation block, the terminal rows of the finished environments, the state and bookkeeping of the step; and E's forecast
columns against the rule restated in numpy, weather[clip(w_off + max(ts1 - 1, 0) + 1 + i, 0, rows - 1), c].  E's observation and
terminal blocks are pre-filled with NaN (every element must have been written) and followed by guard rows that must come back as
they were.

Shapes: B = 1, 63, 64, 65, 80 (one partial strip; three full strips and a partial one; a full wavefront; a second wavefront with one
live lane whose dead lanes shadow row B - 1; a second wavefront of one strip).  Forecast module off, Np = 1, 13 (65 elements: one pass of
the wavefront and one lane) and 48.  Table ends: a table so short that every window clamps, one environment of the first wavefront at
the high end, one below the low end (each makes its whole wavefront take the clamped strips), none, and w_off = 0 at timestep 0.  Two
env-steps per scenario: the first finishes nothing, the second finishes every third environment and, with B > 5, one whose integration
fails.  ls5 and rk4, one- and two-waves builds, default and handle parameters, per-environment crop blocks (which have the observation
epilogue and no auto-reset epilogue: there the library runs reset and masked observation as launches of their own)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BATCHES = (1, 63, 64, 65, 80)
FORECASTS = ("off", 1, 13, 48)
ENDS = ("none", "every", "one_high", "one_low", "zero")
CONFIGS = {
    "ls5": dict(scheme="ls5"),
    "rk4": dict(scheme="rk4"),
    "ls5_two_waves": dict(scheme="ls5", occ=2),
    "rk4_two_waves": dict(scheme="rk4", occ=2),
    "ls5_crop": dict(scheme="ls5", uncertainty_scale=0.2),
    "rk4_crop": dict(scheme="rk4", uncertainty_scale=0.2),
    "ls5_handle_params": dict(scheme="ls5", params="handle"),
}
GUARD_ROWS = 3
GUARD = 12345.0
NO_FORECAST = ["IndoorClimateObservations", "BasicCropObservations", "ControlObservations", "WeatherObservations", "TimeObservations"]
STATE = ("x_T", "u_T", "timestep_t", "w_off_t", "start_day_t", "episode_t", "reward_t", "done_t", "info_T", "step_flags_t")
_W = []


def weather():
    if not _W:
        from gl_gym_amd.utils import synthetic_weather
        _W.append(synthetic_weather(n_rows=1000))
    return _W[0]


def handle_params():
    from gl_gym_amd.parameters import init_default_params
    p = np.asarray(init_default_params(), dtype=np.float64).copy()
    p[:127] *= 1 + 0.01 * np.random.default_rng(42).uniform(-1, 1, 127)
    return p.astype(np.float32)


def make_env(B, forecast, scheme="ls5", occ=1, params=None, **kw):
    from gl_gym_amd.tomato_env import TomatoVecEnv
    Np = 48 if forecast == "off" else forecast
    env = TomatoVecEnv(B, weather=weather(), dtype="float32", scheme=scheme, season_length=1, pred_horizon=(Np + 0.5) * 900.0 / 86400.0, seed=11,
                       start_rows=[0, 96, 480], observation_modules=NO_FORECAST if forecast == "off" else None,
                       params=handle_params() if params == "handle" else None, **kw)
    assert env.Np == Np
    env.set_layout("one")
    env.set_occupancy(occ)
    env.reset_tensor()
    return env


def bits(t):
    import torch
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


class Stepper:
    """One environment driven through the C ABI with a weather_rows of the test's choosing."""

    def __init__(self, env, rows):
        import torch
        from gl_gym_amd import _lib as L
        self.L, self.lib, self.env, self.rows = L, L.load(), env, rows
        n = (env.B + GUARD_ROWS) * env.obs_dim
        self.obs = torch.full((n,), float("nan"), dtype=torch.float32, device=env.device)
        self.term = torch.full((n,), float("nan"), dtype=torch.float32, device=env.device)
        for t in (self.obs, self.term):
            t[env.B * env.obs_dim:] = GUARD

    def block(self, t):
        return t[:self.env.B * self.env.obs_dim].view(self.env.B, self.env.obs_dim)

    def guard_intact(self):
        e = self.env
        return bool((self.obs[e.B * e.obs_dim:] == GUARD).all()) and bool((self.term[e.B * e.obs_dim:] == GUARD).all())

    def step_args(self, action):
        e, L = self.env, self.L
        e.action_t.copy_(action)
        if e.crop_T is not None:                      # a fresh draw every step, the same in both twins (seed, draw counter)
            L.check(self.lib.glgym_crop_noise(e._h, e.crop_T.data_ptr(), e.B, e.ld, e.uncertainty_scale, e.seed_value, e._draw, e._stream()),
                    "glgym_crop_noise")
            e._draw += 1
        return L.make_step_args(e.B, e.ld, e.x_T.data_ptr(), e.u_T.data_ptr(), e.action_t.data_ptr(), None, e.weather_t.data_ptr(), self.rows,
                                e.w_off_t.data_ptr(), e.timestep_t.data_ptr(), e.crop_T.data_ptr() if e.crop_T is not None else None, e.N,
                                e.reward_t.data_ptr(), e.info_T.data_ptr(), e.done_t.data_ptr(), None, e.step_flags_t.data_ptr())

    def obs_args(self, mask=None, term=None):
        e = self.env
        return self.L.ObsArgs(e.B, e.ld, e.x_T.data_ptr(), e.u_T.data_ptr(), e.weather_t.data_ptr(), self.rows, e.w_off_t.data_ptr(),
                              e.timestep_t.data_ptr(), e.start_day_t.data_ptr(), e.Np, self.obs.data_ptr(),
                              mask.data_ptr() if mask is not None else None, term.data_ptr() if term is not None else None)

    def reset_args(self):
        e = self.env
        return self.L.ResetArgs(e.B, e.ld, e.done_t.data_ptr(), e.x_T.data_ptr(), e.u_T.data_ptr(), e.timestep_t.data_ptr(),
                                e.weather_t.data_ptr(), self.rows, e.w_off_t.data_ptr(), e._start_rows_t.data_ptr(), e._start_days_t.data_ptr(),
                                len(e.start_rows), e.start_day_t.data_ptr(), e.episode_t.data_ptr(), e.seed_value)

    def unfused(self, action, with_reset):
        e, L, lib = self.env, self.L, self.lib
        a = self.step_args(action)
        L.check(lib.glgym_step(e._h, C.byref(a), e._stream()), "glgym_step")
        L.check(lib.glgym_obs(e._h, C.byref(self.obs_args()), e._stream()), "glgym_obs")
        if with_reset:
            L.check(lib.glgym_reset(e._h, C.byref(self.reset_args()), e._stream()), "glgym_reset")
            L.check(lib.glgym_obs(e._h, C.byref(self.obs_args(e.done_t, self.term)), e._stream()), "glgym_obs")

    def fused(self, action, with_reset):
        """Returns the epilogue bits of the build the step launched (8: observation, 24: observation and auto-reset; 0: none)."""
        e, L, lib = self.env, self.L, self.lib
        a = self.step_args(action)
        if with_reset:
            L.check(lib.glgym_step_obs_reset(e._h, C.byref(a), C.byref(self.obs_args(None, self.term)), C.byref(self.reset_args()),
                                             e._stream(), None), "glgym_step_obs_reset")
        else:
            L.check(lib.glgym_step_obs(e._h, C.byref(a), C.byref(self.obs_args()), e._stream()), "glgym_step_obs")
        out = (C.c_int32 * 10)()
        L.check(lib.glgym_last_step_build(e._h, out), "glgym_last_step_build")
        return out[6] if out[9] else 0


def place(envs, end):
    """The table-end scenario: the weather_rows both twins' launches state, after moving the windows of chosen environments."""
    rows = envs[0].weather_rows
    for e in envs:
        if end == "every":
            pass
        elif end == "one_high":                       # its window runs past the last row from its 10th forecast row on (Np = 1: its only one)
            e.w_off_t[min(e.B - 1, 37)] = rows - min(e.Np, 10)
        elif end == "one_low":                        # its first forecast rows lie before the table
            e.w_off_t[min(e.B - 1, 5)] = -7
        elif end == "zero":
            e.w_off_t.zero_()
            e.timestep_t.zero_()
    return 20 if end == "every" else rows


def forecast_by_rule(env, rows):
    """[B, 5 Np]: the forecast columns of the state as it stands."""
    w = env.weather_t.cpu().numpy()
    w_off, ts1 = env.w_off_t.cpu().numpy().astype(np.int64), env.timestep_t.cpu().numpy().astype(np.int64)
    r = np.clip(w_off[:, None] + np.maximum(ts1 - 1, 0)[:, None] + 1 + np.arange(env.Np)[None, :], 0, rows - 1)
    return w[r][:, :, :5].reshape(env.B, 5 * env.Np)


def scenario(R, E, end, expect_epi):
    import torch
    B = R.B
    for e in (R, E):
        e.reset_tensor()
        e.timestep_t[0:B:2] += 7                      # windows at different rows inside a strip
    rows = place((R, E), end)
    sr, se = Stepper(R, rows), Stepper(E, rows)
    g = torch.Generator().manual_seed(5)
    acts = (torch.rand(2, B, 6, generator=g) * 2 - 1).to(device=R.device, dtype=torch.float32)
    for i, with_reset in enumerate((False, True)):
        if with_reset:
            for e in (R, E):
                e.timestep_t[0:B:3] = e.N             # these finish: the step ends an episode whose timestep is >= N
                if B > 5:
                    e.x_T[2, 5] = float("nan")        # and this one fails
            se.block(se.obs).fill_(float("nan"))
        sr.unfused(acts[i], with_reset)
        epi = se.fused(acts[i], with_reset)
        assert epi == (expect_epi[1] if with_reset else expect_epi[0]), (epi, i)
        where = (end, i)
        for name in STATE:
            assert torch.equal(bits(getattr(R, name)), bits(getattr(E, name))), (name, where)
        assert torch.equal(bits(sr.block(sr.obs)), bits(se.block(se.obs))), ("obs", where)
        assert se.guard_intact() and sr.guard_intact(), ("guard rows", where)
        if R.observation_modules[-1].name == "WeatherForecastObservations":
            got = se.block(se.obs)[:, R.obs_dim - 5 * R.Np:].cpu().numpy()
            assert np.array_equal(got.view(np.int32), forecast_by_rule(E, rows).astype(np.float32).view(np.int32)), ("forecast rule", where)
        if with_reset:
            done = R.done_t.bool()
            assert bool(done[0]) and (B <= 5 or bool(done[5])) and (B < 2 or not bool(done.all()))
            assert torch.equal(bits(sr.block(sr.term)[done]), bits(se.block(se.term)[done])), ("term_obs", where)
            assert bool(torch.isnan(se.block(se.term)[~done]).all()), ("term_obs rows of unfinished environments", where)


@pytest.mark.parametrize("forecast", FORECASTS, ids=lambda f: f"np{f}")
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_step_obs_epilogue_equals_obs_kernel(cfg, B, forecast):
    c = CONFIGS[cfg]
    R, E = make_env(B, forecast, **c), make_env(B, forecast, **c)
    # the builds this configuration has: the observation epilogue everywhere, the auto-reset epilogue with shared crop parameters
    expect_epi = (8, 8 if "uncertainty_scale" in c else 24)
    for end in ENDS:
        scenario(R, E, end, expect_epi)
    R.close(); E.close()
