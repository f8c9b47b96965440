"""Batched TomatoEnv on the MI355X.

``TomatoVecEnv`` keeps B independent greenhouse environments resident in HBM (state, controls, clocks,
weather window offsets) and advances all of them with ONE fused kernel launch per env-step
(libglgym.so: glgym_step), then assembles the row-major observation block (glgym_obs).  It exposes

  * the Stable-Baselines3 ``VecEnv`` calling convention that the reference's experiment manager consumes
    (gl_gym/RL/utils.py:44-69, gl_gym/common/evaluation.py:73-104): reset() / step(actions) -> (obs, rewards,
    dones, infos) with auto-reset and ``infos[i]["terminal_observation"]``, step_async/step_wait, num_envs,
    observation_space / action_space, get_attr / set_attr / env_method / env_is_wrapped / close;
  * a zero-copy tensor interface (``step_tensor``) for device-resident RL loops.

``TomatoEnv`` is the single-environment Gymnasium-style view (reset(seed) -> (obs, {}), step(a) ->
(obs, reward, terminated, False, info)) with the attributes the reference's tooling reads
(x, u, p, N, Np, timestep, weather_data, start_day, growth_year, ...; tomato_env.py:28-270).

Semantics reproduced from the reference (file:line in gl_gym/environments/):
  action -> control clip            tomato_env.py:109-113      episode = N+1 steps        tomato_env.py:131-137
  weather row = timestep (pre-++)   tomato_env.py:120          obs at step k uses row k   observations.py:133,161
  reward / info keys                rewards.py:218-231, tomato_env.py:208-222
  ODE failure -> terminated, x kept tomato_env.py:119-123
PyTorch is used for device memory, streams and RNG plumbing only; all arithmetic is in the HIP kernels.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _lib as L
from . import np_stream
from .greenlight_model import _check_integrator, _check_tolerances
from .parameters import init_default_params
from .step_fusion import StepFusion
from .utils import synthetic_weather

try:  # spaces are optional plumbing: use gymnasium's when present
    from gymnasium import spaces as _spaces

    def _box(low, high, shape, dtype=np.float32):
        return _spaces.Box(low=low, high=high, shape=shape, dtype=dtype)
except Exception:  # pragma: no cover - gymnasium is absent in the build image
    class _Box:
        def __init__(self, low, high, shape, dtype):
            self.low = np.broadcast_to(np.asarray(low, dtype=dtype), shape).copy()
            self.high = np.broadcast_to(np.asarray(high, dtype=dtype), shape).copy()
            self.shape, self.dtype = tuple(shape), np.dtype(dtype)
            self._rng = np.random.default_rng()

        def seed(self, seed=None):
            self._rng = np.random.default_rng(seed)

        def sample(self):
            return self._rng.uniform(self.low, self.high).astype(self.dtype)

        def contains(self, v):
            v = np.asarray(v)
            return v.shape == self.shape and bool(np.all(v >= self.low) and np.all(v <= self.high))

    def _box(low, high, shape, dtype=np.float32):
        return _Box(low, high, shape, dtype)

DEFAULT_REWARD = dict(fixed_greenhouse_cost=15., fixed_co2_cost=0.015, fixed_lamp_cost=0.07, fixed_screen_cost=2.,
                      elec_price=0.3, heating_price=0.09, co2_price=0.3, fruit_price=1.6, dmfm=0.065,
                      pen_weights=[4.e-4, 5.e-3, 7.e-4], pen_lamp=0.1)               # TomatoEnv.yml:56-67
DEFAULT_CONSTRAINTS = dict(co2_min=300., co2_max=1600., temp_min=15., temp_max=34., rh_min=50., rh_max=85.)


def _torch():
    import torch
    return torch


RNGS = ("philox", "numpy")


def _check_rng(rng, start_grid, n_starts):
    """-> (rng, start_grid) as TomatoVecEnv stores them.  rng = "numpy" without a grid means (1, n_starts): one year, every start a day."""
    if rng not in RNGS:
        raise ValueError("rng must be 'philox' or 'numpy'")
    if start_grid is None:
        return rng, ((1, int(n_starts)) if rng == "numpy" else None)
    grid = tuple(int(v) for v in start_grid)
    if len(grid) != 2 or grid[0] < 1 or grid[1] < 1 or grid[0] * grid[1] != int(n_starts):
        raise ValueError(f"start_grid must be (n_years, n_days) with n_years * n_days = len(start_rows) = {n_starts}, got {start_grid!r}")
    return rng, grid


def _observation_modules(Np, names):       # TomatoVecEnv.__init__ has a keyword argument of the same name as the function
    return observation_modules(Np, names)


class ObservationModule:
    """Descriptor of one of the reference's observation modules (observations.py:59-182): what the experiment manager
    reads through ``env.get_attr("observation_modules")`` (RL/experiment_manager.py:43-45).  The values themselves are
    produced by glgym_obs; ``low`` / ``high`` are the module's Box bounds as the reference declares them."""

    def __init__(self, name, obs_names, low=-1e-4, high=1e4):
        self.name, self.obs_names, self.n_obs, self.low, self.high = name, list(obs_names), len(obs_names), low, high

    def __repr__(self):
        return f"{self.name}({self.n_obs})"


OBSERVATION_MODULE_IDS = {"IndoorClimateObservations": 0, "BasicCropObservations": 1, "ControlObservations": 2,
                          "WeatherObservations": 3, "TimeObservations": 4, "WeatherForecastObservations": 5}   # GLGYM_OBS_*
DEFAULT_OBSERVATION_MODULES = ["IndoorClimateObservations", "BasicCropObservations", "ControlObservations",
                               "WeatherObservations", "TimeObservations", "WeatherForecastObservations"]  # TomatoEnv.yml:25-32


def observation_modules(Np: int, names: Optional[Sequence[str]] = None):
    """Descriptors of the configured modules, in the order of the list = the column layout of glgym_obs
    (tomato_env.py:77-81, 193-198).  Default: the six of configs/envs/TomatoEnv.yml."""
    wx = ["glob_rad", "temp_out", "rh_out", "co2_out", "wind_speed"]
    table = {"IndoorClimateObservations": (["co2_air", "temp_air", "rh_air", "pipe_temp"],),
             "BasicCropObservations": (["24CanTemp", "cFruit", "tSum"],),
             "ControlObservations": (["uBoil", "uCo2", "uThScr", "uVent", "uLamp", "uBlScr"], 0.0, 1.0),
             "WeatherObservations": (wx,),
             "TimeObservations": (["timestep", "day of year sin", "day of year cos", "hour of day sin",
                                   "hour of day cos"],),
             "WeatherForecastObservations": (wx * Np,)}
    names = DEFAULT_OBSERVATION_MODULES if names is None else list(names)
    for n in names:
        if n == "StateObservations":
            raise NotImplementedError("StateObservations cannot be built by the reference's TomatoEnv either "
                                      "(observations.py:42: __init__ takes no env) and returns random numbers (:57)")
        if n not in table:
            raise KeyError(f"unknown observation module {n!r}; known: {sorted(table)}")
    if len(set(names)) != len(names) or not names:
        raise ValueError("observation_modules must be a non-empty list without repeats")
    return [ObservationModule(n, *table[n]) for n in names]


class LazyInfos:
    """List-like view of the per-env info dicts (SB3: ``infos[i]``).  Dicts are built on first access and cached, so
    wrappers that only touch finished envs (VecMonitor, VecNormalize) cost O(#done), not O(B), per step."""

    def __init__(self, keys, info_rows, controls, dones, term_obs, step_flags=None):
        self._keys, self._rows, self._ctrl, self._dones, self._term = keys, info_rows, controls, dones, term_obs
        self._flags = step_flags
        self._cache = {}

    def __len__(self):
        return len(self._rows)

    def _make(self, b):
        d = dict(zip(self._keys, self._rows[b].tolist()))
        d["controls"] = self._ctrl[b]
        d["TimeLimit.truncated"] = False
        if self._flags is not None:
            d["integration"] = int(self._flags[b])        # GLGYM_SF_* word: 0 = first attempt accepted as it stood
        if self._term is not None and self._dones[b]:
            d["terminal_observation"] = self._term[b]
        return d

    def __getitem__(self, b):
        if isinstance(b, slice):
            return [self[i] for i in range(*b.indices(len(self)))]
        b = int(b)
        if b < 0:
            b += len(self)
        if b not in self._cache:
            self._cache[b] = self._make(b)
        return self._cache[b]

    def __setitem__(self, b, value):
        self._cache[int(b)] = value

    def __iter__(self):
        return (self[i] for i in range(len(self)))


class _EpochLib:
    """The library as a TomatoVecEnv sees it: every call through it -- kernel launches, setters, whatever a caller does with `env._lib` and
    `env._h` through raw pointers -- advances the epoch of the environment's StepFusion first, which invalidates the tokens of a fused
    step.  Wrappers are made once per entry point."""

    def __init__(self, lib, fusion):
        self.__dict__["_lib"], self.__dict__["_fusion"] = lib, fusion

    def __getattr__(self, name):
        fn, advance = getattr(self._lib, name), self._fusion.advance

        def call(*args):
            advance()
            return fn(*args)
        self.__dict__[name] = call
        return call


class TomatoVecEnv:
    def __init__(self, num_envs: int, weather: Optional[np.ndarray] = None, params: Optional[np.ndarray] = None,
                 dt: float = 900.0, season_length: float = 60, pred_horizon: float = 0.5, dtype: str = "float32",
                 n_sub: Optional[int] = None, device: str = "cuda:0", seed: int = 0, uncertainty_scale: float = 0.0,
                 start_rows: Optional[Sequence[int]] = None, start_days: Optional[Sequence[float]] = None,
                 reward_params: Optional[Dict[str, Any]] = None, constraints: Optional[Dict[str, float]] = None,
                 auto_reset: bool = True, collect_metrics: bool = True, lazy_infos: Optional[bool] = None,
                 model_variant: str = "ode", scheme: Optional[str] = None, window: Optional[int] = None,
                 preset: Optional[str] = None,
                 observation_modules: Optional[Sequence[str]] = None, u_min: Optional[Sequence[float]] = None,
                 u_max: Optional[Sequence[float]] = None, delta_u_max: float = 0.1, integration_info: bool = True,
                 integrator: str = "explicit", rtol: float = 1e-6, atol: float = 1e-6, max_steps: int = 10000,
                 rng: str = "philox", start_grid: Optional[Sequence[int]] = None, env_index_offset: int = 0):
        """u_min / u_max / delta_u_max: action_to_control's bounds (base_env.py:72-74; default [0, 1] and 0.1).
        observation_modules: names of the reference's modules in output order (default: the six of TomatoEnv.yml).
        scheme / n_sub / window: "ls5" (default; model_variant "ode_pipe" defaults to "rk4" and accepts no other: five-stage fourth-order 2N-storage scheme, n_sub 128, two sub-steps per tier-2b window), "rk4" (classical RK4, 240),
        "rk3" (three-stage third-order scheme, 270) or "rk2" (midpoint rule, 336), all with the cover conduction integrated exactly (include/glgym.h).
        preset: "throughput" (the counts above; default for float32) or "parity" (inside the band of the reference solver's tolerances:
        ls5 n_sub 192 with one sub-step per window; default for float64) -- used for whatever of n_sub / window is not given (_lib.PRESETS);
        integration_info: put the per-env GLGYM_SF_* word of each step into infos[i]["integration"] (one more B x 4-byte D2H copy
        per host-side step; False: not copied, key absent -- the device tensor `step_flags_t` is always written);
        weather: [rows, nd] with nd = 10, or 14 when the rows carry the measured pipe columns
        (experiments/gl_predefined_controls.py:95, 107).  model_variant = "ode" | "ode_pipe" (ode.hpp:126-263, nd >= 14).
        integrator: "explicit" (default: the scheme / n_sub / window above) or "bdf" -- every env-step integrated by the adaptive,
        error-controlled variable-order BDF in fp64 at rtol / atol, at most max_steps steps per env-step (include/glgym.h
        glgym_set_step_integrator; the algorithm family of the reference's CVODES call); scheme, n_sub, window and preset stay stored and
        apply again after set_integrator("explicit").  "bdf" does not combine with model_variant "ode_pipe".
        rng: "philox" (default: counter-based draws keyed by (seed, env, draw counter)) or "numpy": every environment owns the NumPy
        generator the reference's TomatoEnv owns, Generator(PCG64(SeedSequence(seed + env_index_offset + b))) (RL/utils.py:39: make_env seeds
        environment `rank` with seed + rank), kept on the device (include/glgym.h glgym_rng_*) and drawn from in the reference's order: at a
        reset choice(years), choice(days) (tomato_env.py:236-241), at every step 34 uniforms whether or not uncertainty_scale is 0
        (tomato_env.py:118).  Start rows, start days and crop blocks then equal the reference's bit for bit.  A reset without a seed continues
        the streams (gymnasium.Env.reset(seed=None)); reset_tensor(seed=s) / seed(s) / set_seed(s) reseed; get_rng_state / set_rng_state.
        start_grid: (n_years, n_days) of the year-major start table (make_env.season_table), n_years * n_days = len(start_rows); default
        (1, len(start_rows)).  env_index_offset: global index of this shard's first environment (rng="numpy" only)."""
        _check_integrator(integrator, model_variant)
        _check_tolerances(rtol, atol, max_steps)
        _check_rng(rng, start_grid, 1 if start_rows is None else len(start_rows))
        torch = _torch()
        if not torch.cuda.is_available():
            raise L.GlgymError("TomatoVecEnv needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self._fusion = StepFusion()         # what the last _launch_step has already done: _launch_step / _launch_obs / _launch_reset
        self._lib = _EpochLib(L.load(), self._fusion)
        self.torch = torch
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        self.num_envs = self.B = int(num_envs)
        self.ld = (self.B + 63) // 64 * 64
        self.dt = float(dt)
        self.c = 86400
        self.nx, self.nu, self.num_params = L.NX, L.NU, L.NP
        weather_is_tensor = weather is not None and hasattr(weather, "data_ptr")          # a torch tensor (device table)
        self.nd = L.ND if weather is None else int(np.shape(weather)[1])        # arrays and nested lists alike
        if model_variant not in ("ode", "ode_pipe"):
            raise ValueError("model_variant must be 'ode' or 'ode_pipe'")
        self.model_variant = model_variant
        self.season_length = season_length
        self.N = int(season_length * self.c / self.dt)                     # base_env.py:88
        self.Np = int(pred_horizon * self.c / self.dt)                     # base_env.py:80
        self.observation_modules = _observation_modules(self.Np, observation_modules)
        if self.observation_modules[0].name != "IndoorClimateObservations":
            # GreenhouseReward reads its constraint inputs positionally, obs[[0, 1, 2]] = co2_air, temp_air, rh_air
            # (rewards.py:192-194): with another module first the reference penalises whatever lands in those slots
            raise NotImplementedError("observation_modules must start with IndoorClimateObservations: the reference's "
                                      "GreenhouseReward takes co2 / temperature / humidity from obs[0:3]")
        self.obs_dim = sum(m.n_obs for m in self.observation_modules)
        self.f64 = str(dtype) in ("float64", "f64", "double")
        self.tdtype = torch.float64 if self.f64 else torch.float32
        scheme = L.resolve_scheme(scheme, model_variant)     # None: "ls5"; "rk4" for ode_pipe (the only scheme its kernels are built for)
        self.preset = ("parity" if self.f64 else "throughput") if preset is None else preset
        if self.preset not in L.PRESETS:
            raise ValueError("preset must be 'throughput' or 'parity'")
        self.scheme = scheme
        n_def, w_def = L.preset_n_sub(scheme, self.dt, self.preset)
        self.n_sub = int(n_def if n_sub is None else n_sub)
        self.window = int((w_def if n_sub is None else 0) if window is None else window)      # 0 = the scheme's own
        self.uncertainty_scale = float(uncertainty_scale)
        self.auto_reset = auto_reset
        self.lazy_infos = (int(num_envs) > 4096) if lazy_infos is None else bool(lazy_infos)
        self.integration_info = bool(integration_info)
        self.seed_value = int(seed)

        self._p = np.asarray(init_default_params(L.NP) if params is None else params, dtype=np.float32)
        self._h = C.c_void_p()
        p64 = np.ascontiguousarray(self.p, dtype=np.float64)
        L.check(self._lib.glgym_create(L.NX, L.NU, self.nd, L.NP, self.dt, p64.ctypes.data_as(L._DP),
                                       L.F64 if self.f64 else L.F32, self.n_sub, self.device.index or 0,
                                       C.byref(self._h)), "glgym_create")
        # GLGYM_LAYOUT / GLGYM_OCC / GLGYM_VERIFY are read ONCE, here in glgym_create (handle state since round 5): changing os.environ
        # afterwards has no effect on this handle -- _launch_step warns once if that is attempted (use set_layout / set_occupancy / set_verify)
        self._env_at_create = tuple(os.environ.get(k) for k in ("GLGYM_LAYOUT", "GLGYM_OCC", "GLGYM_VERIFY"))
        if model_variant == "ode_pipe":
            L.check(self._lib.glgym_set_model_variant(self._h, L.ODE_PIPE), "glgym_set_model_variant")
        L.check(self._lib.glgym_set_scheme(self._h, L.SCHEMES[scheme]), "glgym_set_scheme")
        L.check(self._lib.glgym_set_window(self._h, self.window), "glgym_set_window")
        self.rtol, self.atol, self.max_steps = float(rtol), float(atol), int(max_steps)
        self.set_integrator(integrator)
        self.u_min = np.asarray([0.0] * L.NU if u_min is None else u_min, dtype=np.float32)            # base_env.py:72-74
        self.u_max = np.asarray([1.0] * L.NU if u_max is None else u_max, dtype=np.float32)
        self.delta_u_max = np.ones(L.NU, dtype=np.float32) * np.float32(delta_u_max)
        if self.u_min.shape != (L.NU,) or self.u_max.shape != (L.NU,):
            raise ValueError("u_min / u_max must have 6 entries")
        lo64, hi64 = self.u_min.astype(np.float64), self.u_max.astype(np.float64)
        L.check(self._lib.glgym_set_control_limits(self._h, lo64.ctypes.data_as(L._DP), hi64.ctypes.data_as(L._DP),
                                                   float(delta_u_max)), "glgym_set_control_limits")
        ids = (C.c_int32 * len(self.observation_modules))(*[OBSERVATION_MODULE_IDS[m.name] for m in self.observation_modules])
        L.check(self._lib.glgym_set_obs_modules(self._h, ids, len(ids)), "glgym_set_obs_modules")
        assert self._lib.glgym_obs_dim(self._h, self.Np) == self.obs_dim
        rp = dict(DEFAULT_REWARD, **(reward_params or {}))
        cs = dict(DEFAULT_CONSTRAINTS, **(constraints or {}))
        self.reward_params, self.constraints = rp, cs
        cfg = L.RewardCfg(rp["elec_price"], rp["heating_price"], rp["co2_price"], rp["fruit_price"], rp["dmfm"],
                          rp["fixed_greenhouse_cost"], rp["fixed_co2_cost"], rp["fixed_lamp_cost"],
                          rp["fixed_screen_cost"], rp["pen_lamp"], cs["co2_min"], cs["co2_max"], cs["temp_min"],
                          cs["temp_max"], cs["rh_min"], cs["rh_max"])
        L.check(self._lib.glgym_set_reward(self._h, C.byref(cfg)), "glgym_set_reward")
        mx, mn, fx = C.c_double(), C.c_double(), C.c_double()
        L.check(self._lib.glgym_get_reward_scale(self._h, C.byref(mx), C.byref(mn), C.byref(fx)))
        self.max_profit, self.min_profit, self.fixed_costs = mx.value, mn.value, fx.value

        # ---- weather tensor (shared by all envs) and the admissible episode start rows
        if weather is None:
            weather = synthetic_weather(dt=self.dt)
        self._weather_data = (weather.detach().double().cpu().numpy() if weather_is_tensor
                              else np.ascontiguousarray(weather, dtype=np.float64))
        self.weather_rows = int(self._weather_data.shape[0])
        need = self.N + 1 + self.Np + 1
        if self.weather_rows < need:
            raise ValueError(f"weather tensor has {self.weather_rows} rows, an episode needs {need}")
        if start_rows is None:
            start_rows = [0]
        self.start_rows = np.asarray(start_rows, dtype=np.int64)
        if np.any(self.start_rows + need > self.weather_rows) or np.any(self.start_rows < 0):
            raise ValueError("start_rows + episode length exceeds the weather tensor")
        self.start_days = np.asarray(start_days if start_days is not None
                                     else self.start_rows * self.dt / self.c, dtype=np.float32)
        self.rng, self.start_grid = _check_rng(rng, start_grid, len(self.start_rows))
        self.env_index_offset = int(env_index_offset)

        dev, T = self.device, self.tdtype
        z = lambda *s, dtype=T: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        self.weather_t = (weather.to(device=dev, dtype=T).contiguous() if weather_is_tensor
                          else torch.as_tensor(self.weather_data, dtype=T, device=dev).contiguous())
        self.x_T, self.u_T = z(L.NX, self.ld), z(L.NU, self.ld)
        self.ctrl_T = z(L.NU, self.ld)
        self.info_T = z(L.NINFO, self.ld)
        self.reward_t = z(self.ld)
        self.done_t = z(self.B, dtype=torch.uint8)
        self.timestep_t = z(self.B, dtype=torch.int32)
        self.w_off_t = z(self.B, dtype=torch.int32)
        self.start_day_t = z(self.B, dtype=torch.float32)
        self.action_t = z(self.B, L.NU, dtype=torch.float32)
        self.obs_t = z(self.B, self.obs_dim, dtype=torch.float32)
        self.term_obs_t = z(self.B, self.obs_dim, dtype=torch.float32)
        self.metrics_t = z(L.METRIC_REPLICAS, L.METRIC_STRIDE, dtype=torch.float32) if collect_metrics else None
        # how each env-step's integration went (include/glgym.h GLGYM_SF_*: first-attempt flags, extra attempts, and whether the
        # result was accepted by agreement on a flagged attempt / as the finest attempt alone / not at all); infos["integration"]
        self.step_flags_t = z(self.B, dtype=torch.int32)
        self.crop_T = z(L.NCROP, self.ld) if self.uncertainty_scale > 0 else None
        self._start_rows_t = torch.as_tensor(self.start_rows, dtype=torch.int32, device=dev)
        self._start_days_t = torch.as_tensor(self.start_days, dtype=torch.float32, device=dev)
        self.episode_t = z(self.B, dtype=torch.int32)           # episodes started per env (keys the start draw)
        self._draw = 0
        # rng="numpy": the PCG64 streams, SoA uint64 [5][ld] (torch has no arithmetic on uint64: carried as int64, same bits)
        self.rng_state_t = z(np_stream.NWORD, self.ld, dtype=torch.int64) if self.rng == "numpy" else None
        if self.rng == "numpy":
            self._seed_streams(self.seed_value)
        self.x, self.u = self.x_T[:, :self.B].t(), self.u_T[:, :self.B].t()      # [B,28] / [B,6] views

        # observation space = concatenation of the modules' bounds (tomato_env.py:83-95; the reference's lower bound
        # really is -1e-4)
        lo = np.concatenate([np.full(m.n_obs, m.low, np.float32) for m in self.observation_modules])
        hi = np.concatenate([np.full(m.n_obs, m.high, np.float32) for m in self.observation_modules])
        self.observation_space = _box(lo, hi, (self.obs_dim,), np.float32)
        self.action_space = _box(-1.0, 1.0, (L.NU,), np.float32)
        self._actions = None
        self._action_src = self.action_t    # where the step kernel reads the actions (step_tensor: the caller's tensor where it can be read in place)
        self.freeze_crop_noise = False      # True: no per-step crop noise draw (a hand-set per-env block is held)
        self._keep_applied_u, self._u_applied_T, self._u_applied_valid = False, None, False
        self._hod_table_t = None
        self.reset_infos: List[dict] = [{} for _ in range(self.B)]
        # pinned host staging for the numpy (SB3) path: the 1 KB/env observation block dominates the D2H traffic
        self._obs_host = [torch.empty(self.B, self.obs_dim, dtype=torch.float32).pin_memory() for _ in range(2)]
        self._obs_flip = 0

    n_fused_steps = property(lambda self: self._fusion.n_fused_steps)        # the StepFusion's counters
    n_obs_elided = property(lambda self: self._fusion.n_obs_elided)
    n_fused_resets = property(lambda self: self._fusion.n_fused_resets)
    n_reset_elided = property(lambda self: self._fusion.n_reset_elided)

    def _obs_to_host(self, obs_t):
        """D2H into one of two pinned buffers (alternating) and return a numpy VIEW of it: the array stays valid
        until the call after next.  (A second host-side copy of the 1 KB/env block would cost more than the PCIe
        transfer itself; consumers such as SB3's rollout buffer copy what they keep.)"""
        buf = self._obs_host[self._obs_flip]
        self._obs_flip ^= 1
        buf.copy_(obs_t, non_blocking=True)
        self.torch.cuda.current_stream(self.device).synchronize()
        return buf.numpy()

    # ------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream(self.device).cuda_stream)

    # ---- rng="numpy": the reference's per-environment NumPy streams ------------------------------
    def _seed_streams(self, seed: int):
        """Environment b <- PCG64(SeedSequence(seed + env_index_offset + b)), seeded on the host (np_stream.seed_states) and uploaded."""
        first = int(seed) + self.env_index_offset
        self.set_rng_state(np_stream.seed_states(range(first, first + self.B)))

    def get_rng_state(self) -> List[dict]:
        """The streams as NumPy `bit_generator.state` dicts, one per environment (rng="numpy"): `np.random.PCG64().state = d` continues
        environment b's stream on the host; set_rng_state(get_rng_state()) of an earlier moment restores it (checkpoints)."""
        if self.rng_state_t is None:
            raise L.GlgymError("get_rng_state: this environment was built with rng='philox' (stateless, keyed by seed and counters)")
        return np_stream.unpack_states(self.rng_state_t[:, :self.B].cpu().numpy().view(np.uint64))

    def set_rng_state(self, states):
        """states: list of B PCG64 `bit_generator.state` dicts, or the packed uint64 [5, B] array of np_stream."""
        if self.rng_state_t is None:
            raise L.GlgymError("set_rng_state: this environment was built with rng='philox'")
        words = states if isinstance(states, np.ndarray) else np_stream.pack_states(states)
        if words.shape != (np_stream.NWORD, self.B):
            raise ValueError(f"set_rng_state: expected {self.B} states, got an array of shape {words.shape}")
        self.rng_state_t[:, :self.B].copy_(self.torch.as_tensor(np.ascontiguousarray(words, dtype=np.uint64).view(np.int64)))

    # ---- snapshots and planning -------------------------------------------------------------------
    _STATE_TENSORS = ("x_T", "u_T", "timestep_t", "w_off_t", "start_day_t", "episode_t", "crop_T", "rng_state_t", "obs_t", "done_t")

    def get_state(self) -> Dict[str, Any]:
        """Snapshot of everything the next step_tensor depends on: clones of the device tensors x_T, u_T, timestep_t, w_off_t,
        start_day_t, episode_t, crop_T (None at uncertainty_scale 0), rng_state_t (None with rng="philox"), obs_t, done_t, plus the
        host scalars _draw (Philox draw counter) and seed_value, and the shape / dtype / rng mode set_state checks.  The reference has no
        counterpart.  set_state(get_state()) of an earlier moment makes the environment repeat what it did from there, bit for bit."""
        state: Dict[str, Any] = {k: (None if getattr(self, k) is None else getattr(self, k).clone()) for k in self._STATE_TENSORS}
        state.update(_draw=int(self._draw), seed_value=int(self.seed_value), num_envs=self.B, dtype=str(self.tdtype), rng=self.rng)
        return state

    def set_state(self, state: Dict[str, Any]):
        """Restore a get_state() snapshot.  A snapshot of an environment of another batch size, dtype, rng mode or crop-noise setting
        raises ValueError and changes nothing."""
        missing = [k for k in self._STATE_TENSORS + ("_draw", "seed_value", "num_envs", "dtype", "rng") if k not in state]
        if missing:
            raise ValueError(f"set_state: not a get_state() snapshot (missing {missing})")
        if state["num_envs"] != self.B or state["dtype"] != str(self.tdtype) or state["rng"] != self.rng:
            raise ValueError(f"set_state: snapshot of {state['num_envs']} envs, {state['dtype']}, rng={state['rng']!r} does not fit "
                             f"this environment ({self.B} envs, {self.tdtype}, rng={self.rng!r})")
        for k in self._STATE_TENSORS:
            mine, theirs = getattr(self, k), state[k]
            if (mine is None) != (theirs is None) or (mine is not None and (mine.shape != theirs.shape or mine.dtype != theirs.dtype)):
                raise ValueError(f"set_state: {k} of the snapshot does not fit this environment")
        for k in self._STATE_TENSORS:
            if getattr(self, k) is not None:
                getattr(self, k).copy_(state[k])
        self._draw, self.seed_value = int(state["_draw"]), int(state["seed_value"])

    def planner(self, n_candidates: int, horizon: int, gamma: float = 1.0, crop: str = "nominal", **scenarios):
        """A gl_gym_amd.planner.Planner for this environment: n_candidates control sequences per environment, simulated over `horizon`
        env-steps on forked copies (buffers allocated once, here), scored and selected on the device.  crop="current" forks this
        environment's per-env crop block (uncertainty_scale > 0) and holds it over the horizon; "nominal" plans with the handle's
        parameters.  Robust planning, keyword-only: n_scenarios=S simulates every candidate under S sampled futures of the crop block
        (noise_scale, default this environment's uncertainty_scale; noise="step" | "hold") and scores it by the mean of its n_tail
        worst returns (default S: the mean); scenario_seed keys the futures.  weather_sigma (7 floats or a dict by column name) with
        weather_phi gives every scenario its own wrong weather forecast as well (planner.py).  constraints=planner.Constraints(...)
        ranks the candidates under violation budgets (feasible first, or with a penalty) instead of by return alone."""
        from .planner import Planner
        constraints = scenarios.pop("constraints", None)
        plan = Planner(self, n_candidates, horizon, gamma=gamma, crop=crop, **scenarios)
        if constraints is not None:
            plan._constrain(constraints)
        return plan

    def rule_search(self, n_candidates: int, horizon: int, tune, base=None, gamma: float = 1.0, **scenario_kwargs):
        """A gl_gym_amd.planner.RuleSearch for this environment: closed-loop rollouts of n_candidates rule-based controllers per
        environment over `horizon` env-steps on forked copies, and the tuning of the constants named in tune = {name: (lo, hi), ...}
        by the cross-entropy method; the other constants come from `base` (default RuleBasedController()).  The scenario arguments of
        planner() (n_scenarios, n_tail, noise, noise_scale, scenario_seed, weather_sigma, weather_phi) make the tuning robust to crop
        noise and forecast error; constraints=planner.Constraints(...) tunes under violation budgets.  Needs dt to be a multiple of
        450 s (planner.check_rule_dt)."""
        from .planner import RuleSearch
        return RuleSearch(self, n_candidates, horizon, tune, base=base, gamma=gamma, **scenario_kwargs)

    def policy_search(self, n_candidates: int, horizon: int, spec, share: str = "greenhouse", gamma: float = 1.0, **scenario_kwargs):
        """A gl_gym_amd.planner.PolicySearch for this environment: closed-loop rollouts of n_candidates MLP policies (spec: a
        planner.MLPSpec with in_dim = obs_dim) over `horizon` env-steps on forked copies, and gradient-free policy search by the
        cross-entropy method.  share="greenhouse": candidates per greenhouse; "all": every policy runs on all greenhouses and is scored
        by its mean return.  The scenario arguments of planner() except weather_sigma apply (evaluation and search under crop noise);
        constraints=planner.Constraints(...) searches under violation budgets (with share="all" a policy's runs are its greenhouses
        times its scenarios)."""
        from .planner import PolicySearch
        return PolicySearch(self, n_candidates, horizon, spec, share=share, gamma=gamma, **scenario_kwargs)

    def _launch_reset(self, mask_t):
        """Masked reset; the kernel draws each new episode's start from the start table (Philox on (seed, env, episode)).
        rng="numpy": glgym_rng_reset_draw takes choice(years), choice(days) from each masked environment's stream first, and
        glgym_reset, called without a start table, initialises from the w_off it wrote.
        After a step that has done its own auto-reset the call launches nothing, or runs over the environments the caller added to
        done_t only (step_fusion.StepFusion)."""
        launch, mask_t = self._fusion.reset(self, mask_t)
        if not launch:
            return
        mask_ptr = mask_t.data_ptr() if mask_t is not None else None
        if self.rng == "numpy":
            L.check(self._lib.glgym_rng_reset_draw(self._h, self.B, self.ld, mask_ptr, self.rng_state_t.data_ptr(), self.start_grid[0],
                                                   self.start_grid[1], self._start_rows_t.data_ptr(), self._start_days_t.data_ptr(),
                                                   self.w_off_t.data_ptr(), self.start_day_t.data_ptr(), self._stream()),
                    "glgym_rng_reset_draw")
            a = L.ResetArgs(self.B, self.ld, mask_ptr, self.x_T.data_ptr(), self.u_T.data_ptr(), self.timestep_t.data_ptr(),
                            self.weather_t.data_ptr(), self.weather_rows, self.w_off_t.data_ptr(), None, None, 0,
                            self.start_day_t.data_ptr(), self.episode_t.data_ptr(), self.seed_value)
            L.check(self._lib.glgym_reset(self._h, C.byref(a), self._stream()), "glgym_reset")
            return
        L.check(self._lib.glgym_reset(self._h, C.byref(self._reset_args(mask_t)), self._stream()), "glgym_reset")

    def _reset_args(self, mask_t):
        """glgym_reset's arguments with the start table (rng="philox")."""
        return L.ResetArgs(self.B, self.ld, mask_t.data_ptr() if mask_t is not None else None, self.x_T.data_ptr(),
                           self.u_T.data_ptr(), self.timestep_t.data_ptr(), self.weather_t.data_ptr(), self.weather_rows,
                           self.w_off_t.data_ptr(), self._start_rows_t.data_ptr(), self._start_days_t.data_ptr(),
                           len(self.start_rows), self.start_day_t.data_ptr(), self.episode_t.data_ptr(), self.seed_value)

    def _obs_args(self, out_t, mask_t=None, term_t=None):
        return L.ObsArgs(self.B, self.ld, self.x_T.data_ptr(), self.u_T.data_ptr(), self.weather_t.data_ptr(),
                         self.weather_rows, self.w_off_t.data_ptr(), self.timestep_t.data_ptr(),
                         self.start_day_t.data_ptr(), self.Np, out_t.data_ptr(),
                         mask_t.data_ptr() if mask_t is not None else None,
                         term_t.data_ptr() if term_t is not None else None)

    def _launch_obs(self, out_t, mask_t=None, term_t=None):
        """glgym_obs into out_t: every row (mask_t None, "full mode"), or the rows of mask_t after saving them to term_t.
        Launches nothing where the last step's own launch has written these rows already, and does not save terminal rows a second time
        (step_fusion.StepFusion)."""
        if mask_t is None:
            launches = [] if self._fusion.full_obs(self, out_t) else [(None, term_t)]
        else:
            launches = self._fusion.masked_obs(self, out_t, mask_t, term_t)
        for mask_t, term_t in launches:
            L.check(self._lib.glgym_obs(self._h, C.byref(self._obs_args(out_t, mask_t, term_t)), self._stream()), "glgym_obs")

    def _launch_step(self, raw_control: bool, want_obs: Optional[bool] = None, with_reset: Optional[bool] = None):
        """One glgym_step.  want_obs True: glgym_step_obs, which also leaves the full-mode observation of the new state in obs_t; False:
        the plain step.  with_reset True (auto_reset, rng="philox" only): glgym_step_obs_reset -- the step, the full-mode observation, the
        reset of the environments this step finished (mask done_t) and their masked observation with the terminal rows saved to
        term_obs_t.  Either is one launch where the library has a kernel with that epilogue for this configuration, and back to back
        launches elsewhere.  None (a bare call, as bench.py's loop): adaptive, by what followed the previous step.  The rules, and the
        contract on what the buffers hold after a fused auto-reset: step_fusion.StepFusion."""
        if self._env_at_create is not None and tuple(os.environ.get(k) for k in ("GLGYM_LAYOUT", "GLGYM_OCC", "GLGYM_VERIFY")) != self._env_at_create:
            import warnings
            warnings.warn("GLGYM_LAYOUT / GLGYM_OCC / GLGYM_VERIFY changed after this TomatoVecEnv was created: they are read once, at glgym_create, "
                          "and have no effect on an existing handle -- use set_layout() / set_occupancy() / set_verify()", RuntimeWarning, stacklevel=3)
            self._env_at_create = None                     # once
        fuse, with_reset = self._fusion.begin_step(want_obs, with_reset, self.auto_reset and self.rng != "numpy")
        if self.rng == "numpy":
            if not self.freeze_crop_noise:   # tomato_env.py:118: 34 draws every step, also at scale 0 (no block: streams advance)
                L.check(self._lib.glgym_rng_crop_noise(self._h, self.crop_T.data_ptr() if self.crop_T is not None else None, self.B, self.ld,
                                                       self.uncertainty_scale, self.rng_state_t.data_ptr(), self._stream()),
                        "glgym_rng_crop_noise")
        elif self.crop_T is not None and not self.freeze_crop_noise:       # noise.py: a fresh draw every step
            L.check(self._lib.glgym_crop_noise(self._h, self.crop_T.data_ptr(), self.B, self.ld,
                                               self.uncertainty_scale, self.seed_value, self._draw, self._stream()),
                    "glgym_crop_noise")
            self._draw += 1
        a = L.make_step_args(self.B, self.ld, self.x_T.data_ptr(), self.u_T.data_ptr(),
                       None if raw_control else self._action_src.data_ptr(),
                       self.ctrl_T.data_ptr() if raw_control else None, self.weather_t.data_ptr(), self.weather_rows,
                       self.w_off_t.data_ptr(), self.timestep_t.data_ptr(),
                       self.crop_T.data_ptr() if self.crop_T is not None else None, self.N,
                       self.reward_t.data_ptr(), self.info_T.data_ptr(), self.done_t.data_ptr(),
                       self.metrics_t.data_ptr() if self.metrics_t is not None else None, self.step_flags_t.data_ptr())
        if not fuse:
            L.check(self._lib.glgym_step(self._h, C.byref(a), self._stream()), "glgym_step")
            return
        if with_reset:
            one = C.c_int32(0)
            L.check(self._lib.glgym_step_obs_reset(self._h, C.byref(a), C.byref(self._obs_args(self.obs_t, None, self.term_obs_t)),
                                                   C.byref(self._reset_args(self.done_t)), self._stream(), C.byref(one)),
                    "glgym_step_obs_reset")
            self._fusion.step_launched(self, True, one.value)
            return
        L.check(self._lib.glgym_step_obs(self._h, C.byref(a), C.byref(self._obs_args(self.obs_t)), self._stream()), "glgym_step_obs")
        self._fusion.step_launched(self, False)

    # ---- tensor interface (no host synchronisation) ---------------------------------------------
    def reset_tensor(self, seed: Optional[int] = None):
        if seed is not None:
            self.seed_value = int(seed)
            self.episode_t.zero_()
            if self.rng == "numpy":
                self._seed_streams(self.seed_value)
        self._launch_reset(None)
        self._launch_obs(self.obs_t)
        return self.obs_t

    def _launch_rule_based(self, controller, hour_t=None, doy_t=None):
        """glgym_rule_based: controller.predict for every env, written to the SoA control buffer of step_raw_control."""
        cfg = L.RuleCfg(*[float(getattr(controller, n)) for n in L.RULE_FIELDS])
        if hour_t is None and (self.dt / 3600) * 8 != round((self.dt / 3600) * 8):    # increments other than multiples of 1/8 h do not sum exactly
            hour_t = self.hour_of_day()
        a = L.RuleArgs(self.B, self.ld, self.x_T.data_ptr(), self.weather_t.data_ptr(), self.weather_rows,
                       self.w_off_t.data_ptr(), self.timestep_t.data_ptr(), self.start_day_t.data_ptr(),
                       hour_t.data_ptr() if hour_t is not None else None,
                       doy_t.data_ptr() if doy_t is not None else None, self.ctrl_T.data_ptr())
        L.check(self._lib.glgym_rule_based(self._h, C.byref(cfg), C.byref(a), self._stream()), "glgym_rule_based")

    def step_tensor(self, actions_t=None, controls_t=None, want_obs: bool = True, controller=None):
        """actions_t [B,6] f32 in [-1,1] (step), controls_t [B,6] (step_raw_control) or controller (a
        RuleBasedController evaluated on the device, then step_raw_control).  Returns
        (obs [B,dim] f32, reward [B], done [B] uint8, info [11,B]) as device tensors; with auto_reset the
        finished envs are re-initialised and ``term_obs_t`` keeps their last observation."""
        if (actions_t is not None) + (controls_t is not None) + (controller is not None) != 1:
            raise ValueError("give exactly one of actions_t / controls_t / controller")
        self._action_src = self.action_t
        if actions_t is not None:
            if (actions_t.dtype == self.torch.float32 and actions_t.is_cuda and actions_t.device == self.device and
                    actions_t.is_contiguous() and actions_t.numel() == self.B * L.NU):
                self._action_src = actions_t          # read in place by the kernel (no 1.5 MB copy, no extra launch)
            else:
                self.action_t.copy_(actions_t.reshape(self.B, L.NU))
        elif controls_t is not None:
            self.ctrl_T[:, :self.B].copy_(controls_t.reshape(self.B, L.NU).t())
        else:
            self._launch_rule_based(controller)
        # one library call for step, observation, auto-reset and terminal observations (one launch where the library has the kernel)
        # unless the host infos need the applied controls copied between step and reset (step_wait)
        self._launch_step(raw_control=actions_t is None, want_obs=want_obs,
                          with_reset=want_obs and self.auto_reset and not self._keep_applied_u)
        if want_obs:
            self._launch_obs(self.obs_t)
        if self.auto_reset:      # SB3 semantics: finished envs restart; their last obs goes to term_obs_t
            if self._keep_applied_u:     # host infos report the control applied in THIS step (tomato_env.py:221), which the
                if self._u_applied_T is None:                        # reset below zeroes for the finished envs
                    self._u_applied_T = self.torch.empty_like(self.u_T)
                self._u_applied_T.copy_(self.u_T)
                self._u_applied_valid = True
            else:
                self._u_applied_valid = False        # a later host_infos() must not report an EARLIER step's controls
            self._launch_reset(self.done_t)
            if want_obs:
                self._launch_obs(self.obs_t, self.done_t, self.term_obs_t)
        self._fusion.own_calls()         # these were step_tensor's own calls: they arm no bare _launch_step
        return self.obs_t, self.reward_t[:self.B], self.done_t, self.info_T[:, :self.B]

    # ---- SB3 VecEnv calling convention ------------------------------------------------------------
    def reset(self):
        return self._obs_to_host(self.reset_tensor())

    def seed(self, seed: Optional[int] = None):
        if seed is not None:
            self.seed_value = int(seed)
            if self.rng == "numpy":
                self._seed_streams(self.seed_value)
        return [seed] * self.B

    def step_async(self, actions):
        self._actions = np.asarray(actions, dtype=np.float32)

    def step_wait(self):
        self._keep_applied_u = True
        try:
            return self._host_result(self.step_tensor(self.torch.as_tensor(self._actions, device=self.device)))
        finally:
            self._keep_applied_u = False

    def _host_result(self, out):
        """(obs, rewards, dones, infos) as SB3 consumes them, from step_tensor's device tensors."""
        obs_t, r_t, d_t, info_T = out
        obs, rew = self._obs_to_host(obs_t), r_t.float().cpu().numpy()
        dones, infos = self.host_infos(d_t, info_T)
        return obs, rew, dones, infos

    def host_infos(self, d_t, info_T, term_obs=None):
        """(dones [B] bool, infos) on the host.  term_obs: replacement for the raw terminal observations (a wrapper
        that rescales observations passes its own)."""
        dones = d_t.cpu().numpy().astype(bool)
        # infos: SB3 wants a list of per-env dicts.  Built from two bulk D2H copies (info block, controls) with
        # zip over Python lists -- the cheapest pure-Python construction (about 1 us per env per key).
        rows = info_T.double().t().cpu().numpy()
        applied = self._u_applied_T if (self.auto_reset and self._u_applied_valid) else self.u_T
        ctrl = applied[:, :self.B].t().double().cpu().numpy()
        term = None
        if self.auto_reset and dones.any():
            term = self.term_obs_t.cpu().numpy() if term_obs is None else term_obs
        flags = self.step_flags_t.cpu().numpy() if self.integration_info else None
        if self.lazy_infos:
            infos = LazyInfos(L.INFO_KEYS, rows, ctrl, dones, term, flags)
        else:
            infos = [dict(zip(L.INFO_KEYS, row), controls=c) for row, c in zip(rows.tolist(), ctrl)]
            for d in infos:
                d["TimeLimit.truncated"] = False
            if flags is not None:
                for d, f in zip(infos, flags.tolist()):
                    d["integration"] = f      # GLGYM_SF_* word: 0 = first attempt accepted as it stood
            if term is not None:
                for b in np.nonzero(dones)[0]:
                    infos[b]["terminal_observation"] = term[b]
        return dones, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def step_raw_control(self, controls):
        torch = self.torch
        obs_t, r_t, d_t, info_T = self.step_tensor(controls_t=torch.as_tensor(np.asarray(controls), dtype=self.tdtype,
                                                                              device=self.device))
        return self._obs_to_host(obs_t), r_t.float().cpu().numpy(), d_t.cpu().numpy().astype(bool), info_T.cpu().numpy()

    def step_raw_control_pipeinput(self, controls):
        """tomato_env.py:175-191: controls applied directly, no noise / observation / info; returns (x [B,28], terminated [B])."""
        torch = self.torch
        _, _, d_t, _ = self.step_tensor(controls_t=torch.as_tensor(np.asarray(controls), dtype=self.tdtype,
                                                                   device=self.device), want_obs=False)
        return self.x.double().cpu().numpy(), d_t.cpu().numpy().astype(bool)

    def _indices(self, indices):
        if indices is None:
            return list(range(self.B))
        return [indices] if isinstance(indices, int) else list(indices)

    def get_attr(self, attr_name: str, indices=None):
        idx = self._indices(indices)
        per_env = {"x": lambda b: self.x[b].double().cpu().numpy(), "u": lambda b: self.u[b].double().cpu().numpy(),
                   "timestep": lambda b: int(self.timestep_t[b]), "start_day": lambda b: float(self.start_day_t[b]),
                   "w_off": lambda b: int(self.w_off_t[b])}
        if attr_name == "growth_year" and getattr(self, "start_years", None) is not None:
            # the (year, day) pair an env drew at its last reset = the entry of the start table its w_off points at
            w_off = self.w_off_t.cpu().numpy()
            return [int(self.start_years[int(np.searchsorted(self.start_rows, w_off[b], side="right")) - 1]) for b in idx]
        if attr_name in per_env:
            return [per_env[attr_name](b) for b in idx]
        return [getattr(self, attr_name) for _ in idx]

    def set_attr(self, attr_name: str, value, indices=None):
        setattr(self, attr_name, value)

    def env_method(self, method_name: str, *args, indices=None, **kwargs):
        return [getattr(self, method_name)(*args, **kwargs) for _ in self._indices(indices)]

    def env_is_wrapped(self, wrapper_class, indices=None):
        return [False for _ in self._indices(indices)]

    def get_obs_names(self):
        return [n for m in self.observation_modules for n in m.obs_names]

    def set_seed(self, seed: int):
        """base_env.py:166-170 (called through env_method in experiments/evaluate_rl.py:113): re-seed the generator
        that draws the episode starts."""
        self.seed_value = int(seed)
        self.episode_t.zero_()
        if self.rng == "numpy":
            self._seed_streams(self.seed_value)

    # ---- clocks and the weather row of the coming step, as device tensors (for controllers) ---------
    def current_weather(self):
        """[B,10] rows weather[w_off + timestep] -- what the reference passes to RuleBasedController.predict."""
        idx = (self.w_off_t + self.timestep_t).long().clamp_(0, self.weather_rows - 1)
        return self.weather_t[idx]

    @property
    def weather_data(self):
        """The resident weather table [rows, nd] (float64 copy on the host).  ASSIGNING to it is the reference's `env.weather_data = table` on a
        constructed env (experiments/run_time.py:39, gl_predefined_controls.py:114): the reference's step reads `weather_data[timestep]`, so the new
        table is indexed from its row 0 by every environment, running episodes included (their `timestep` is kept), and later resets start at row
        0 / the first start day.  The column count is fixed at construction (`nd`: 10, or 14 for the measured-pipe variant); a step graph captured before
        the assignment holds the old table's address and has to be captured again."""
        return self._weather_data

    @weather_data.setter
    def weather_data(self, table):
        torch = self.torch
        table = np.ascontiguousarray(table.detach().double().cpu().numpy() if hasattr(table, "detach") else table, dtype=np.float64)
        if table.ndim != 2 or table.shape[1] != self._weather_data.shape[1]:
            raise ValueError(f"weather_data: expected [rows, {self._weather_data.shape[1]}] like the table this env was built with, got {table.shape}")
        need = self.N + 1 + self.Np + 1
        if table.shape[0] < need:
            raise ValueError(f"weather_data has {table.shape[0]} rows, an episode needs {need}")
        self._weather_data = table
        self.weather_rows = int(table.shape[0])
        self._fusion.advance()              # another table, another row count: a fused observation of the old one is void
        self.weather_t = torch.as_tensor(table, dtype=self.tdtype, device=self.device).contiguous()
        self.start_rows = np.zeros(1, dtype=np.int64)
        self.start_days = np.asarray(self.start_days[:1], dtype=np.float32)
        self._start_rows_t = torch.as_tensor(self.start_rows, dtype=torch.int32, device=self.device)
        self._start_days_t = torch.as_tensor(self.start_days, dtype=torch.float32, device=self.device)
        if self.rng == "numpy":
            self.start_grid = (1, 1)        # one start left: choice() of one-element lists draws nothing
        self.w_off_t.zero_()

    @property
    def p(self):
        """The shared parameter block (float32, tomato_env.py:62).  ASSIGNING to it is the reference's `env.p = new_p` on a constructed env
        (experiments/run_time.py:40-41: `env.p = set_matlab_params(env.p)`): the device model, the crop block and the reward's per-step cost
        coefficients follow the new block; the reward's scale max_profit / min_profit stays what it was at construction, as in the reference
        (rewards.py:82-83 computes it once in __init__) -- glgym_set_params_keep_reward_scale.  Construct with `params=` to have both from one block."""
        return self._p

    @p.setter
    def p(self, value):
        value = np.asarray(value, dtype=np.float32)
        if value.shape != (L.NP,):
            raise ValueError(f"p: expected {L.NP} parameters, got an array of shape {value.shape}")
        p64 = np.ascontiguousarray(value, dtype=np.float64)
        L.check(self._lib.glgym_set_params_keep_reward_scale(self._h, p64.ctypes.data_as(L._DP)), "glgym_set_params_keep_reward_scale")
        self._p = value

    def _hod_table(self):
        """The reference ACCUMULATES its clock, hour_of_day = (hour_of_day + dt / 3600) % 24 once per step (tomato_env.py:127-128).  With
        dt = 900 s the increment 0.25 is exact and the sum equals timestep * dt / 3600; with dt = 300 s (experiments/run_time.py) the sum
        drifts by ulps and reads 17.999999999999996 where the product reads 18.0 -- and the rule-based controller compares the clock with
        whole hours (baseline.py:76-77, 107, 113): 13 of 960 steps of the dt = 300 hold-out switch the lamps one step apart.  The table
        holds the reference's sum for every timestep of an episode; timestep indexes it."""
        if self._hod_table_t is None:
            t = np.empty(self.N + 4, dtype=np.float64)
            h = 0.0
            for k in range(len(t)):
                t[k] = h
                h = (h + self.dt / 3600) % 24
            self._hod_table_t = self.torch.as_tensor(t, device=self.device)
        return self._hod_table_t

    def hour_of_day(self):
        return self._hod_table()[self.timestep_t.long().clamp_(0, self.N + 3)]      # tomato_env.py:127-128, accumulated like the reference's

    def day_of_year(self):
        return self.start_day_t.double() + self.timestep_t.double() * ((self.dt / self.c) % 365)   # :126

    def rule_based_controls(self, controller):
        """u[B,6] of a gl_gym_amd.baseline.RuleBasedController for the current state (experiments/evaluate_baseline.py:22),
        computed by the glgym_rule_based kernel."""
        self._launch_rule_based(controller)
        return self.ctrl_T[:, :self.B].t().clone()

    def step_rule_based(self, controller):
        """One env-step under the rule-based controller, everything on the device (config 1, batched)."""
        return self._host_result(self.step_tensor(controller=controller))

    def metrics(self) -> Dict[str, float]:
        if self.metrics_t is None:
            return {}
        v = self.metrics_t.double().sum(dim=0)[:L.NMETRIC].cpu().numpy()      # sum of the replicas
        return {k: float(v[i]) for i, k in enumerate(L.METRIC_KEYS)}

    def capture_step_graph(self, want_obs: bool = True):
        """Capture one full step (action copy -> glgym_step_obs_reset, one node where the library has the kernel with both epilogues; without want_obs:
        action copy -> glgym_step -> masked glgym_reset) in a HIP graph, a single chain of nodes.  The library's device-pointer entry
        points never synchronise, so they can be stream-captured; one graph launch then replaces the kernel launches of a step
        (about 2 % at B = 65 536, more when B is small).  Returns
        ``replay(actions_t) -> (obs, reward, done, info)`` with the same device tensors ``step_tensor`` returns.
        Per-env crop noise (uncertainty_scale > 0) of rng="philox" advances a host-side draw counter per step and is not capturable;
        with rng="numpy" the streams live on the device and the noise and start-draw launches are captured with the rest."""
        if self.crop_T is not None and self.rng != "numpy":
            raise L.GlgymError("capture_step_graph: per-step crop noise carries a host-side draw counter; use step_tensor")
        torch = self.torch
        static_a = torch.zeros(self.B, L.NU, dtype=torch.float32, device=self.device)

        def seq():
            self.action_t.copy_(static_a)
            self._action_src = self.action_t
            self._launch_step(raw_control=False, want_obs=want_obs, with_reset=want_obs and self.auto_reset)
            if want_obs:
                self._launch_obs(self.obs_t)
            if self.auto_reset:
                self._launch_reset(self.done_t)
                if want_obs:
                    self._launch_obs(self.obs_t, self.done_t, self.term_obs_t)
            self._fusion.own_calls()        # the captured sequence's own calls: they arm no bare _launch_step

        # warm-up on a side stream (torch's capture protocol), with the state restored afterwards
        state = [self.x_T, self.u_T, self.timestep_t, self.w_off_t, self.start_day_t, self.episode_t, self.obs_t]
        if self.rng == "numpy":             # the warm-up draws from the streams: they go back to where they were
            state += [self.rng_state_t] + ([self.crop_T] if self.crop_T is not None else [])
        keep = [b.clone() for b in state]
        metrics = None if self.metrics_t is None else self.metrics_t.clone()
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            seq()
        torch.cuda.current_stream(self.device).wait_stream(side)
        for b, k in zip(state, keep):
            b.copy_(k)
        if metrics is not None:
            self.metrics_t.copy_(metrics)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            seq()
        for b, k in zip(state, keep):
            b.copy_(k)                      # capture does not execute, but keep the contract explicit
        if metrics is not None:
            self.metrics_t.copy_(metrics)

        def replay(actions_t):
            static_a.copy_(actions_t.reshape(self.B, L.NU))
            graph.replay()
            return self.obs_t, self.reward_t[:self.B], self.done_t, self.info_T[:, :self.B]
        replay.graph = graph
        return replay

    def set_scheme(self, scheme: str, n_sub: Optional[int] = None, window: Optional[int] = None):
        """Switch the sub-stepper ("ls5" | "rk4" | "rk3" | "rk2", include/glgym.h), its sub-step count and tier-2b window (default: what
        this env's preset gives for the scheme; with an explicit n_sub the scheme's own window)."""
        if scheme not in L.SCHEMES:
            raise ValueError("scheme must be 'ls5', 'rk4', 'rk3' or 'rk2'")
        L.check(self._lib.glgym_set_scheme(self._h, L.SCHEMES[scheme]), "glgym_set_scheme")
        self.scheme = scheme
        n_def, w_def = L.preset_n_sub(scheme, self.dt, self.preset)
        self.set_n_sub(n_def if n_sub is None else n_sub)
        self.set_window((w_def if n_sub is None else 0) if window is None else window)

    def set_integrator(self, name: str, rtol: Optional[float] = None, atol: Optional[float] = None,
                       max_steps: Optional[int] = None):
        """Integrator of the env-steps: "explicit" (the stored scheme / n_sub / window / preset) or "bdf" (adaptive, error-controlled
        variable-order BDF in fp64, include/glgym.h glgym_set_step_integrator).  Tolerances not given keep their current values."""
        rtol = self.rtol if rtol is None else rtol
        atol = self.atol if atol is None else atol
        max_steps = self.max_steps if max_steps is None else max_steps
        _check_integrator(name, self.model_variant)
        _check_tolerances(rtol, atol, max_steps)
        L.check(self._lib.glgym_set_tolerances(self._h, float(rtol), float(atol), int(max_steps)), "glgym_set_tolerances")
        L.check(self._lib.glgym_set_step_integrator(self._h, L.INTEGRATORS[name]), "glgym_set_step_integrator")
        self.integrator, self.rtol, self.atol, self.max_steps = name, float(rtol), float(atol), int(max_steps)

    def solver_metrics(self) -> Dict[str, float]:
        """Totals of the BDF env-steps since the metrics were last zeroed (metric slots GLGYM_METRIC_BDF..+3): steps, right-hand-side
        evaluations, Jacobians, LU factorisations.  The per-env step count of the last step is in bits 16..30 of step_flags_t."""
        if self.metrics_t is None:
            return {}
        v = self.metrics_t.double().sum(dim=0)[L.METRIC_BDF:L.METRIC_BDF + len(L.BDF_METRIC_KEYS)].cpu().numpy()
        return {k: float(v[i]) for i, k in enumerate(L.BDF_METRIC_KEYS)}

    def set_window(self, window: int):
        """Nominal sub-steps per tier-2b / harvest window (glgym_set_window): 0 = the scheme's own."""
        self.window = int(window)
        L.check(self._lib.glgym_set_window(self._h, self.window), "glgym_set_window")

    def set_layout(self, layout: str):
        """Kernel layout of float32 steps (glgym_set_layout): "auto" | "one" (lane per environment) | "quad" (four lanes)."""
        L.check(self._lib.glgym_set_layout(self._h, L.LAYOUTS[layout]), "glgym_set_layout")

    def set_occupancy(self, waves_per_simd: int):
        """0 (default): the one-lane fp32 kernel's two-waves-per-SIMD build from 131 072 environments, the one-wave build below; 1 / 2 force a build
        (include/glgym.h glgym_set_occupancy)."""
        L.check(self._lib.glgym_set_occupancy(self._h, int(waves_per_simd)), "glgym_set_occupancy")

    def set_ladder_parallel(self, on: bool):
        """Verified steps (raw controls) on up to 8 192 environments run the step-doubling ladder two rungs at a time (default; identical
        results and step_flags, two thirds of the latency: include/glgym.h glgym_set_ladder_parallel).  False: always the sequential ladder."""
        L.check(self._lib.glgym_set_ladder_parallel(self._h, int(bool(on))), "glgym_set_ladder_parallel")

    def set_n_sub(self, n_sub: int):
        self.n_sub = int(n_sub)
        L.check(self._lib.glgym_set_n_sub(self._h, self.n_sub), "glgym_set_n_sub")

    def set_verify(self, mode: str):
        """Step-doubling verified integration (include/glgym.h, glgym_verify): "auto" (default) verifies wherever the control
        can jump -- step_raw_control / controller= steps, or delta_u_max > 0.1 -- "always" / "never" every / no env-step."""
        L.check(self._lib.glgym_set_verify(self._h, L.VERIFY_MODES[mode]), "glgym_set_verify")

    def timer_start(self):
        L.check(self._lib.glgym_timer_start(self._h, self._stream()))

    def timer_stop(self) -> float:
        ms = C.c_float()
        L.check(self._lib.glgym_timer_stop(self._h, self._stream(), C.byref(ms)))
        return float(ms.value)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self.torch.cuda.synchronize(self.device)
            self._lib.glgym_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TomatoEnv:
    """Single-environment Gymnasium-style view over a B = 1 ``TomatoVecEnv`` (no auto-reset)."""

    def __init__(self, weather=None, params=None, dt=900.0, season_length=60, pred_horizon=0.5, dtype="float64",
                 n_sub=None, device="cuda:0", uncertainty_scale=0.0, start_day=0.0, growth_year=2010,
                 reward_params=None, constraints=None, location="synthetic", training=True, model_variant="ode",
                 scheme="rk4", observation_modules=None, u_min=None, u_max=None, delta_u_max=0.1, integrator="explicit", rtol=1e-6,
                 atol=1e-6, max_steps=10000, rng="philox"):
        """integrator / rtol / atol / max_steps: as TomatoVecEnv ("bdf": error-controlled BDF env-steps).
        rng: "numpy" = the reference env's own generator: reset(seed=s) seeds Generator(PCG64(SeedSequence(s))), every step draws
        its 34 uniforms from it (also at uncertainty_scale 0), reset() without a seed continues the stream."""
        self.vec = TomatoVecEnv(1, rng=rng, model_variant=model_variant, scheme=scheme, observation_modules=observation_modules,
                                u_min=u_min, u_max=u_max, delta_u_max=delta_u_max, integrator=integrator, rtol=rtol, atol=atol,
                                max_steps=max_steps,
                                weather=weather, params=params, dt=dt, season_length=season_length,
                                pred_horizon=pred_horizon, dtype=dtype, n_sub=n_sub, device=device,
                                uncertainty_scale=uncertainty_scale, start_rows=[0], start_days=[start_day],
                                reward_params=reward_params, constraints=constraints, auto_reset=False)
        v = self.vec
        self.nx, self.nu, self.nd, self.num_params, self.dt, self.c = v.nx, v.nu, v.nd, v.num_params, v.dt, v.c
        self.N, self.Np = v.N, v.Np
        self.observation_space, self.action_space = v.observation_space, v.action_space
        self.start_day, self.growth_year, self.location, self.training = start_day, growth_year, location, training
        self.u_min, self.u_max, self.delta_u_max = v.u_min, v.u_max, v.delta_u_max
        self.terminated = False

    def _set_x(self, value):          # `env.x = init_mat_state(...)` (gl_predefined_controls.py:116)
        value = np.asarray(value, dtype=np.float64).reshape(L.NX)
        self.vec.x_T[:, 0] = self.vec.torch.as_tensor(value, dtype=self.vec.tdtype, device=self.vec.device)

    x = property(lambda self: self.vec.x[0].double().cpu().numpy(), _set_x)
    weather_data = property(lambda self: self.vec.weather_data, lambda self, table: setattr(self.vec, "weather_data", table))   # run_time.py:39
    u = property(lambda self: self.vec.u[0].double().cpu().numpy())
    p = property(lambda self: self.vec.p, lambda self, value: setattr(self.vec, "p", value))     # `env.p = set_matlab_params(env.p)` (run_time.py:40)
    timestep = property(lambda self: int(self.vec.timestep_t[0]))
    day_of_year = property(lambda self: self.start_day + self.timestep * ((self.dt / self.c) % 365))
    hour_of_day = property(lambda self: float(self.vec.hour_of_day()[0]))

    def reset(self, seed: Optional[int] = None):
        obs = self.vec.reset_tensor(seed)
        self.terminated = False
        return obs[0].double().cpu().numpy(), {}

    def action_to_control(self, action):
        return np.clip(self.u + np.asarray(action) * self.delta_u_max, self.u_min, self.u_max)

    def _finish(self, out):
        obs_t, r_t, d_t, info_T = out
        info = {k: float(info_T[i, 0]) for i, k in enumerate(L.INFO_KEYS)}
        info["controls"] = self.u
        self.terminated = bool(d_t[0])
        return obs_t[0].double().cpu().numpy(), float(r_t[0]), self.terminated, False, info

    def step(self, action):
        t = self.vec.torch
        return self._finish(self.vec.step_tensor(t.as_tensor(np.asarray(action, dtype=np.float32).reshape(1, 6),
                                                             device=self.vec.device)))

    def step_raw_control(self, control):
        t = self.vec.torch
        return self._finish(self.vec.step_tensor(controls_t=t.as_tensor(np.asarray(control).reshape(1, 6),
                                                                        dtype=self.vec.tdtype, device=self.vec.device)))

    def step_raw_control_pipeinput(self, control):
        x, term = self.vec.step_raw_control_pipeinput(np.asarray(control).reshape(1, 6))
        self.terminated = bool(term[0])
        return x[0], self.terminated

    def set_crop_state(self, cBuf, cLeaf, cStem, cFruit, tCanSum):
        for i, v in zip((22, 23, 24, 25, 26), (cBuf, cLeaf, cStem, cFruit, tCanSum)):
            self.vec.x_T[i, 0] = v

    def get_state(self):
        """TomatoVecEnv.get_state of the wrapped environment, plus this view's `terminated`."""
        return dict(self.vec.get_state(), terminated=self.terminated)

    def set_state(self, state):
        self.vec.set_state(state)
        self.terminated = bool(state.get("terminated", False))

    def get_obs_names(self):
        return self.vec.get_obs_names()

    def close(self):
        self.vec.close()
