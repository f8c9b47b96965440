"""Sampling-based planning on the device (include/glgym.h glgym_plan_*): from the current state of each of an environment's B
greenhouses, simulate K candidate control sequences over H env-steps on forked copies, score them by their discounted return, and
pick the best per greenhouse (random shooting) or the exponentially weighted mean sequence (MPPI).  The reference has no counterpart;
its README lists MPC as a next step.

What the planner sees.  By default the children step on the true future rows of the environment's weather table -- the rows the
observation's forecast module exposes -- clamped at the end of the table: perfect foresight of the weather.  With weather_sigma (below)
every scenario steps on its own, wrong forecast instead.  Without n_scenarios no noise is drawn inside the horizon: with crop="current"
the parent's present crop block is held over the horizon, with "nominal" the handle's parameters are used.  No reset happens either: a
child that reaches its season end stops accumulating (`alive`), the step that reports `done` being its last.

Robust planning (n_scenarios = S, glgym_plan_scenario / _rollout_scenarios / _aggregate): every candidate is simulated under S sampled
futures of the 34 crop parameters -- the environment's own uncertainty_scale process, redrawn at every step (noise="step") or drawn
once and held (noise="hold") -- and scored by the mean of its n_tail worst returns (n_tail = S: the mean; 1: the worst case).
Scenario s of greenhouse b is the same future for all K candidates (common random numbers), and the scenarios stay the same from
rollout to rollout until new_scenarios(): candidates, and the iterations of one cem(), are compared like with like.  select, elites,
refit, sample, cem and shift work on the aggregated [B, K] scores as they do on plain returns.

Weather-forecast uncertainty (n_scenarios = S with weather_sigma, glgym_plan_weather): scenario s of greenhouse b gets a private window
of H weather rows, the parent's coming rows with a forecast error on the seven columns the model reads -- zero at the row being
integrated now, lag-1 correlated along the horizon (weather_phi), saturating at weather_sigma: additive [K] on tOut, tSky and tSoOut,
relative and floored at 0 on iGlob, vpOut, co2Out and wind.  The futures are keyed like the crop scenarios' (scenario_seed, the same
draw index: new_scenarios() and scenario_base_t move both) and shared by the K candidates.  noise_scale=0.0 gives weather-only
scenarios: the prologue of every step then writes the nominal crop block, and the steps still run the per-env-crop build.  S = 1 is
certainty-equivalent MPC on one wrong forecast.  The environment's own table is only read; dli and the day flags are not re-derived
from the perturbed radiation, and vapour pressure, not relative humidity, is what stays put when tOut moves.

The parent environment is only read: its state, random streams, draw counter, episode counters, metrics() and step_flags_t are after
a rollout what they were before.

Iterated sampling (the cross-entropy method, glgym_plan_sample / _elites / _refit; _CemStages below): cem() draws the candidates on the device from a
Gaussian per (horizon step, greenhouse, actuator), simulates them, ranks each greenhouse's returns, refits mean and spread to the best
n_elite, and repeats; sample(), elites() and refit() are the single stages, shift() the receding-horizon warm start.

Closed-loop candidates (RuleSearch below, glgym_rule_rows / glgym_plan_rollout_rule): every candidate above is an open-loop sequence.
RuleSearch rolls out a feedback law instead -- the rule-based controller with per-candidate constants, evaluated on each child's own
state before every step -- and tunes those constants with the same cross-entropy stages.  PolicySearch (glgym_policy_rows /
glgym_plan_rollout_policy) does the same with a learned feedback law: an MLP from the child's observation row to the six actions
(MLPSpec), with per-candidate weights -- scenario evaluation of a trained policy, and CEM over the weights of small nets.

Evolution strategy (glgym_plan_es_sample / _es_utilities / _es_update; _EsStages below): both searches also offer es() -- candidates in
mirrored pairs around the mean, centred ranks over the whole population, a search-gradient step on the mean (Adam or SGD) and the
separable-NES update of the per-parameter spread -- with sample_mirrored(), utilities() and es_update() as the single stages.  The CEM
refits an independent Gaussian to the best few of K, which suits a handful of set-points; the ES uses every return and suits the
hundreds of weights of a net.

CMA-ES (glgym_plan_cma_sample / _cma_update; _CmaStages below): RuleSearch.cma() keeps a full covariance matrix per greenhouse over its
at most 32 tuned constants -- the separable searches above cannot follow constants that interact -- with sample_cma() and cma_update()
as the single stages.  PolicySearch and Planner have none: even a linear policy has 144 parameters.

Violation budgets (Constraints below, glgym_plan_constrain; _ConstrainStage): all of the above rank on the return alone.  With
constraints=Constraints(...) one more scoring stage runs behind every rollout -- after the scenario aggregate, on the per-run CO2,
temperature and humidity violation sums -- and select, elites, utilities and the CMA update rank ITS scores: feasible candidates (at
most n_allow runs over budget) by return, then infeasible ones by ascending excess, or return - rho * excess.  The tensors a rollout
returns stay the raw ones; feasible, excess, n_violating and n_feasible are new views on the planner or search.

How the code is shared.  One stage object per algorithm holds its library calls, argument checks and loop: _CemStages (Planner and both
searches; it also owns the two population blocks every sampler writes into), _EsStages, _CmaStages.  _ThetaSearch is the base of
RuleSearch and PolicySearch: the Planner they roll out on, theta in place or staged, the distribution, select, the start of a search
(_start) and the CEM / ES methods; a subclass adds its argument checks, its rollout call and its defaults.  The three rollouts build
their arguments with Planner._rollout_args and Planner._scenario_args."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import Any, Dict, Optional

import numpy as np

from . import _lib as L


def _weather_sigma(weather_sigma, weather_phi):
    """weather_sigma as the seven floats of include/glgym.h glgym_plan_weather_args.sigma; ValueError on anything else."""
    if isinstance(weather_sigma, dict):
        unknown = sorted(set(weather_sigma) - set(L.WEATHER_COLUMNS))
        if unknown:
            raise ValueError(f"weather_sigma: unknown columns {unknown}; the keys are {L.WEATHER_COLUMNS}")
        weather_sigma = [weather_sigma.get(k, 0.0) for k in L.WEATHER_COLUMNS]
    try:
        sigma = [float(v) for v in weather_sigma]
    except TypeError:
        raise ValueError("weather_sigma must be a sequence of 7 floats or a dict keyed by column name") from None
    if len(sigma) != len(L.WEATHER_COLUMNS) or not all(0.0 <= v < float("inf") for v in sigma):
        raise ValueError(f"weather_sigma must hold 7 finite values >= 0, in the order {L.WEATHER_COLUMNS}")
    if not 0.0 <= float(weather_phi) < 1.0:
        raise ValueError("weather_phi must be in [0, 1)")
    return sigma


def _select_temperature(temperature) -> float:
    """The MPPI temperature as glgym_plan_select takes it: > 0 with a finite reciprocal (the kernel multiplies by 1 / temperature; at
    2^-1024 and below that is +inf, and the best candidate's own 0 * inf a NaN); ValueError on anything else."""
    t = float(temperature)
    if not t > 0.0:
        raise ValueError("temperature must be > 0")
    if 1.0 / t == float("inf"):
        raise ValueError("temperature must have a finite reciprocal (above 2^-1024, about 5.6e-309): 1 / temperature overflows")
    return t


class Constraints:
    """Violation budgets on a rollout's accumulated CO2, temperature and humidity violations, and how the candidates are ranked
    under them (include/glgym.h glgym_plan_constrain).  co2 / temp / rh: the budget of each violation sum, >= 0, or inf for none;
    per="step": on the sum divided by the steps the run accumulated ("at most x over the line on average"), per="total": on the sum
    itself.  A run violates when its weighted excess over the budgets, sum_i weights[i] * max(0, measure_i - budget_i), is positive; a
    candidate is feasible when at most n_allow of its runs do (its scenarios, and with PolicySearch(share="all") its greenhouses):
    n_allow = 0 is a hard budget on every sampled future, n_allow = floor(eps * runs) a chance constraint.
    mode="feasible_first": every feasible candidate outranks every infeasible one; feasible ones are ordered by return, infeasible
    ones by ascending mean excess (the constrained cross-entropy ordering).  The score of an infeasible candidate is (the smallest
    feasible return of its greenhouse, or 0 without one) - 1 - excess: at least 1 below every feasible score, which is all an MPPI mean
    (select(temperature=...)) sees of the order.  mode="penalty": score = return - rho * excess.
    Hand it to env.planner / env.rule_search / env.policy_search as constraints=..., or attach() it to a Planner built directly."""

    def __init__(self, co2: float = float("inf"), temp: float = float("inf"), rh: float = float("inf"), per: str = "step",
                 weights=(1.0, 1.0, 1.0), n_allow: int = 0, mode: str = "feasible_first", rho: float = 0.0):
        inf = float("inf")
        try:
            self.budgets = tuple(float(v) for v in (co2, temp, rh))
        except (TypeError, ValueError):
            raise ValueError("co2, temp and rh must be numbers: budgets >= 0, or inf for no budget") from None
        if not all(v >= 0.0 for v in self.budgets):
            raise ValueError("co2, temp and rh must be >= 0, or inf for no budget (not NaN)")
        if per not in ("step", "total"):
            raise ValueError("per must be 'step' or 'total'")
        try:
            self.weights = tuple(float(v) for v in weights)
        except (TypeError, ValueError):
            raise ValueError("weights must be three numbers (co2, temp, rh)") from None
        if len(self.weights) != 3 or not all(0.0 <= v < inf for v in self.weights):
            raise ValueError("weights must be three finite numbers >= 0 (co2, temp, rh)")
        if isinstance(n_allow, bool) or int(n_allow) != n_allow or int(n_allow) < 0:
            raise ValueError("n_allow must be an integer >= 0")
        if mode not in L.CONSTRAIN_MODES:
            raise ValueError(f"mode must be one of {sorted(L.CONSTRAIN_MODES)}")
        if not 0.0 <= float(rho) < inf:
            raise ValueError("rho must be finite and >= 0")
        self.per, self.n_allow, self.mode, self.rho = per, int(n_allow), mode, float(rho)

    def attach(self, planner: "Planner") -> "Planner":
        """Rank the candidates of `planner` (a Planner without constraints yet) under these constraints from its next rollout on;
        returns it.  ValueError if n_allow exceeds the planner's runs per candidate."""
        planner._constrain(self)
        return planner


class _ConstrainStage:
    """glgym_plan_constrain behind a rollout, in one place for Planner (P = B groups, O = 1) and PolicySearch(share="all") (P = 1,
    O = B): the buffers, allocated once here -- score_con_t f64, failed_con_t / feasible_t u8, excess_t f64, n_viol_t i32 [P*K],
    n_feasible_t i32 and best_feasible_t u8 [P] -- the argument block over them and over the owner's returns (ret_t / failed_t [P*K]),
    per-run violations (viol_T [3, ld]) and step counts, and the two calls: run() after every rollout, best() after every select."""

    def __init__(self, env, constraints, P, O, K, S, ld, ret_t, failed_t, viol_T, n_steps_t):
        if not isinstance(constraints, Constraints):
            raise TypeError("constraints must be a planner.Constraints")
        c, torch, dev = constraints, env.torch, env.device
        if c.n_allow > O * S:
            raise ValueError(f"n_allow = {c.n_allow} exceeds the {O * S} runs of a candidate")
        self.env, self.torch, self.constraints, self.P, self.K = env, torch, c, int(P), int(K)
        J = self.P * self.K
        z = lambda n, dtype: torch.zeros(n, dtype=dtype, device=dev)  # noqa: E731
        self.score_con_t, self.excess_t = z(J, torch.float64), z(J, torch.float64)
        self.failed_con_t, self.feasible_t = z(J, torch.uint8), z(J, torch.uint8)
        self.n_viol_t, self.n_feasible_t = z(J, torch.int32), z(self.P, torch.int32)
        self.best_feasible_t = z(self.P, torch.uint8)
        self._idx_t, self._none_t = z(self.P, torch.int64), z(self.P, torch.bool)
        self._inputs = (ret_t, failed_t, viol_T, n_steps_t)          # kept alive with the pointers below
        self._args = L.make_plan_args(L.PlanConstrainArgs, self.P, int(O), self.K, int(S), int(ld), 1 if c.per == "step" else 0, c.n_allow,
                                      L.CONSTRAIN_MODES[c.mode], (C.c_double * 3)(*c.budgets), (C.c_double * 3)(*c.weights), c.rho,
                                      ret_t.data_ptr(), failed_t.data_ptr(), viol_T.data_ptr(), n_steps_t.data_ptr(),
                                      self.score_con_t.data_ptr(), self.failed_con_t.data_ptr(), self.feasible_t.data_ptr(),
                                      self.excess_t.data_ptr(), self.n_viol_t.data_ptr(), self.n_feasible_t.data_ptr())

    def views(self, rows):
        """(feasible, excess, n_violating) as [rows, K] views, and n_feasible [P]."""
        return (self.feasible_t.view(rows, self.K), self.excess_t.view(rows, self.K), self.n_viol_t.view(rows, self.K), self.n_feasible_t)

    def run(self):
        e = self.env
        L.check(e._lib.glgym_plan_constrain(e._h, C.byref(self._args), e._stream()), "glgym_plan_constrain")

    def best(self, best_k_t, out):
        """best_feasible [P] u8 = feasible[p, best_k[p]], 0 where best_k = -1, and n_feasible into the dict `out`; no allocation."""
        torch = self.torch
        self._idx_t.copy_(best_k_t)
        torch.lt(self._idx_t, 0, out=self._none_t)
        self._idx_t.clamp_(min=0)
        torch.gather(self.feasible_t.view(self.P, self.K), 1, self._idx_t.view(self.P, 1), out=self.best_feasible_t.view(self.P, 1))
        self.best_feasible_t.masked_fill_(self._none_t, 0)
        out["best_feasible"], out["n_feasible"] = self.best_feasible_t, self.n_feasible_t
        return out


class Planner:
    def __init__(self, env, n_candidates: int, horizon: int, gamma: float = 1.0, crop: str = "nominal", n_scenarios: Optional[int] = None,
                 noise_scale: Optional[float] = None, noise: str = "step", n_tail: Optional[int] = None, scenario_seed: int = 0,
                 weather_sigma=None, weather_phi: float = 0.0):
        if int(n_candidates) < 1 or int(horizon) < 1:
            raise ValueError("n_candidates and horizon must be at least 1")
        if n_scenarios is None:
            if noise_scale is not None or n_tail is not None:
                raise ValueError("noise_scale and n_tail belong to scenario rollouts: give n_scenarios")
            if weather_sigma is not None:
                raise ValueError("weather_sigma belongs to scenario rollouts: give n_scenarios")
        else:
            if not 1 <= int(n_scenarios) <= L.MAX_SCENARIOS:
                raise ValueError(f"n_scenarios must be in 1 .. {L.MAX_SCENARIOS}")
            if not 1 <= int(n_scenarios if n_tail is None else n_tail) <= int(n_scenarios):
                raise ValueError("n_tail must be in 1 .. n_scenarios")
            if noise_scale is not None and not 0.0 <= float(noise_scale) < float("inf"):
                raise ValueError("noise_scale must be finite and >= 0")
            if int(horizon) > 65536 or int(scenario_seed) < 0:
                raise ValueError("scenario rollouts take horizon <= 65 536 and scenario_seed >= 0")
        if noise not in ("step", "hold"):
            raise ValueError("noise must be 'step' or 'hold'")
        sigma = None if weather_sigma is None else _weather_sigma(weather_sigma, weather_phi)
        if sigma is not None and env.B * int(n_scenarios) * int(horizon) > 2 ** 31 - 1:
            raise ValueError("num_envs * n_scenarios * horizon (the rows of the weather windows) must not exceed 2^31 - 1")
        if crop not in ("nominal", "current"):
            raise ValueError("crop must be 'nominal' or 'current'")
        if not (float(gamma) >= 0.0) or float(gamma) == float("inf"):
            raise ValueError("gamma must be finite and >= 0")
        torch = env.torch
        self.env, self.torch = env, torch
        self.K, self.H, self.gamma, self.crop = int(n_candidates), int(horizon), float(gamma), crop
        self.B = env.B
        self.J = self.B * self.K                                     # candidates: rows of an action plane, entries of the scores
        self.S = None if n_scenarios is None else int(n_scenarios)   # scenarios per candidate; None: one deterministic future
        self.C = self.J * (self.S or 1)                              # children
        if self.C > 2 ** 31 - 1:
            raise ValueError("num_envs * n_candidates * n_scenarios must not exceed 2^31 - 1")
        self.ld = (self.C + 63) // 64 * 64
        dev, T = env.device, env.tdtype
        z = lambda *s, dtype=T: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        # the children's environment buffers (what glgym_step reads and writes) ...
        self.x_T, self.u_T = z(L.NX, self.ld), z(L.NU, self.ld)
        self.timestep_t, self.w_off_t = z(self.C, dtype=torch.int32), z(self.C, dtype=torch.int32)
        self.start_day_t = z(self.C, dtype=torch.float32)
        self.crop_T = z(L.NCROP, self.ld) if (self.S or (crop == "current" and env.crop_T is not None)) else None
        self.reward_t, self.info_T = z(self.ld), z(L.NINFO, self.ld)
        self.done_t = z(self.C, dtype=torch.uint8)
        self.step_flags_t = z(self.C, dtype=torch.int32)
        # ... their accumulators ...
        self.ret_t = z(self.C, dtype=torch.float64)
        self.viol_T = z(3, self.ld, dtype=torch.float64)
        self.n_steps_t = z(self.C, dtype=torch.int32)
        self.alive_t, self.failed_t = z(self.C, dtype=torch.uint8), z(self.C, dtype=torch.uint8)
        # ... and the selection's outputs
        self.best_k_t = z(self.B, dtype=torch.int32)
        self.best_ret_t = z(self.B, dtype=torch.float64)
        self.best_action_t = z(self.B, L.NU, dtype=torch.float32)
        self.best_sequence_t = z(self.H, self.B, L.NU, dtype=torch.float32)
        self.mean_sequence_t = z(self.H, self.B, L.NU, dtype=torch.float32)
        self._actions_buf = self._controls_T = None                  # staging, allocated at first use
        self._actions = None                                         # the [H, C, 6] block of the last rollout (select reads it)
        self.draw_base_t = z(1, dtype=torch.int64)                   # device word added to every draw index: add to it between replays
        # the cross-entropy method's population state; its buffers, the elite indices and the distribution are allocated at first use
        self._cem = _CemStages(self, self.B, self.H, self.draw_base_t, "horizon x num_envs x 6")
        self.elite_k_t = self.n_elite_t = self.cem_mean_t = self.cem_std_t = None
        self._draw = 0                                               # draw index of cem()'s next population
        # what select() and elites() score: the children's own returns, or with scenarios the candidates' aggregated ones
        self._score_t, self._score_failed_t = self.ret_t, self.failed_t
        if self.S:
            self.noise_scale = float(env.uncertainty_scale if noise_scale is None else noise_scale)
            self.noise, self.n_tail, self.scenario_seed = noise, int(self.S if n_tail is None else n_tail), int(scenario_seed)
            self.ld_cand = (self.J + 63) // 64 * 64
            self.stage_t = z(self.C, L.NU, dtype=torch.float32)      # ONE expanded action plane, rewritten before every step
            self.ret_cand_t = z(self.J, dtype=torch.float64)
            self.failed_cand_t, self.alive_cand_t = z(self.J, dtype=torch.uint8), z(self.J, dtype=torch.uint8)
            self.viol_cand_T = z(3, self.ld_cand, dtype=torch.float64)
            self.steps_cand_t = z(self.J, dtype=torch.int32)
            self.scenario_base_t = z(1, dtype=torch.int64)           # device word added to the scenario draw index (apart from draw_base_t)
            self._scen_draw = 0                                      # which set of scenarios: new_scenarios() takes the next
            self._score_t, self._score_failed_t = self.ret_cand_t, self.failed_cand_t
            self.scenario_returns = self.ret_t.view(self.B, self.K, self.S)       # per-scenario results of the last rollout
            self.scenario_failed = self.failed_t.view(self.B, self.K, self.S)
        self.weather_sigma, self.weather_phi = sigma, float(weather_phi)
        self.weather_window_t = self.weather_window = None
        if sigma is not None:
            self.weather_window_t = z(self.B * self.S * self.H, env.nd)       # row (b*S + s)*H + h: scenario s of greenhouse b at horizon step h
            self.weather_window = self.weather_window_t.view(self.B, self.S, self.H, env.nd)
        self.x, self.u = self.x_T[:, :self.C].t(), self.u_T[:, :self.C].t()
        self.constraints = self._con = None                          # Constraints.attach / env.planner(constraints=...): _constrain

    def _constrain(self, constraints):
        """Put glgym_plan_constrain behind every rollout (_ConstrainStage: its buffers are allocated here, once) and have select, elites
        and the searches rank its scores.  The runs of a candidate are its S scenarios (one run without scenarios): the stage reads the
        per-run viol_T / n_steps_t, not the scenario means.  Afterwards, per rollout: feasible [B, K] u8, excess [B, K] f64,
        n_violating [B, K] i32, n_feasible [B] i32 (read-only views), score_con_t / failed_con_t [B*K] what is ranked."""
        if self._con is not None:
            raise ValueError("this planner already has constraints")
        self._con = con = _ConstrainStage(self.env, constraints, self.B, 1, self.K, self.S or 1, self.ld, self._score_t, self._score_failed_t,
                                          self.viol_T, self.n_steps_t)
        self.constraints = constraints
        self.score_con_t, self.failed_con_t, self.feasible_t, self.excess_t = con.score_con_t, con.failed_con_t, con.feasible_t, con.excess_t
        self.n_viol_t, self.n_feasible_t = con.n_viol_t, con.n_feasible_t
        self.feasible, self.excess, self.n_violating, self.n_feasible = con.views(self.B)
        self._score_t, self._score_failed_t = con.score_con_t, con.failed_con_t

    def set_layout(self, layout: str):
        """Kernel layout of float32 env-steps (TomatoVecEnv.set_layout; handle state, shared with the environment).  With "auto" the
        CHILD batch decides for the planner's steps: four lanes per environment up to 16 384 children, one lane beyond."""
        self.env.set_layout(layout)

    # ------------------------------------------------------------------------------------------------
    def fork(self, parent_t=None):
        """Copy the environment's current state into the children and zero their accumulators (rollout() calls this).  parent_t:
        optional int32 [B*K] parent index per child (with scenarios [B*K*S]); default child c <- environment c // K (c // (K*S))."""
        e = self.env
        if parent_t is not None and (parent_t.dtype != self.torch.int32 or parent_t.numel() != self.C or not parent_t.is_contiguous()):
            raise ValueError(f"parent_t must be a contiguous int32 tensor of {self.C} entries")
        fork_crop = self.crop_T is not None and not self.S           # scenario children get their block from the prologue of every step
        a = L.make_plan_args(L.PlanForkArgs, self.C, e.B, self.K * (self.S or 1), e.ld, self.ld,
                             parent_t.data_ptr() if parent_t is not None else None,
                             e.x_T.data_ptr(), e.u_T.data_ptr(), e.timestep_t.data_ptr(), e.w_off_t.data_ptr(), e.start_day_t.data_ptr(),
                             e.crop_T.data_ptr() if fork_crop else None,
                             self.x_T.data_ptr(), self.u_T.data_ptr(), self.timestep_t.data_ptr(), self.w_off_t.data_ptr(),
                             self.start_day_t.data_ptr(), self.crop_T.data_ptr() if fork_crop else None,
                             self.ret_t.data_ptr(), self.viol_T.data_ptr(), self.n_steps_t.data_ptr(), self.alive_t.data_ptr(),
                             self.failed_t.data_ptr())
        L.check(e._lib.glgym_plan_fork(e._h, C.byref(a), e._stream()), "glgym_plan_fork")

    def _step_args(self):
        e = self.env
        table, rows = (e.weather_t, e.weather_rows) if self.weather_window_t is None else (self.weather_window_t, self.B * self.S * self.H)
        return L.make_step_args(self.C, self.ld, self.x_T.data_ptr(), self.u_T.data_ptr(), None, None, table.data_ptr(),
                                rows, self.w_off_t.data_ptr(), self.timestep_t.data_ptr(),
                                self.crop_T.data_ptr() if self.crop_T is not None else None, e.N, self.reward_t.data_ptr(),
                                self.info_T.data_ptr(), self.done_t.data_ptr(), None, self.step_flags_t.data_ptr())

    def _weather(self):
        """glgym_plan_weather: the scenarios' windows from the parents' coming rows, and the children's offsets into them (after fork(),
        whose w_off they replace).  Reads the parents' w_off / timestep on the device: a replayed graph follows the environment."""
        e = self.env
        a = L.make_plan_args(L.PlanWeatherArgs, self.B, self.K, self.S, self.H, e.weather_rows, e.weather_t.data_ptr(), e.w_off_t.data_ptr(),
                             e.timestep_t.data_ptr(), (C.c_double * 7)(*self.weather_sigma), self.weather_phi,
                             self.scenario_seed & (2 ** 64 - 1), self._scen_draw, self.scenario_base_t.data_ptr(),
                             self.weather_window_t.data_ptr(), self.w_off_t.data_ptr())
        L.check(e._lib.glgym_plan_weather(e._h, C.byref(a), e._stream()), "glgym_plan_weather")

    def rollout(self, actions_t=None, controls_t=None):
        """Fork from the environment's current state and run the H-step rollout of every candidate.
        actions_t [H, B*K, 6] (or [H, B, K, 6]) f32 in [-1, 1]: the action path of step_tensor; a contiguous float32 tensor on the
        environment's device is read in place.  controls_t [H, B*K, 6]: raw controls (step_raw_control).  Child b*K + k is candidate k
        of environment b.
        Returns device tensors (views of the planner's buffers, overwritten by the next rollout): returns [B, K] f64, alive [B, K] u8,
        steps [B, K] i32, violations [3, B, K] f64 (co2, temp, rh), failed [B, K] u8.
        With scenarios (actions_t only): every candidate runs under its S futures; returned per candidate are the mean of its n_tail
        worst returns (NaN, with failed = 1, if a scenario failed or came back non-finite), alive = alive in every scenario, steps =
        the fewest over the scenarios, the violations' means; scenario_returns / scenario_failed [B, K, S] hold the single runs.
        With weather_sigma the scenarios' weather windows are rebuilt from the environment's present position first (weather_window
        [B, S, H, nd] holds them afterwards)."""
        if (actions_t is None) == (controls_t is None):
            raise ValueError("give exactly one of actions_t / controls_t")
        if self.S and controls_t is not None:
            raise ValueError("scenario rollouts take actions_t: raw controls are not supported")
        torch, e = self.torch, self.env
        n = self.H * self.J * L.NU
        act_ptr = ctl_ptr = None
        if actions_t is not None:
            if actions_t.numel() != n:
                raise ValueError(f"actions_t must hold horizon x (num_envs * n_candidates) x 6 = {n} values, got {tuple(actions_t.shape)}")
            if actions_t.dtype == torch.float32 and actions_t.is_cuda and actions_t.device == e.device and actions_t.is_contiguous():
                self._actions = actions_t.view(self.H, self.J, L.NU)
            else:
                if self._actions_buf is None:
                    self._actions_buf = torch.zeros(self.H, self.J, L.NU, dtype=torch.float32, device=e.device)
                self._actions_buf.copy_(actions_t.reshape(self.H, self.J, L.NU))
                self._actions = self._actions_buf
            act_ptr = self._actions.data_ptr()
        else:
            if controls_t.numel() != n:
                raise ValueError(f"controls_t must hold horizon x (num_envs * n_candidates) x 6 = {n} values, got {tuple(controls_t.shape)}")
            if self._controls_T is None:
                self._controls_T = torch.zeros(self.H, L.NU, self.ld, dtype=e.tdtype, device=e.device)
            self._controls_T[:, :, :self.C].copy_(controls_t.reshape(self.H, self.C, L.NU).transpose(1, 2))
            self._actions = None
            ctl_ptr = self._controls_T.data_ptr()
        self._cem.note_rollout(actions_t)                            # one of the CEM's own blocks is always read in place
        self._fork_children()
        a = self._rollout_args(act_ptr, ctl_ptr)
        if self.S:
            sc = L.make_plan_args(L.PlanRolloutScenariosArgs, *self._scenario_args(), self.stage_t.data_ptr(), a)
            L.check(e._lib.glgym_plan_rollout_scenarios(e._h, C.byref(sc), e._stream()), "glgym_plan_rollout_scenarios")
        else:
            L.check(e._lib.glgym_plan_rollout(e._h, C.byref(a), e._stream()), "glgym_plan_rollout")
        return self._results()

    # what the three rollouts (this one, RuleSearch's, PolicySearch's) share
    def _fork_children(self):
        """fork(), then with weather_sigma the scenarios' windows."""
        self.fork()
        if self.weather_window_t is not None:
            self._weather()

    def _rollout_args(self, act_ptr, ctl_ptr):
        """The glgym_plan_rollout_args over the children's buffers and accumulators, reading actions / controls planes at these pointers."""
        return L.make_plan_args(L.PlanRolloutArgs, self.H, self.gamma, self._step_args(), act_ptr, ctl_ptr, self.ret_t.data_ptr(),
                                self.viol_T.data_ptr(), self.n_steps_t.data_ptr(), self.alive_t.data_ptr(), self.failed_t.data_ptr())

    def _scenario_args(self):
        """(B, K, S, hold, noise_scale, seed, draw, scenario_base) as the scenario rollouts take them; all zero without scenarios."""
        if not self.S:
            return (0, 0, 0, 0, 0.0, 0, 0, None)
        return (self.B, self.K, self.S, 1 if self.noise == "hold" else 0, self.noise_scale, self.scenario_seed & (2 ** 64 - 1),
                self._scen_draw, self.scenario_base_t.data_ptr())

    def _results(self):
        """The five tensors a rollout returns: views of the children's accumulators, or with scenarios glgym_plan_aggregate over the S
        runs of every candidate.  With constraints glgym_plan_constrain comes last: the five tensors stay the raw ones, the scores that
        select and elites rank go to score_con_t / failed_con_t."""
        e, B, K = self.env, self.B, self.K
        if not self.S:
            if self._con is not None:
                self._con.run()
            return (self.ret_t.view(B, K), self.alive_t.view(B, K), self.n_steps_t.view(B, K), self.viol_T[:, :self.C].view(3, B, K),
                    self.failed_t.view(B, K))
        g = L.make_plan_args(L.PlanAggregateArgs, self.J, self.S, self.n_tail, self.ld, self.ld_cand, self.ret_t.data_ptr(),
                             self.failed_t.data_ptr(), self.viol_T.data_ptr(), self.n_steps_t.data_ptr(), self.ret_cand_t.data_ptr(),
                             self.failed_cand_t.data_ptr(), self.viol_cand_T.data_ptr(), self.steps_cand_t.data_ptr())
        L.check(e._lib.glgym_plan_aggregate(e._h, C.byref(g), e._stream()), "glgym_plan_aggregate")
        self.torch.amin(self.alive_t.view(self.J, self.S), dim=1, out=self.alive_cand_t)
        if self._con is not None:
            self._con.run()
        return (self.ret_cand_t.view(B, K), self.alive_cand_t.view(B, K), self.steps_cand_t.view(B, K),
                self.viol_cand_T[:, :self.J].view(3, B, K), self.failed_cand_t.view(B, K))

    def new_scenarios(self):
        """Draw other futures (crop and weather alike) from the next scenario rollout on: the scenario draw index moves by one.  (A replayed
        graph carries the index it was captured with: add to scenario_base_t instead.)"""
        if not self.S:
            raise ValueError("new_scenarios() belongs to a planner built with n_scenarios")
        self._scen_draw += 1

    def select(self, temperature: Optional[float] = None, sequence: bool = False) -> Dict[str, Any]:
        """Best candidate per environment from the last rollout: {"best_k" [B] i32 (-1: every candidate failed or came back
        non-finite), "best_return" [B] f64 (NaN then), "best_action" [B, 6] f32 = the best candidate's first action (zeros then)}, with
        sequence=True also "best_sequence" [H, B, 6], with temperature > 0 also "mean_sequence" [H, B, 6]: the MPPI mean with weights
        exp((return - max) / temperature) over the admissible candidates.  After a rollout of raw controls only best_k / best_return
        are available.  Device tensors, overwritten by the next call.
        With constraints the candidates are ranked by their constrained scores, best_return is the best SCORE -- the candidate's
        return whenever best_feasible = 1 -- and the dict gains "best_feasible" [B] u8 (0 when best_k = -1) and "n_feasible" [B] i32."""
        e = self.env
        has_a = self._actions is not None
        if not has_a and (sequence or temperature is not None):
            raise ValueError("best_sequence / mean_sequence need a rollout of actions_t")
        if temperature is not None:
            _select_temperature(temperature)
        a = L.make_plan_args(L.PlanSelectArgs, self.B, self.K, self.H, self._score_t.data_ptr(), self._score_failed_t.data_ptr(),
                             self._actions.data_ptr() if has_a else None, self.best_k_t.data_ptr(), self.best_ret_t.data_ptr(),
                             self.best_action_t.data_ptr() if has_a else None, self.best_sequence_t.data_ptr() if sequence else None,
                             float(temperature) if temperature is not None else 0.0,
                             self.mean_sequence_t.data_ptr() if temperature is not None else None)
        L.check(e._lib.glgym_plan_select(e._h, C.byref(a), e._stream()), "glgym_plan_select")
        out = {"best_k": self.best_k_t, "best_return": self.best_ret_t}
        if has_a:
            out["best_action"] = self.best_action_t
        if sequence:
            out["best_sequence"] = self.best_sequence_t
        if temperature is not None:
            out["mean_sequence"] = self.mean_sequence_t
        if self._con is not None:
            self._con.best(self.best_k_t, out)
        return out

    # ---- the cross-entropy method ------------------------------------------------------------------------------------------
    def _cem_alloc(self):
        """The first CEM call allocates (a random-shooting planner never does): the population blocks, the elite indices, the distribution."""
        if self.cem_mean_t is None:
            self.elite_k_t, self.n_elite_t = self._cem.alloc()
            self.cem_mean_t = self.torch.zeros(self.H, self.B, L.NU, dtype=self.torch.float32, device=self.env.device)
            self.cem_std_t = self.torch.zeros_like(self.cem_mean_t)

    def sample(self, mean_t, std_t, beta: float = 0.0, seed: int = 0, draw_index: int = 0, carry: int = 0):
        """glgym_plan_sample: draw the population [H, B*K, 6] from N(mean_t, std_t) [H, B, 6] with lag-1 correlation beta along the
        horizon, clipped to [-1, 1], into the planner's action block that the previous population does not occupy; returns it (pass it
        to rollout()).  Candidate 0 is the clipped mean; with carry >= 1, and elites() of the previous sampled population at hand,
        candidates 1 .. carry are its best sequences.  Noise: Philox keyed by seed, counter (child, step, draw_index + draw_base_t)."""
        return self._cem.sample(mean_t, std_t, beta, seed, draw_index, carry)

    def elites(self, n_elite: int):
        """glgym_plan_elites on the last rollout: (elite_k [B, n_elite] i32 -- the admissible candidates by return, best first, ties to
        the lower index, padded with -1 --, n_elite [B] i32).  Views of planner buffers, overwritten by the next call."""
        return self._cem.elites(self._score_t, self._score_failed_t, n_elite)

    def refit(self, mean_t, std_t, alpha: float, min_std: float):
        """glgym_plan_refit, in place on mean_t / std_t [H, B, 6]: mean <- alpha*mean + (1-alpha)*(the elites' mean), std <-
        max(alpha*std + (1-alpha)*(their standard deviation, ddof 0), min_std), over the elites() of the last rollout's actions.  A
        greenhouse without an elite keeps its row."""
        return self._cem.refit(self._actions, mean_t, std_t, alpha, min_std)

    def cem(self, n_iter: int, n_elite: int, init_std: float = 0.5, min_std: float = 0.05, alpha: float = 0.1, beta: float = 0.0,
            carry: int = 0, seed: int = 0, mean_t=None, std_t=None) -> Dict[str, Any]:
        """One receding-horizon decision by the cross-entropy method: n_iter x (sample -> rollout -> elites -> refit), then
        select(sequence=True) on the last population.  mean_t None: start from zeros ("hold the controls"), spread init_std, nothing
        carried into the first population; otherwise from mean_t / std_t [H, B, 6] (std_t None: init_std) -- the planner's own
        cem_mean_t / cem_std_t after shift() for a warm start.  carry <= n_elite elites survive from one population into the next.
        Every sample() takes the next draw index of the planner's lifetime.
        Returns device tensors, planner buffers overwritten by the next call: mean_sequence, std_sequence [H, B, 6], best_sequence,
        best_action, best_return, best_k (select()'s), elite_k [B, n_elite], n_elite [B].  No host synchronisation and, after the
        first call, no allocation: a whole cem() can be captured in a graph (add n_iter to draw_base_t between replays for fresh
        noise).  With scenarios every iteration scores its population on the SAME futures (a carried elite keeps its score); call
        new_scenarios(), or add to scenario_base_t between replays, for other ones."""
        st = self._cem
        n_iter, E, carry = st.check_hyper(n_iter, n_elite, carry, init_std, min_std, alpha, beta, seed)
        self._cem_alloc()
        if mean_t is not None or std_t is not None:
            st.check_dist(mean_t if mean_t is not None else std_t, std_t if std_t is not None else mean_t)
        if mean_t is None:
            self.cem_mean_t.zero_()
            st.drop_carry()
        elif mean_t.data_ptr() != self.cem_mean_t.data_ptr():
            self.cem_mean_t.copy_(mean_t.view(self.H, self.B, L.NU))
        if std_t is None:
            self.cem_std_t.fill_(float(init_std))
        elif std_t.data_ptr() != self.cem_std_t.data_ptr():
            self.cem_std_t.copy_(std_t.view(self.H, self.B, L.NU))
        elite_k, n_el = st.run(self.cem_mean_t, self.cem_std_t, n_iter, E, alpha, min_std, beta, carry, seed)
        sel = self.select(sequence=True)
        out = {"mean_sequence": self.cem_mean_t, "std_sequence": self.cem_std_t, "best_sequence": sel["best_sequence"],
               "best_action": sel["best_action"], "best_return": sel["best_return"], "best_k": sel["best_k"], "elite_k": elite_k,
               "n_elite": n_el}
        if self._con is not None:                                    # with constraints: select()'s best_feasible and n_feasible as well
            out.update(best_feasible=sel["best_feasible"], n_feasible=sel["n_feasible"])
        return out

    def shift(self, fill_std: float):
        """Receding-horizon warm start on cem()'s distribution: mean[h] <- mean[h+1], last row 0; std[h] <- std[h+1], last row
        fill_std.  The carried elites belong to the unshifted horizon and are dropped."""
        if self.cem_mean_t is None:
            raise ValueError("shift() moves the distribution of a previous cem()")
        if not 0.0 <= float(fill_std) < float("inf"):
            raise ValueError("fill_std must be finite and >= 0")
        for t, last in ((self.cem_mean_t, 0.0), (self.cem_std_t, float(fill_std))):
            if self.H > 1:
                t[:-1].copy_(t[1:].clone())
            t[-1].fill_(last)
        self._cem.drop_carry()
        return self.cem_mean_t, self.cem_std_t


# ---- closed-loop rule-based rollouts and controller tuning (include/glgym.h glgym_rule_rows / glgym_plan_rollout_rule) --------------
RULE_CLOCK_QUANTUM = 450.0        # [s] dt / 3600 must be a multiple of 1/8 h: then timestep * dt / 3600 is the reference's running sum


def check_rule_dt(dt: float) -> None:
    """The children's clocks are DERIVED, hour = (timestep * dt / 3600) mod 24 (glgym_rule_args with hour = NULL).  The reference keeps
    a running sum, which the product reproduces exactly only where the increment is a multiple of 1/8 h, dt a multiple of 450 s; the
    environment's running-sum table for other steps (dt = 300 s) is not forked.  ValueError otherwise."""
    if not float(dt) > 0.0 or float(dt) % RULE_CLOCK_QUANTUM != 0.0:
        raise ValueError(f"rule-based rollouts need dt to be a multiple of {RULE_CLOCK_QUANTUM:g} s (got {dt}): the children's clocks are "
                         "derived from the timestep by the product form; the running-sum clock of other steps is not forked")


class RuleParams:
    """The search space of a controller tuning on the host: which of the 29 constants of gl_gym_amd.baseline.RuleBasedController are
    tuned, between which bounds, and the base controller the others come from -- include/glgym.h glgym_rule_space.  tune: {name: (lo, hi)},
    in the order given (component i of theta is the i-th name).  encode / decode are NumPy restatements of the header's map."""

    def __init__(self, tune, base=None):
        import numpy as np
        from .baseline import RuleBasedController
        self.np = np
        self.base = RuleBasedController() if base is None else base
        if not tune:
            raise ValueError("tune must name at least one controller constant: {name: (lo, hi), ...}")
        unknown = sorted(set(tune) - set(L.RULE_FIELDS))
        if unknown:
            raise ValueError(f"tune: unknown controller constants {unknown}; the names are {L.RULE_FIELDS}")
        self.names = tuple(tune)
        self.D, self.Ht = len(self.names), (len(self.names) + L.NU - 1) // L.NU
        self.field = [L.RULE_FIELDS.index(n) for n in self.names]
        try:
            bounds = np.array([[float(tune[n][0]), float(tune[n][1])] for n in self.names], dtype=np.float64).reshape(self.D, 2)
        except (TypeError, IndexError):
            raise ValueError("tune: every entry must be a (lo, hi) pair of numbers") from None
        self.lo, self.hi = bounds[:, 0].copy(), bounds[:, 1].copy()
        if not np.isfinite(bounds).all() or (self.lo > self.hi).any():
            raise ValueError("tune: bounds must be finite with lo <= hi")
        for n, lo, hi in zip(self.names, self.lo, self.hi):
            if n in L.RULE_BANDS and lo <= 0.0 <= hi:
                raise ValueError(f"tune: the interval of the proportional band {n} must not contain 0 (the rules divide by it)")
        for n in L.RULE_BANDS:
            if n not in self.names and float(getattr(self.base, n)) == 0.0:
                raise ValueError(f"base: the proportional band {n} is 0 (the rules divide by it)")

    def struct(self):
        """The glgym_rule_space: the base controller's 29 constants, and field index, lo and hi of every tuned one."""
        s = L.RuleSpace()
        s.base = L.RuleCfg(*[float(getattr(self.base, n)) for n in L.RULE_FIELDS])
        s.D = self.D
        for i in range(self.D):
            s.field[i], s.lo[i], s.hi[i] = self.field[i], self.lo[i], self.hi[i]
        return s

    def values(self, controller_or_dict):
        """The tuned constants of a controller, or of a dict (names it lacks come from base) -> float64 [D]."""
        src = controller_or_dict
        if isinstance(src, dict):
            unknown = sorted(set(src) - set(L.RULE_FIELDS))
            if unknown:
                raise ValueError(f"unknown controller constants {unknown}")
            return self.np.array([float(src.get(n, getattr(self.base, n))) for n in self.names], dtype=self.np.float64)
        return self.np.array([float(getattr(src, n)) for n in self.names], dtype=self.np.float64)

    def inside(self, controller_or_dict) -> bool:
        """Whether every tuned constant of the controller (or dict) lies within its bounds: whether encode() takes it."""
        v = self.values(controller_or_dict)
        return bool(((self.lo <= v) & (v <= self.hi)).all())

    def encode(self, controller_or_dict):
        """-> theta float32 [Ht, 1, 6]: tuned constant i mapped from [lo_i, hi_i] onto [-1, 1] (0 where lo_i = hi_i), padding 0.
        ValueError if a value lies outside its bounds."""
        np, v = self.np, self.values(controller_or_dict)
        if not self.inside(controller_or_dict):
            bad = [n for n, x, lo, hi in zip(self.names, v, self.lo, self.hi) if not lo <= x <= hi]
            raise ValueError(f"encode: {bad} outside the bounds of the search space")
        span = self.hi - self.lo
        t = np.where(span > 0, 2.0 * (v - self.lo) / np.where(span > 0, span, 1.0) - 1.0, 0.0)
        theta = np.zeros(self.Ht * L.NU, dtype=np.float32)
        theta[:self.D] = t.astype(np.float32)
        return theta.reshape(self.Ht, 1, L.NU)

    def decode(self, theta):
        """theta [Ht, J, 6] (any float array) -> {name: float64 [J]} by the header's formula; a NaN reads as -1, i.e. lo."""
        np = self.np
        th = np.asarray(theta, dtype=np.float32).reshape(self.Ht, -1, L.NU)
        comp = th.transpose(1, 0, 2).reshape(th.shape[1], self.Ht * L.NU)[:, :self.D].astype(np.float64)
        t = np.fmin(np.fmax(comp, -1.0), 1.0)
        v = self.lo + (self.hi - self.lo) * (0.5 * (t + 1.0))
        return {n: v[:, i].copy() for i, n in enumerate(self.names)}


# ---- the cross-entropy method's stages (include/glgym.h glgym_plan_sample / _elites / _refit) ----------------------------------------
class _CemStages:
    """sample, elites and refit over a population block [Hd, P*K, 6], in one place for Planner (Hd = H, P = B, its own beta) and the
    theta searches (Hd = Ht, P = B or 1, beta = 0), and the population state every sampler shares: `blocks`, the two blocks (a
    population is sampled into the one the previous population does not occupy, so that its elites can be carried over); `cur`, which of
    them holds the population sampled last; `rolled`, which of them the last rollout simulated, if one of them; `ranked`, (E, block) of
    the last elites(): the row length of elite_k_t, and the block it ranks if the next sample() may carry from it, else None.
    `owner` supplies env, torch, K, rollout, elites, refit, _draw and _cem_alloc, which is called before the first launch and has
    alloc() allocate: Planner at its first CEM call, the searches in __init__.  What a rollout leaves behind -- its block and the scores
    -- stays with the owner and is passed to elites() and refit().  The owner holds the stages, the stages only a weak reference back:
    without a reference cycle a dropped planner frees its device buffers at once, not at the next garbage collection."""

    def __init__(self, owner, P, Hd, draw_base_t, dist_doc):
        self.o, self.P, self.Hd, self.draw_base_t, self.dist_doc = weakref.proxy(owner), int(P), int(Hd), draw_base_t, dist_doc
        self.blocks = self.cur = self.rolled = self.ranked = None
        self.elite_k_t = self.n_elite_t = None

    def alloc(self):
        """-> (elite_k_t [P*K] i32: rows of E <= K entries, [P, E] is a view; n_elite_t [P] i32), after the two blocks."""
        torch, dev, J = self.o.torch, self.o.env.device, self.P * self.o.K
        self.blocks = [torch.zeros(self.Hd, J, L.NU, dtype=torch.float32, device=dev) for _ in range(2)]
        self.elite_k_t = torch.full((J,), -1, dtype=torch.int32, device=dev)
        self.n_elite_t = torch.zeros(self.P, dtype=torch.int32, device=dev)
        return self.elite_k_t, self.n_elite_t

    # the population state, for every sampler (sample below, _EsStages.sample_mirrored, _CmaStages.sample) and every rollout
    def free(self):
        """Index of the block the next population goes into."""
        return 0 if self.cur is None else 1 - self.cur

    def occupy(self, dst):
        """A population was sampled into blocks[dst]: the elites at hand rank another one, and none of them is carried."""
        self.cur = dst
        self.drop_carry()
        return self.blocks[dst]

    def drop_carry(self):
        if self.ranked:
            self.ranked = (self.ranked[0], None)

    def note_rollout(self, block_t):
        """The owner's rollout reads block_t (None: something else than a tensor read in place)."""
        self.rolled = next((i for i, b in enumerate(self.blocks or ()) if block_t is b), None)

    def check_dist(self, mean_t, std_t):
        torch, n = self.o.torch, self.Hd * self.P * L.NU
        for name, t in (("mean_t", mean_t), ("std_t", std_t)):
            if (t is None or t.dtype != torch.float32 or not t.is_cuda or t.device != self.o.env.device or not t.is_contiguous()
                    or t.numel() != n):
                raise ValueError(f"{name} must be a contiguous float32 tensor of {self.dist_doc} = {n} values on the environment's device")

    def sample(self, mean_t, std_t, beta=0.0, seed=0, draw_index=0, carry=0):
        self.check_dist(mean_t, std_t)
        if not 0.0 <= float(beta) < 1.0:
            raise ValueError("beta must be in [0, 1)")
        if int(carry) < 0 or int(seed) < 0 or int(draw_index) < 0:
            raise ValueError("carry, seed and draw_index must be >= 0")
        n_elites, src = self.ranked or (0, None)
        carried = int(carry) if src is not None else 0               # nothing ranked to carry from: every candidate but 0 is sampled
        if carried > n_elites:
            raise ValueError(f"carry = {carry} exceeds the {n_elites} elites of the previous population")
        self.o._cem_alloc()
        e, dst = self.o.env, self.free()                             # src, when set, is cur: the other block
        a = L.make_plan_args(L.PlanSampleArgs, self.P, self.o.K, self.Hd, mean_t.data_ptr(), std_t.data_ptr(), float(beta),
                             int(seed) & (2 ** 64 - 1), int(draw_index) & (2 ** 64 - 1), self.draw_base_t.data_ptr(),
                             self.blocks[dst].data_ptr(), carried, n_elites if carried else 0,
                             self.blocks[src].data_ptr() if carried else None, self.elite_k_t.data_ptr() if carried else None,
                             self.n_elite_t.data_ptr() if carried else None)
        L.check(e._lib.glgym_plan_sample(e._h, C.byref(a), e._stream()), "glgym_plan_sample")
        return self.occupy(dst)

    def elites(self, score_t, score_failed_t, n_elite):
        E = int(n_elite)
        if not 1 <= E <= self.o.K:
            raise ValueError(f"n_elite must be in 1 .. n_candidates = {self.o.K}")
        self.o._cem_alloc()
        e = self.o.env
        a = L.make_plan_args(L.PlanElitesArgs, self.P, self.o.K, E, score_t.data_ptr(), score_failed_t.data_ptr(), self.elite_k_t.data_ptr(),
                             self.n_elite_t.data_ptr())
        L.check(e._lib.glgym_plan_elites(e._h, C.byref(a), e._stream()), "glgym_plan_elites")
        self.ranked = (E, self.rolled if self.rolled == self.cur else None)
        return self.elite_k_t[:self.P * E].view(self.P, E), self.n_elite_t

    def refit(self, block_t, mean_t, std_t, alpha, min_std):
        """block_t: the block of the owner's last rollout, None if it read none."""
        self.check_dist(mean_t, std_t)
        if not 0.0 <= float(alpha) < 1.0:
            raise ValueError("alpha must be in [0, 1)")
        if not 0.0 <= float(min_std) < float("inf"):
            raise ValueError("min_std must be finite and >= 0")
        if block_t is None or self.ranked is None:
            raise ValueError("refit needs a rollout (of actions or theta, not of raw controls) and its elites()")
        e = self.o.env
        a = L.make_plan_args(L.PlanRefitArgs, self.P, self.o.K, self.Hd, self.ranked[0], block_t.data_ptr(), self.elite_k_t.data_ptr(),
                             self.n_elite_t.data_ptr(), float(alpha), float(min_std), mean_t.data_ptr(), std_t.data_ptr(),
                             mean_t.data_ptr(), std_t.data_ptr())
        L.check(e._lib.glgym_plan_refit(e._h, C.byref(a), e._stream()), "glgym_plan_refit")
        return mean_t, std_t

    def check_hyper(self, n_iter, n_elite, carry, init_std, min_std, alpha, beta, seed):
        """ValueError on what cem() refuses; -> (n_iter, n_elite, carry) as ints."""
        n_iter, E, carry = int(n_iter), int(n_elite), int(carry)
        if n_iter < 1:
            raise ValueError("n_iter must be at least 1")
        if not 1 <= E <= self.o.K:
            raise ValueError(f"n_elite must be in 1 .. n_candidates = {self.o.K}")
        if not 0 <= carry <= E:
            raise ValueError("carry must be in 0 .. n_elite")
        if not 0.0 <= float(beta) < 1.0 or not 0.0 <= float(alpha) < 1.0:
            raise ValueError("alpha and beta must be in [0, 1)")
        if not 0.0 <= float(min_std) < float("inf") or not 0.0 <= float(init_std) < float("inf") or int(seed) < 0:
            raise ValueError("min_std and init_std must be finite and >= 0, seed >= 0")
        return n_iter, E, carry

    def run(self, mean_t, std_t, n_iter, n_elite, alpha, min_std, beta, carry, seed):
        """n_iter x (sample -> rollout -> elites -> refit) on the owner's distribution; -> the last elites()."""
        o = self.o
        for _ in range(n_iter):
            block = self.sample(mean_t, std_t, beta, seed, o._draw, carry)
            o._draw += 1
            o.rollout(block)
            ranked = o.elites(n_elite)
            o.refit(mean_t, std_t, alpha, min_std)
        return ranked


# ---- evolution strategy over theta (include/glgym.h glgym_plan_es_sample / _es_utilities / _es_update) -------------------------------
class _EsStages:
    """The evolution strategy's stages for the theta searches, in one place.  `search` (a _ThetaSearch) supplies env, K, Ht, plan, the
    population state (_cem: the two blocks and which one is free), the block of its last rollout (_theta), rollout, select, _start,
    mean_t / std_t and _draw, P, the number of distribution rows, and score_t / score_failed_t [P*K], what its rollouts leave behind.
    Built at the first ES call, which is the only one that allocates: u_t [P*K] f64, n_adm_t [P] i32, the Adam moments m1_t / m2_t
    [Ht, P, 6] f64, and t_base_t, the device word added to every step count (as plan.draw_base_t is to every draw index)."""

    def __init__(self, search):
        torch, dev = search.torch, search.env.device
        if search.K < 2 or search.K % 2:
            raise ValueError(f"the evolution strategy draws mirrored pairs: n_candidates must be even and >= 2, got {search.K}")
        self.s, self.P, self.score_t, self.score_failed_t = search, search.P, search.score_t, search.score_failed_t
        self.u_t = torch.zeros(self.P * search.K, dtype=torch.float64, device=dev)
        self.n_adm_t = torch.zeros(self.P, dtype=torch.int32, device=dev)
        self.m1_t = torch.zeros(search.Ht, self.P, L.NU, dtype=torch.float64, device=dev)
        self.m2_t = torch.zeros_like(self.m1_t)
        self.t_base_t = torch.zeros(1, dtype=torch.int64, device=dev)
        self.t = 0                                                   # updates since the last restart
        self._scored = None                                          # the block utilities() belongs to

    def restart(self):
        self.m1_t.zero_()
        self.m2_t.zero_()
        self.t = 0

    def sample_mirrored(self, mean_t, std_t, seed=0, draw_index=0):
        s, e = self.s, self.s.env
        s._cem.check_dist(mean_t, std_t)
        if int(seed) < 0 or int(draw_index) < 0:
            raise ValueError("seed and draw_index must be >= 0")
        dst = s._cem.free()
        a = L.make_plan_args(L.PlanEsSampleArgs, self.P, s.K, s.Ht, mean_t.data_ptr(), std_t.data_ptr(), int(seed) & (2 ** 64 - 1),
                             int(draw_index) & (2 ** 64 - 1), s.plan.draw_base_t.data_ptr(), s._cem.blocks[dst].data_ptr())
        L.check(e._lib.glgym_plan_es_sample(e._h, C.byref(a), e._stream()), "glgym_plan_es_sample")
        return s._cem.occupy(dst)

    def utilities(self):
        s, e = self.s, self.s.env
        if s._theta is None:
            raise ValueError("utilities needs a rollout")
        a = L.make_plan_args(L.PlanEsUtilitiesArgs, self.P, s.K, self.score_t.data_ptr(), self.score_failed_t.data_ptr(),
                             self.u_t.data_ptr(), self.n_adm_t.data_ptr())
        L.check(e._lib.glgym_plan_es_utilities(e._h, C.byref(a), e._stream()), "glgym_plan_es_utilities")
        self._scored = s._theta
        return self.u_t.view(self.P, s.K), self.n_adm_t

    @staticmethod
    def check_hyper(lr, lr_std, std_decay, min_std, max_std, optimizer, betas, eps):
        inf = float("inf")
        if optimizer not in L.ES_OPTIMIZERS:
            raise ValueError(f"optimizer must be one of {sorted(L.ES_OPTIMIZERS)}")
        if not 0.0 <= float(lr) < inf or not 0.0 <= float(lr_std) < inf:
            raise ValueError("lr and lr_std must be finite and >= 0")
        if not 0.0 < float(std_decay) < inf:
            raise ValueError("std_decay must be finite and > 0")
        if not 0.0 <= float(min_std) <= float(max_std) < inf:
            raise ValueError("min_std and max_std must be finite with 0 <= min_std <= max_std")
        b1, b2 = (float(b) for b in betas)
        if optimizer == "adam" and (not 0.0 <= b1 < 1.0 or not 0.0 <= b2 < 1.0 or not 0.0 < float(eps) < inf):
            raise ValueError("betas must lie in [0, 1) and eps must be finite and > 0")
        return b1, b2

    def update(self, mean_t, std_t, lr, lr_std=0.0, std_decay=1.0, *, min_std, max_std=1.0, optimizer="adam", betas=(0.9, 0.999), eps=1e-8):
        s, e = self.s, self.s.env
        s._cem.check_dist(mean_t, std_t)
        b1, b2 = self.check_hyper(lr, lr_std, std_decay, min_std, max_std, optimizer, betas, eps)
        if self._scored is None or self._scored is not s._theta:
            raise ValueError("es_update needs a rollout and its utilities()")
        a = L.make_plan_args(L.PlanEsUpdateArgs, self.P, s.K, s.Ht, L.ES_OPTIMIZERS[optimizer], self._scored.data_ptr(), self.u_t.data_ptr(),
                             self.n_adm_t.data_ptr(), float(lr), float(lr_std), float(std_decay), float(min_std), float(max_std), b1, b2,
                             float(eps), self.t + 1, self.t_base_t.data_ptr(), self.m1_t.data_ptr(), self.m2_t.data_ptr(),
                             mean_t.data_ptr(), std_t.data_ptr(), mean_t.data_ptr(), std_t.data_ptr())
        L.check(e._lib.glgym_plan_es_update(e._h, C.byref(a), e._stream()), "glgym_plan_es_update")
        self.t += 1
        return mean_t, std_t

    def run(self, n_iter, lr, lr_std, init_std, min_std, max_std, std_decay, optimizer, betas, eps, seed, mean, resume):
        s = self.s
        n_iter = int(n_iter)
        if n_iter < 1:
            raise ValueError("n_iter must be at least 1")
        self.check_hyper(lr, lr_std, std_decay, min_std, max_std, optimizer, betas, eps)
        if not 0.0 <= float(init_std) < float("inf") or int(seed) < 0:
            raise ValueError("init_std must be finite and >= 0, seed >= 0")
        if resume and mean is not None:
            raise ValueError("resume=True continues from mean_t / std_t: it takes no mean")
        if not resume:
            s._start(mean)
            s.std_t.fill_(float(init_std))
            self.restart()
        for _ in range(n_iter):
            block = self.sample_mirrored(s.mean_t, s.std_t, seed=seed, draw_index=s._draw)
            s._draw += 1
            s.rollout(block)
            u, n_adm = self.utilities()
            self.update(s.mean_t, s.std_t, lr, lr_std, std_decay, min_std=min_std, max_std=max_std, optimizer=optimizer, betas=betas, eps=eps)
        out = dict(s.select())
        out.update(mean=s.mean_t, std=s.std_t, u=u, n_adm=n_adm)
        return out


_ES_DOC = """Evolution strategy: n_iter x (sample_mirrored -> rollout -> utilities -> es_update), then select() on the last population.
        Mirrored pairs (n_candidates even), centred ranks over the WHOLE population, a search-gradient step on the mean ("adam" or
        "sgd", ascending the return) and the separable-NES update of the spread, std <- clip(std * std_decay * exp(lr_std / 2 * s),
        min_std, max_std); lr_std = 0 with std_decay = 1 keeps the spread at init_std.  The start is cem()'s: `mean`, or this object's
        default.  resume=True continues instead from mean_t / std_t, the Adam moments and the step count of the previous call.  Every
        sample takes the next draw index of this object's lifetime.
        Returns device tensors, overwritten by the next call: what select() returns, mean, std, u [P, K] f64, n_adm [P] i32.  No host
        synchronisation and, after the first call, no allocation: a whole es() can be captured in a graph; between replays add n_iter
        to plan.draw_base_t for fresh noise and, with resume=True, to es_t_base for the next Adam steps."""


# ---- CMA-ES with a full covariance matrix over theta (include/glgym.h glgym_plan_cma_sample / _cma_update) ---------------------------
class _CmaStages:
    """The CMA-ES stages for RuleSearch.  `search` supplies env, B, K, D, Ht, plan, the population state (_cem: the two blocks, which
    one is free, the elites), the block of its last rollout (_theta), elites, rollout, select, _start, mean_t and _draw.  Built at the
    first CMA call, which is the only one that allocates: sigma_t [B] f64, cov_t / chol_t [B, N, N] f64, p_sigma_t / p_c_t [B, N] f64,
    status_t [B] i32, the weights on the device (one array per n_elite, kept), and t_base_t, the device word added to every generation
    count.  A policy net is not served: even a linear policy has 144 parameters, and a 144 x 144 matrix per row is another design
    (DESIGN.md section 2.18)."""

    def __init__(self, search):
        torch, dev = search.torch, search.env.device
        self.s, self.P, self.N = search, int(search.B), int(search.D)
        if not 1 <= self.N <= L.CMA_NMAX:
            raise ValueError(f"CMA-ES keeps a full covariance matrix: 1 .. {L.CMA_NMAX} tuned constants, got {self.N}")
        z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)  # noqa: E731
        self.sigma_t, self.cov_t, self.chol_t = z(self.P), z(self.P, self.N, self.N), z(self.P, self.N, self.N)
        self.p_sigma_t, self.p_c_t = z(self.P, self.N), z(self.P, self.N)
        self.status_t = torch.zeros(self.P, dtype=torch.int32, device=dev)
        self.t_base_t = torch.zeros(1, dtype=torch.int64, device=dev)
        self._eye = torch.eye(self.N, dtype=torch.float64, device=dev).expand(self.P, self.N, self.N)
        self._weights = {}                                           # w as bytes -> (host array, device tensor)
        self.t = 0                                                   # updates since the last restart
        self.restart(0.3)

    def restart(self, init_sigma):
        self.sigma_t.fill_(float(init_sigma))
        self.cov_t.copy_(self._eye)
        self.chol_t.copy_(self._eye)
        self.p_sigma_t.zero_()
        self.p_c_t.zero_()
        self.t = 0

    def weights(self, w):
        """The weights on both sides of the call; a new vector allocates once (not inside a capture: call cma_update eagerly first)."""
        w = np.ascontiguousarray(w, dtype=np.float64)
        key = w.tobytes()
        if key not in self._weights:
            self._weights[key] = (w, self.s.torch.as_tensor(w, device=self.s.env.device))
        return self._weights[key]

    def sample(self, seed=0, draw_index=0):
        s, e = self.s, self.s.env
        if int(seed) < 0 or int(draw_index) < 0:
            raise ValueError("seed and draw_index must be >= 0")
        dst = s._cem.free()
        a = L.make_plan_args(L.PlanCmaSampleArgs, self.P, s.K, self.N, s.mean_t.data_ptr(), self.sigma_t.data_ptr(), self.chol_t.data_ptr(),
                             int(seed) & (2 ** 64 - 1), int(draw_index) & (2 ** 64 - 1), s.plan.draw_base_t.data_ptr(),
                             s._cem.blocks[dst].data_ptr())
        L.check(e._lib.glgym_plan_cma_sample(e._h, C.byref(a), e._stream()), "glgym_plan_cma_sample")
        return s._cem.occupy(dst)

    @staticmethod
    def check_hyper(N, E, hp, min_sigma, max_sigma):
        """ValueError with the meaning of glgym_plan_cma_update's refusal; -> the weights as a float64 array."""
        inf = float("inf")
        w = np.asarray(hp["w"], dtype=np.float64).reshape(-1)
        if w.size != E:
            raise ValueError(f"w must hold n_elite = {E} weights, got {w.size}")
        if not np.isfinite(w).all() or (w < 0).any():
            raise ValueError("the weights must be finite and >= 0")
        for k in L.CMA_CONSTANTS:
            if not -inf < float(hp[k]) < inf:
                raise ValueError(f"{k} must be finite")
        for k in ("c_sigma", "c_c", "c_1", "c_mu"):
            if not 0.0 <= float(hp[k]) <= 1.0:
                raise ValueError(f"{k} must lie in [0, 1]")
        if float(hp["c_1"]) + float(hp["c_mu"]) > 1.0:
            raise ValueError("c_1 + c_mu must not exceed 1")
        for k in ("d_sigma", "chi_n", "mu_eff"):
            if not float(hp[k]) > 0.0:
                raise ValueError(f"{k} must be > 0")
        if not 0.0 <= float(min_sigma) <= float(max_sigma) < inf:
            raise ValueError("min_sigma and max_sigma must be finite with 0 <= min_sigma <= max_sigma")
        return w

    def update(self, E, hp, min_sigma, max_sigma):
        s, e = self.s, self.s.env
        w = self.check_hyper(self.N, E, hp, min_sigma, max_sigma)
        if s._theta is None or s._cem.ranked is None or s._cem.ranked[0] != E:
            raise ValueError("cma_update needs a rollout and its elites()")
        w_host, w_dev = self.weights(w)
        a = L.make_plan_args(L.PlanCmaUpdateArgs, self.P, s.K, self.N, E, s._theta.data_ptr(), s.elite_k_t.data_ptr(), s.n_elite_t.data_ptr(),
                             w_host.ctypes.data, w_dev.data_ptr(), *(float(hp[k]) for k in L.CMA_CONSTANTS), float(min_sigma),
                             float(max_sigma), self.t + 1, self.t_base_t.data_ptr(), s.mean_t.data_ptr(), self.sigma_t.data_ptr(),
                             self.cov_t.data_ptr(), self.chol_t.data_ptr(), self.p_sigma_t.data_ptr(), self.p_c_t.data_ptr(),
                             self.status_t.data_ptr())
        L.check(e._lib.glgym_plan_cma_update(e._h, C.byref(a), e._stream()), "glgym_plan_cma_update")
        self.t += 1
        return self.status_t

    def run(self, n_iter, E, init_sigma, min_sigma, max_sigma, seed, mean, resume, overrides):
        s = self.s
        n_iter = int(n_iter)
        if n_iter < 1:
            raise ValueError("n_iter must be at least 1")
        if not 1 <= E <= s.K:
            raise ValueError(f"n_elite must be in 1 .. n_candidates = {s.K}")
        unknown = sorted(set(overrides) - {"w", *L.CMA_CONSTANTS})
        if unknown:
            raise TypeError(f"unexpected arguments {unknown}; the constants are w and {L.CMA_CONSTANTS}")
        hp = {**s.cma_defaults(self.N, s.K, E), **overrides}
        self.check_hyper(self.N, E, hp, min_sigma, max_sigma)
        if not 0.0 < float(init_sigma) < float("inf") or int(seed) < 0:
            raise ValueError("init_sigma must be finite and > 0, seed >= 0")
        if resume and mean is not None:
            raise ValueError("resume=True continues from mean_t and the CMA state: it takes no mean")
        if not resume:
            s._start(mean)
            self.restart(init_sigma)
        for _ in range(n_iter):
            block = self.sample(seed=seed, draw_index=s._draw)
            s._draw += 1
            s.rollout(block)
            s.elites(E)
            self.update(E, hp, min_sigma, max_sigma)
        sel = s.select()
        out = {"best_theta": sel["best_theta"], "best_params": sel["best_params"], "best_return": sel["best_return"], "best_k": sel["best_k"],
               "mean": s.mean_t, "sigma": self.sigma_t, "cov": self.cov_t, "status": self.status_t}
        if "best_feasible" in sel:                                   # a search with constraints
            out.update(best_feasible=sel["best_feasible"], n_feasible=sel["n_feasible"])
        return out


class _ThetaSearch:
    """What the searches over a feedback law's parameters share (RuleSearch, PolicySearch).  A candidate is a row of the float32 block
    theta [Ht, J, 6], Ht = ceil(D / 6), J = P*K: K candidates for each of P distribution rows [Ht, P, 6] (mean_t / std_t).  A Planner
    (self.plan) owns the children's buffers, the fork, the accumulators, the scenarios and the weather windows.  theta has the layout of
    an action block of horizon Ht, so the CEM stages are the library's, called with H = Ht and beta = 0 (_CemStages); _EsStages and,
    where a subclass offers it, _CmaStages sample into the same two population blocks.

    A subclass checks its own arguments (after _check_scenario_kwargs, before the environment is touched by this constructor), gives
    D, Ht and P, and writes rollout(): _take(theta_t), plan._fork_children(), its library call on plan._rollout_args() and
    plan._scenario_args(), then plan._results().  It may override _es_start (where a search starts without a mean), replace score_t /
    score_failed_t [P*K] (what elites, utilities and select rank: by default the plan's) and best_k_t / best_ret_t [P], and wrap cem /
    es with its own defaults."""

    SCENARIO_KEYS = ("n_scenarios", "n_tail", "noise", "noise_scale", "scenario_seed", "weather_sigma", "weather_phi")

    @classmethod
    def _check_scenario_kwargs(cls, scenario_kwargs):
        unknown = sorted(set(scenario_kwargs) - set(cls.SCENARIO_KEYS))
        if unknown:
            raise TypeError(f"unexpected arguments {unknown}; the scenario arguments are {cls.SCENARIO_KEYS}")

    def __init__(self, env, n_candidates, horizon, gamma, scenario_kwargs, D, Ht, P, constraints=None):
        self.plan = p = Planner(env, n_candidates, horizon, gamma=gamma, crop="nominal", **scenario_kwargs)
        self.constraints, self._con = constraints, None
        if constraints is not None:                                  # a group per greenhouse: the plan's own stage, behind its _results
            p._constrain(constraints)
            self._con = p._con
        self.env, self.torch = env, env.torch
        torch, dev = env.torch, env.device
        self.B, self.K, self.H, self.C, self.S = p.B, p.K, p.H, p.C, p.S
        self.D, self.Ht, self.P = int(D), int(Ht), int(P)            # P distributions: rows of mean / std, calls of the stages
        self.J = self.P * self.K                                     # rows of theta
        Ht, P = self.Ht, self.P
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        self._theta_buf = None
        self._theta = None                                           # the [Ht, J, 6] block of the last rollout
        self._cem = _CemStages(self, P, Ht, p.draw_base_t, f"ceil(D / 6) x {P} x 6")
        self.elite_k_t, self.n_elite_t = self._cem.alloc()
        self.mean_t, self.std_t = z(Ht, P, L.NU), z(Ht, P, L.NU)
        self.best_sequence_t = z(Ht, P, L.NU)
        self.best_theta_t = z(P, Ht * L.NU)
        self.score_t, self.score_failed_t = p._score_t, p._score_failed_t
        self.best_k_t, self.best_ret_t = p.best_k_t, p.best_ret_t
        self._draw = 0
        self._es_stages = None
        self.scenario_returns = getattr(p, "scenario_returns", None)
        self.scenario_failed = getattr(p, "scenario_failed", None)
        if self._con is not None:
            self.feasible, self.excess, self.n_violating, self.n_feasible = self._con.views(self.B)

    @staticmethod
    def _pop_constraints(scenario_kwargs):
        """constraints=... travels beside the scenario keywords, not among them (SCENARIO_KEYS): -> (it or None, the others)."""
        kw = dict(scenario_kwargs)
        return kw.pop("constraints", None), kw

    def _cem_alloc(self):
        """Nothing left to do: __init__ has allocated."""

    def _take(self, theta_t):
        """The front half of a rollout: theta_t as the block _theta -- a contiguous float32 tensor on the environment's device is read in
        place, anything else is staged -- and the population block it is, if one."""
        torch, e, p = self.torch, self.env, self.plan
        n = self.Ht * self.J * L.NU
        if theta_t.numel() != n:
            raise ValueError(f"theta_t must hold ceil(D / 6) x {self.J} x 6 = {n} values, got {tuple(theta_t.shape)}")
        if theta_t.dtype == torch.float32 and theta_t.is_cuda and theta_t.device == e.device and theta_t.is_contiguous():
            self._theta = theta_t.view(self.Ht, self.J, L.NU)
        else:
            if self._theta_buf is None:
                self._theta_buf = torch.zeros(self.Ht, self.J, L.NU, dtype=torch.float32, device=e.device)
            self._theta_buf.copy_(theta_t.reshape(self.Ht, self.J, L.NU))
            self._theta = self._theta_buf
        self._cem.note_rollout(theta_t)                              # one of the population blocks is always read in place
        p._actions = None                                            # the plan's own select / refit have nothing to read
        p._cem.note_rollout(None)

    def new_scenarios(self):
        """Planner.new_scenarios: other futures from the next scenario rollout on."""
        self.plan.new_scenarios()

    def _es_start(self):
        self.mean_t.zero_()

    def _start(self, mean):
        """Where cem(), es() and cma() start: `mean` [Ht, P, 6] or [Ht, 1, 6] copied into mean_t, without one _es_start()."""
        if mean is None:
            self._es_start()
            return
        if mean.numel() not in (self.Ht * L.NU, self.Ht * self.P * L.NU):
            raise ValueError(f"mean must hold ceil(D / 6) x (1 or {self.P}) x 6 values, got {tuple(mean.shape)}")
        self.mean_t.copy_(mean.reshape(self.Ht, -1, L.NU))

    # ---- the cross-entropy method over theta (_CemStages) ------------------------------------------------------------------------------
    def sample(self, mean_t, std_t, seed: int = 0, draw_index: int = 0, carry: int = 0):
        """glgym_plan_sample with H = Ht, beta = 0: the population theta [Ht, J, 6] from N(mean_t, std_t) [Ht, P, 6], clipped to
        [-1, 1], into the block the previous population does not occupy; returns it.  Candidate 0 is the clipped mean; with carry >= 1
        and elites() of the previous sampled population at hand, candidates 1 .. carry are its best rows."""
        return self._cem.sample(mean_t, std_t, 0.0, seed, draw_index, carry)

    def elites(self, n_elite: int):
        """glgym_plan_elites on the last rollout's scores: (elite_k [P, n_elite] i32, n_elite [P] i32), as Planner.elites."""
        return self._cem.elites(self.score_t, self.score_failed_t, n_elite)

    def refit(self, mean_t, std_t, alpha: float, min_std: float):
        """glgym_plan_refit with H = Ht, in place on mean_t / std_t [Ht, P, 6], over the elites() of the last rollout's theta."""
        return self._cem.refit(self._theta, mean_t, std_t, alpha, min_std)

    def select(self) -> Dict[str, Any]:
        """glgym_plan_select with H = Ht on the last rollout's scores: {"best_k" [P] i32 (-1: every candidate failed), "best_return"
        [P] f64, "best_theta" [P, Ht*6] f32 (component i at [., i]; zeros without an admissible candidate)}.  Device tensors,
        overwritten by the next call; no allocation.  With constraints best_return is the best constrained SCORE -- the return
        whenever best_feasible = 1 -- and the dict gains "best_feasible" [P] u8 (0 when best_k = -1) and "n_feasible" [P] i32."""
        if self._theta is None:
            raise ValueError("select needs a rollout")
        e = self.env
        a = L.make_plan_args(L.PlanSelectArgs, self.P, self.K, self.Ht, self.score_t.data_ptr(), self.score_failed_t.data_ptr(),
                             self._theta.data_ptr(), self.best_k_t.data_ptr(), self.best_ret_t.data_ptr(), None,
                             self.best_sequence_t.data_ptr(), 0.0, None)
        L.check(e._lib.glgym_plan_select(e._h, C.byref(a), e._stream()), "glgym_plan_select")
        self.best_theta_t.view(self.P, self.Ht, L.NU).copy_(self.best_sequence_t.permute(1, 0, 2))
        out = {"best_k": self.best_k_t, "best_return": self.best_ret_t, "best_theta": self.best_theta_t}
        if self._con is not None:                                    # as Planner.select: best_return is the best score
            self._con.best(self.best_k_t, out)
        return out

    def _cem_search(self, n_iter, n_elite, init_std, min_std, alpha, carry, seed, mean):
        """cem() of the subclasses: what select() returns, and mean, std, elite_k, n_elite."""
        st = self._cem
        n_iter, E, carry = st.check_hyper(n_iter, n_elite, carry, init_std, min_std, alpha, 0.0, seed)
        self._start(mean)
        self.std_t.fill_(float(init_std))
        st.ranked = None                                             # nothing is carried into the first population
        elite_k, n_el = st.run(self.mean_t, self.std_t, n_iter, E, alpha, min_std, 0.0, carry, seed)
        out = dict(self.select())
        out.update(mean=self.mean_t, std=self.std_t, elite_k=elite_k, n_elite=n_el)
        return out

    # ---- the evolution strategy over theta (_EsStages) -------------------------------------------------------------------------------
    def _es(self):
        if self._es_stages is None:
            self._es_stages = _EsStages(self)
        return self._es_stages

    @property
    def es_t_base(self):
        """The device word added to every es_update step count (int64 [1])."""
        return self._es().t_base_t

    def sample_mirrored(self, mean_t, std_t, seed: int = 0, draw_index: int = 0):
        """glgym_plan_es_sample with H = Ht: the population theta in mirrored pairs (rows 2m and 2m + 1 of a distribution row:
        clip(mean + std e) and clip(mean - std e)), into the block the previous population does not occupy; returns it.  No reserved
        candidate.  ValueError if n_candidates is odd."""
        return self._es().sample_mirrored(mean_t, std_t, seed, draw_index)

    def utilities(self):
        """glgym_plan_es_utilities on the last rollout's scores: (u [P, K] f64 -- centred ranks 0.5 .. -0.5 over the admissible
        candidates, -0.5 for the others, all 0 with fewer than two -- and n_adm [P] i32)."""
        return self._es().utilities()

    def es_update(self, mean_t, std_t, lr, lr_std=0.0, std_decay=1.0, *, min_std, max_std=1.0, optimizer="adam", betas=(0.9, 0.999), eps=1e-8):
        """glgym_plan_es_update with H = Ht, in place on mean_t / std_t, over the utilities() of the last rollout's theta.  The Adam
        moments and the step count are this object's (es() restarts them)."""
        return self._es().update(mean_t, std_t, lr, lr_std, std_decay, min_std=min_std, max_std=max_std, optimizer=optimizer, betas=betas,
                                 eps=eps)


class RuleSearch(_ThetaSearch):
    """Closed-loop rollouts of the rule-based controller, and the tuning of its constants by the cross-entropy method, on the device
    (TomatoVecEnv.rule_search).  A candidate is not a control sequence but a FEEDBACK LAW: a row of K per greenhouse of the float32 block
    theta [Ht, B*K, 6], Ht = ceil(D / 6), which decodes to the D tuned constants (RuleParams; the others come from `base`).  rollout()
    forks the environment's greenhouses into B*K children (x S scenarios) and runs controller -> env-step -> accumulate for `horizon`
    steps in one library call (glgym_plan_rollout_rule): the control of step h is computed from the child's own state after step h-1.

    A Planner (self.plan) owns the children's buffers, the fork, the accumulators, the scenarios and the weather windows; n_scenarios,
    n_tail, noise, noise_scale, scenario_seed, weather_sigma and weather_phi are its.  theta has the layout of an action block of
    horizon Ht, so sample / elites / refit / select are the Planner's library stages called with H = Ht (no correlation along "the
    horizon": beta = 0).

    Limits.  dt must be a multiple of 450 s (check_rule_dt): the children's clocks are derived by the product form.  The steps are
    raw-control steps: under the default verify mode "auto" they run verified (TomatoVecEnv.set_verify).  The environment is only read."""

    def __init__(self, env, n_candidates: int, horizon: int, tune, base=None, gamma: float = 1.0, **scenario_kwargs):
        constraints, scenario_kwargs = self._pop_constraints(scenario_kwargs)
        self._check_scenario_kwargs(scenario_kwargs)
        check_rule_dt(env.dt)
        self.params = RuleParams(tune, base)
        self.base = self.params.base
        super().__init__(env, n_candidates, horizon, gamma, scenario_kwargs, self.params.D, self.params.Ht, env.B, constraints)
        torch, dev, B = env.torch, env.device, self.B
        self.names = self.params.names
        self._space = self.params.struct()
        self._lo_t = torch.as_tensor(self.params.lo, device=dev).view(self.D, 1)
        self._span_t = torch.as_tensor(self.params.hi - self.params.lo, device=dev).view(self.D, 1)
        self._plane_T = torch.zeros(1, L.NU, self.plan.ld, dtype=env.tdtype, device=dev)   # the one control plane of record=False
        self.controls_T = self.controls = None                       # record=True: [H, 6, ld] and its [H, C, 6] view
        self._dec_t = torch.zeros(B, self.Ht * L.NU, dtype=torch.float64, device=dev)
        self._params_T = torch.zeros(self.D, B, dtype=torch.float64, device=dev)
        self.best_params = {n: self._params_T[i] for i, n in enumerate(self.names)}
        self._base_theta = torch.as_tensor(self.params.encode(self.base), device=dev) if self.params.inside(self.base) else None
        self._cma_stages = None

    # ------------------------------------------------------------------------------------------------
    def encode(self, controller_or_dict):
        """theta [Ht, 1, 6] f32 on the environment's device of a RuleBasedController (or a dict of constants; missing names come from
        base): the tuned constants mapped into [-1, 1], padding 0.  ValueError outside the bounds."""
        return self.torch.as_tensor(self.params.encode(controller_or_dict), device=self.env.device)

    def decode(self, theta_t):
        """theta_t [Ht, n, 6] -> {name: float64 [n]} on theta_t's device, by the formula of include/glgym.h (a NaN reads as lo)."""
        torch = self.torch
        th = theta_t.reshape(self.Ht, -1, L.NU)
        t = th.permute(1, 0, 2).reshape(th.shape[1], self.Ht * L.NU)[:, :self.D].double()
        t = torch.nan_to_num(t, nan=-1.0).clamp(-1.0, 1.0)
        lo, span = self._lo_t.view(-1).to(t.device), self._span_t.view(-1).to(t.device)
        v = lo + span * (0.5 * (t + 1.0))
        return {n: v[:, i] for i, n in enumerate(self.names)}

    def theta_of(self, controller_or_dict):
        """The block [Ht, B*K, 6] in which every candidate is that controller."""
        return self.encode(controller_or_dict).expand(self.Ht, self.J, L.NU).contiguous()

    def rollout(self, theta_t, record: bool = False):
        """Fork from the environment's current state and run the closed-loop rollout of every candidate controller.  theta_t holds
        [Ht, B*K, 6] f32 values (row b*K + k: candidate k of greenhouse b); a contiguous float32 tensor on the environment's device is
        read in place.  Returns what Planner.rollout returns: returns, alive, steps, violations, failed -- with scenarios the aggregated
        ones, scenario_returns / scenario_failed [B, K, S] holding the single runs.  record=True keeps the controls of every step:
        controls_T [H, 6, ld] and controls, its [H, C, 6] view (child c = (b*K + k)*S + s)."""
        torch, e, p = self.torch, self.env, self.plan
        self._take(theta_t)
        if record and self.controls_T is None:
            self.controls_T = torch.zeros(self.H, L.NU, p.ld, dtype=e.tdtype, device=e.device)
            self.controls = self.controls_T[:, :, :self.C].permute(0, 2, 1)
        planes = self.controls_T if record else self._plane_T
        p._fork_children()
        r = L.make_plan_args(L.PlanRolloutRuleArgs, 1 if record else 0, p._rollout_args(None, planes.data_ptr()), self._space,
                             self._theta.data_ptr(), p.start_day_t.data_ptr(), self.J, *p._scenario_args())
        L.check(e._lib.glgym_plan_rollout_rule(e._h, C.byref(r), e._stream()), "glgym_plan_rollout_rule")
        return p._results()

    def select(self) -> Dict[str, Any]:
        """glgym_plan_select with H = Ht on the last rollout: {"best_k" [B] i32 (-1: every candidate failed), "best_return" [B] f64,
        "best_theta" [B, Ht*6] f32 (component i of greenhouse b at [b, i]; zeros without an admissible candidate), "best_params"
        {name: [B] f64}}.  Device tensors, overwritten by the next call; no allocation."""
        out = super().select()
        # the header's decode with in-place operations: t = clamp, half = 0.5 * (t + 1), v = lo + span * half
        d = self._dec_t
        d.copy_(self.best_theta_t)
        d.nan_to_num_(nan=-1.0).clamp_(-1.0, 1.0).add_(1.0).mul_(0.5)
        self.torch.mul(d[:, :self.D].t(), self._span_t, out=self._params_T)
        self._params_T.add_(self._lo_t)
        out["best_params"] = self.best_params
        return out

    def cem(self, n_iter: int, n_elite: int, init_std: float = 0.5, min_std: float = 0.05, alpha: float = 0.1, carry: int = 0,
            seed: int = 0, mean=None) -> Dict[str, Any]:
        """Tune the controller: n_iter x (sample -> rollout -> elites -> refit), then select() on the last population.  mean None:
        start from encode(base) where base lies inside the bounds, else from 0 (the middle of every interval); otherwise from `mean`
        [Ht, B, 6] or [Ht, 1, 6].  The spread starts at init_std (theta units: the half-width of an interval is 1).  carry <= n_elite
        elites survive from one population into the next; nothing is carried into the first.  Every sample() takes the next draw index
        of this object's lifetime.
        Returns device tensors, overwritten by the next call: best_theta [B, Ht*6], best_params {name: [B]}, best_return, best_k,
        mean, std [Ht, B, 6], elite_k [B, n_elite], n_elite [B].  No host synchronisation and, after the first call, no allocation: a
        whole cem() can be captured in a graph (add n_iter to plan.draw_base_t between replays for fresh noise)."""
        return self._cem_search(n_iter, n_elite, init_std, min_std, alpha, carry, seed, mean)

    def _es_start(self):
        if self._base_theta is not None:
            self.mean_t.copy_(self._base_theta)
        else:
            self.mean_t.zero_()

    def es(self, n_iter: int, lr: float, lr_std: float = 0.1, init_std: float = 0.3, min_std: float = 0.02, max_std: float = 1.0,
           std_decay: float = 1.0, optimizer: str = "adam", betas=(0.9, 0.999), eps: float = 1e-8, seed: int = 0, mean=None,
           resume: bool = False) -> Dict[str, Any]:
        return self._es().run(n_iter, lr, lr_std, init_std, min_std, max_std, std_decay, optimizer, betas, eps, seed, mean, resume)

    es.__doc__ = _ES_DOC

    # ---- CMA-ES with a full covariance matrix over theta (_CmaStages) -----------------------------------------------------------------
    def _cma(self):
        if self._cma_stages is None:
            self._cma_stages = _CmaStages(self)
        return self._cma_stages

    @staticmethod
    def cma_defaults(N: int, K: int, E: int) -> Dict[str, Any]:
        """Hansen's default constants for N components, K candidates and E elites: {"w": float64 [E], w_i ~ ln(E + 1/2) - ln i,
        normalised; "mu_eff" = 1 / sum w^2; "c_sigma", "d_sigma", "c_c", "c_1", "c_mu", "chi_n"}."""
        N, K, E = int(N), int(K), int(E)
        if N < 1 or not 1 <= E <= K:
            raise ValueError("cma_defaults needs N >= 1 and 1 <= E <= K")
        w = np.log(E + 0.5) - np.log(np.arange(1, E + 1, dtype=np.float64))
        w = w / w.sum()
        mu = 1.0 / float(np.sum(w * w))
        c_sigma = (mu + 2.0) / (N + mu + 5.0)
        c_1 = 2.0 / ((N + 1.3) ** 2 + mu)
        return {"w": w, "mu_eff": mu, "c_sigma": c_sigma,
                "d_sigma": 1.0 + 2.0 * max(0.0, float(np.sqrt((mu - 1.0) / (N + 1.0))) - 1.0) + c_sigma,
                "c_c": (4.0 + mu / N) / (N + 4.0 + 2.0 * mu / N), "c_1": c_1,
                "c_mu": min(1.0 - c_1, 2.0 * (mu - 2.0 + 1.0 / mu) / ((N + 2.0) ** 2 + mu)),
                "chi_n": float(np.sqrt(N)) * (1.0 - 1.0 / (4.0 * N) + 1.0 / (21.0 * N * N))}

    @property
    def cma_t_base(self):
        """The device word added to every cma_update generation count (int64 [1])."""
        return self._cma().t_base_t

    @property
    def cma_state(self) -> Dict[str, Any]:
        """The CMA state next to mean_t, device tensors updated in place: sigma [B], cov, chol [B, D, D], p_sigma, p_c [B, D] f64,
        status [B] i32 (of the last cma_update: 0 updated, 1 too few elites, 2 not finite, 3 not positive definite, 4 t = 0)."""
        st = self._cma()
        return {"sigma": st.sigma_t, "cov": st.cov_t, "chol": st.chol_t, "p_sigma": st.p_sigma_t, "p_c": st.p_c_t, "status": st.status_t}

    def sample_cma(self, seed: int = 0, draw_index: int = 0):
        """glgym_plan_cma_sample: the population theta = clip(mean_t + sigma * chol z) from this object's mean_t and CMA state, into the
        block the previous population does not occupy; returns it.  No reserved candidate.  ValueError with more than 32 constants."""
        return self._cma().sample(seed, draw_index)

    def cma_update(self, n_elite: Optional[int] = None, min_sigma: float = 1e-6, max_sigma: float = 1.0, **overrides):
        """elites(n_elite) of the last rollout, then glgym_plan_cma_update in place on mean_t and the CMA state; returns status [B] i32.
        n_elite defaults to K // 2; the constants are cma_defaults(D, K, n_elite) unless overridden by name."""
        E = max(1, self.K // 2) if n_elite is None else int(n_elite)
        st = self._cma()
        unknown = sorted(set(overrides) - {"w", *L.CMA_CONSTANTS})
        if unknown:
            raise TypeError(f"unexpected arguments {unknown}; the constants are w and {L.CMA_CONSTANTS}")
        if self._theta is None:
            raise ValueError("cma_update needs a rollout")
        self.elites(E)
        return st.update(E, {**self.cma_defaults(self.D, self.K, E), **overrides}, min_sigma, max_sigma)

    def cma(self, n_iter: int, n_elite: Optional[int] = None, init_sigma: float = 0.3, min_sigma: float = 1e-6, max_sigma: float = 1.0,
            seed: int = 0, mean=None, resume: bool = False, **overrides) -> Dict[str, Any]:
        """Tune the controller by CMA-ES with a full covariance matrix: n_iter x (sample_cma -> rollout -> elites -> cma_update), then
        select() on the last population.  For the few, strongly interacting constants this class tunes (at most 32): the search
        distribution of greenhouse b is N(mean, sigma^2 C) with a D x D matrix C, adapted by the rank-one and rank-mu updates, and a
        step size sigma under cumulative step-size control.  The start is cem()'s: `mean`, or this object's default; sigma starts at
        init_sigma, C at I.  n_elite defaults to K // 2; the constants are cma_defaults(D, K, n_elite) unless overridden by name (w,
        mu_eff, c_sigma, d_sigma, c_c, c_1, c_mu, chi_n).  resume=True continues instead from mean_t, the CMA state and the
        generation count of the previous call.  Every sample takes the next draw index of this object's lifetime.
        Returns device tensors, overwritten by the next call: best_theta [B, Ht*6], best_params {name: [B]}, best_return, best_k, mean
        [Ht, B, 6], sigma [B], cov [B, D, D] f64, status [B] i32 of the last update (0: updated; otherwise the row kept its state).
        No host synchronisation and, after the first call, no allocation: a whole cma() can be captured in a graph; between replays
        add n_iter to plan.draw_base_t for fresh noise and, with resume=True, to cma_t_base for the next generation counts."""
        E = max(1, self.K // 2) if n_elite is None else int(n_elite)
        return self._cma().run(n_iter, E, init_sigma, min_sigma, max_sigma, seed, mean, resume, overrides)

    def best_controller(self, b: int = 0):
        """The RuleBasedController of greenhouse b's best candidate of the last select() / cem(): base with the tuned constants
        replaced.  Synchronises (reads the device)."""
        from .baseline import RULE_BASED_DEFAULTS, RuleBasedController
        if not 0 <= int(b) < self.B:
            raise ValueError(f"b must be in 0 .. {self.B - 1}")
        cfg = {n: getattr(self.base, n) for n in RULE_BASED_DEFAULTS}
        vals = self._params_T[:, int(b)].cpu().numpy()
        cfg.update({n: float(vals[i]) for i, n in enumerate(self.names)})
        return RuleBasedController(**cfg)


# ---- closed-loop neural-policy rollouts and policy search (include/glgym.h glgym_policy_rows / glgym_plan_rollout_policy) -----------
class MLPSpec:
    """The shape of an MLP policy on the host -- include/glgym.h glgym_mlp_net: in_dim observations -> hidden layers of the widths in
    `hidden` (at most 3 of at most 64 neurons; () is a linear policy) -> 6 actions.  activation "relu" | "tanh" | "silu" on the hidden
    layers, squash "clip" | "tanh" on the outputs (both end in a clip to [-1, 1]).  scale: the value of a parameter is scale[g] *
    theta, g = 2 l for the weights of layer l and 2 l + 1 for its biases; one number for all groups or a list of 2 (len(hidden) + 1).
    With scale 1 a trained net loads exactly; with theta sampled in [-1, 1] the scale is the search bound.  obs_norm: None, a
    VecNormalizeGPU, or (mean, var, epsilon, clip_obs): the input is clip((obs - mean) * inv_std, -clip_obs, clip_obs) with inv_std =
    1 / sqrt(var + epsilon) computed in double and rounded once to float32.

    The flat parameter vector has D components, layer by layer the weight [out, in] row-major, then the bias [out] -- the order of
    torch.nn.utils.parameters_to_vector on nn.Sequential(Linear, act, ..., Linear); a block theta is float32 [Ht, J, 6], Ht =
    ceil(D / 6), component i of row j at theta[i // 6, j, i % 6]."""

    def __init__(self, in_dim: int, hidden=(), activation: str = "tanh", squash: str = "clip", scale=1.0, obs_norm=None):
        import numpy as np
        self.np = np
        self.in_dim, self.hidden = int(in_dim), tuple(int(w) for w in hidden)
        if not 1 <= self.in_dim <= L.MLP_MAX_IN:
            raise ValueError(f"in_dim must be in 1 .. {L.MLP_MAX_IN}")
        if len(self.hidden) > L.MLP_MAX_HIDDEN or any(not 1 <= w <= L.MLP_MAX_WIDTH for w in self.hidden):
            raise ValueError(f"hidden: at most {L.MLP_MAX_HIDDEN} layers of 1 .. {L.MLP_MAX_WIDTH} neurons")
        if activation not in L.MLP_ACTIVATIONS:
            raise ValueError(f"activation must be one of {tuple(L.MLP_ACTIVATIONS)}")
        if squash not in L.MLP_SQUASHES:
            raise ValueError(f"squash must be one of {tuple(L.MLP_SQUASHES)}")
        self.activation, self.squash = activation, squash
        sizes = (self.in_dim,) + self.hidden + (L.NU,)
        self.shapes = [(sizes[l + 1], sizes[l]) for l in range(len(sizes) - 1)]          # (out, in) per layer
        self.n_groups = 2 * len(self.shapes)
        try:
            sc = [float(scale)] * self.n_groups
        except TypeError:
            sc = [float(v) for v in scale]
        self.scale = np.asarray(sc, dtype=np.float32)
        if len(sc) != self.n_groups or not (np.isfinite(self.scale).all() and (self.scale > 0).all()):
            raise ValueError(f"scale must be one number or {self.n_groups} numbers (weights, biases per layer), finite and > 0")
        self.D = sum(o * (i + 1) for o, i in self.shapes)
        self.Ht = (self.D + L.NU - 1) // L.NU
        if self.Ht > L.MLP_MAX_HT:
            raise ValueError(f"the net has {self.D} parameters: more than {L.MLP_MAX_HT} planes of 6")
        self.mean = self.inv_std = None
        self.clip_obs = 10.0
        if obs_norm is not None:
            if hasattr(obs_norm, "obs_mean"):
                mean, var = obs_norm.obs_mean.detach().cpu().numpy(), obs_norm.obs_var.detach().cpu().numpy()
                eps, clip = obs_norm.epsilon, obs_norm.clip_obs
            else:
                mean, var, eps, clip = obs_norm
            mean, var = np.asarray(mean, dtype=np.float64).reshape(-1), np.asarray(var, dtype=np.float64).reshape(-1)
            if mean.shape != (self.in_dim,) or var.shape != (self.in_dim,):
                raise ValueError(f"obs_norm: mean and var must hold in_dim = {self.in_dim} values")
            self.mean = mean.astype(np.float32)
            with np.errstate(invalid="ignore", divide="ignore"):             # a bad variance is refused below, not warned about
                self.inv_std = (1.0 / np.sqrt(var + float(eps))).astype(np.float32)
            self.clip_obs = float(np.float32(clip))
            if not (np.isfinite(self.mean).all() and np.isfinite(self.inv_std).all()):
                raise ValueError("obs_norm: mean and 1 / sqrt(var + epsilon) must be finite")
            if not 0.0 < self.clip_obs < float("inf"):
                raise ValueError("obs_norm: clip_obs must be finite and > 0")

    def struct(self, mean_ptr=None, inv_std_ptr=None):
        """The glgym_mlp_net; mean_ptr / inv_std_ptr: device pointers of float32 [in_dim] copies of self.mean / self.inv_std."""
        n = L.MlpNet()
        n.in_dim, n.n_hidden, n.activation, n.squash = self.in_dim, len(self.hidden), L.MLP_ACTIVATIONS[self.activation], L.MLP_SQUASHES[self.squash]
        for l, w in enumerate(self.hidden):
            n.width[l] = w
        for g in range(8):
            n.scale[g] = float(self.scale[g]) if g < self.n_groups else 1.0
        n.clip_obs, n.mean, n.inv_std = self.clip_obs, mean_ptr, inv_std_ptr
        return n

    def _layers(self, src):
        """[(W, b)] as float64 arrays from an nn.Sequential of Linear / activation layers, an SB3-style state dict or a list of (W, b)."""
        np = self.np
        to_np = lambda t: np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64)  # noqa: E731
        if isinstance(src, dict):
            n_h, layers = len(self.hidden), []
            for l in range(n_h):
                layers.append((src[f"mlp_extractor.policy_net.{2 * l}.weight"], src[f"mlp_extractor.policy_net.{2 * l}.bias"]))
            layers.append((src["action_net.weight"], src["action_net.bias"]))
            if f"mlp_extractor.policy_net.{2 * n_h}.weight" in src:
                raise ValueError("the state dict has more policy layers than the spec")
        elif hasattr(src, "children"):
            layers = [(m.weight, m.bias) for m in src.children() if hasattr(m, "weight")]
        else:
            layers = list(src)
        if len(layers) != len(self.shapes):
            raise ValueError(f"{len(layers)} linear layers given, the spec has {len(self.shapes)}")
        out = []
        for l, ((W, b), (o, i)) in enumerate(zip(layers, self.shapes)):
            if b is None:
                raise ValueError(f"layer {l} has no bias")
            W, b = to_np(W), to_np(b)
            if W.shape != (o, i) or b.shape != (o,):
                raise ValueError(f"layer {l}: weight {W.shape} / bias {b.shape}, the spec has ({o}, {i}) / ({o},)")
            out.append((W, b))
        return out

    def encode(self, module_or_arrays):
        """-> theta float32 [Ht, 1, 6]: the parameters divided by their group's scale (in double, rounded once), padding 0.  Takes a
        torch nn.Sequential of Linear / activation layers, an SB3-style state dict (mlp_extractor.policy_net.{2l}.weight | bias,
        action_net.weight | bias) or a list of (W, b); ValueError where a shape differs from the spec."""
        np = self.np
        flat = np.zeros(self.Ht * L.NU, dtype=np.float32)
        at = 0
        for l, (W, b) in enumerate(self._layers(module_or_arrays)):
            for g, v in ((2 * l, W.reshape(-1)), (2 * l + 1, b)):
                flat[at:at + v.size] = (v / np.float64(self.scale[g])).astype(np.float32)
                at += v.size
        return flat.reshape(self.Ht, 1, L.NU)

    def flat(self, theta):
        """theta [Ht, J, 6] -> [J, D] float32: component i of row j at [j, i]."""
        np = self.np
        th = np.asarray(theta, dtype=np.float32).reshape(self.Ht, -1, L.NU)
        return np.ascontiguousarray(th.transpose(1, 0, 2)).reshape(th.shape[1], self.Ht * L.NU)[:, :self.D]

    def decode(self, theta):
        """theta [Ht, J, 6] -> [(W [J, out, in], b [J, out])] float32, every parameter scale[g] * theta in float32."""
        flat, out, at = self.flat(theta), [], 0
        for l, (o, i) in enumerate(self.shapes):
            W = (self.scale[2 * l] * flat[:, at:at + o * i]).reshape(-1, o, i)
            at += o * i
            b = self.scale[2 * l + 1] * flat[:, at:at + o]
            at += o
            out.append((W, b))
        return out


class PolicySearch(_ThetaSearch):
    """Closed-loop rollouts of MLP policies and gradient-free policy search by the cross-entropy method on the device
    (TomatoVecEnv.policy_search).  A candidate is a FEEDBACK LAW: a row of the float32 block theta [Ht, J, 6] holding the D parameters
    of an MLPSpec net.  rollout() forks the environment's greenhouses into B*K children (x S scenarios) and runs observation -> policy
    -> env-step -> accumulate for `horizon` steps in one library call (glgym_plan_rollout_policy): the action of step h is computed from
    the child's own observation after step h-1, the observation the environment itself would return.

    share="greenhouse": every greenhouse has K candidates of its own (J = B*K rows, the distribution is [Ht, B, 6]), as RuleSearch.
    share="all": K policies, each run on all B greenhouses (J = K rows, the distribution is [Ht, 1, 6]); policy k's score is the
    float64 mean over the greenhouses of its (aggregated) returns, and it counts as failed if any of its children failed.

    A Planner (self.plan) owns the children's buffers, the fork, the accumulators and the scenarios; n_scenarios, n_tail, noise,
    noise_scale and scenario_seed are its.  theta has the layout of an action block of horizon Ht, so sample / elites / refit / select
    are the library's CEM stages called with H = Ht (beta = 0).

    Limits.  spec.in_dim must be the environment's observation width.  Weather windows (weather_sigma) are refused: a child on a private
    window keeps the parent's timestep, and the observation's current-row and forecast indices (w_off + timestep - 1 ...) would leave
    the window.  The steps are action steps (u <- clip(u + 0.1 a)); the environment is only read."""

    def __init__(self, env, n_candidates: int, horizon: int, spec: MLPSpec, share: str = "greenhouse", gamma: float = 1.0, **scenario_kwargs):
        constraints, scenario_kwargs = self._pop_constraints(scenario_kwargs)
        self._check_scenario_kwargs(scenario_kwargs)
        if scenario_kwargs.get("weather_sigma") is not None:
            raise ValueError("policy rollouts do not take weather_sigma: a child on a private weather window keeps the parent's timestep, and "
                             "the observation's current-row and forecast indices (w_off + timestep - 1 ...) would leave the window")
        if share not in ("greenhouse", "all"):
            raise ValueError("share must be 'greenhouse' or 'all'")
        if not isinstance(spec, MLPSpec):
            raise TypeError("spec must be an MLPSpec")
        if spec.in_dim != env.obs_dim:
            raise ValueError(f"spec.in_dim = {spec.in_dim}, the environment's observations have {env.obs_dim} columns")
        self.spec, self.share = spec, share
        # P distributions: every greenhouse's own, or one for all
        super().__init__(env, n_candidates, horizon, gamma, scenario_kwargs, spec.D, spec.Ht, env.B if share == "greenhouse" else 1,
                         constraints if share == "greenhouse" else None)
        torch, dev = env.torch, env.device
        self.row_mode = L.POLICY_ROW_CHILD if share == "greenhouse" else L.POLICY_ROW_CANDIDATE
        z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
        self._mean_t = torch.as_tensor(spec.mean, device=dev) if spec.mean is not None else None
        self._inv_std_t = torch.as_tensor(spec.inv_std, device=dev) if spec.inv_std is not None else None
        self._net = spec.struct(self._mean_t.data_ptr() if self._mean_t is not None else None,
                                self._inv_std_t.data_ptr() if self._inv_std_t is not None else None)
        self.obs_t = z(self.C, spec.in_dim)                          # the children's observations: the last step's afterwards
        self._plane_t = z(1, self.C, L.NU)                           # the one action plane of record=False
        self.actions = None                                          # record=True: [H, C, 6], child c = (b*K + k)*S + s
        self.best_k_t, self.best_ret_t = z(self.P, dtype=torch.int32), z(self.P, dtype=torch.float64)   # own ones: P may be 1
        if share == "all":
            self.score_t, self.score_failed_t = z(self.K, dtype=torch.float64), z(self.K, dtype=torch.uint8)
            self._mean_ret_t, self._any_failed_t = self.score_t, self.score_failed_t     # what rollout()'s two reductions write
            if constraints is not None:                              # one group of K policies, each run on the B greenhouses (x S)
                p, self.constraints = self.plan, constraints
                self._con = con = _ConstrainStage(env, constraints, 1, self.B, self.K, self.S or 1, p.ld, self._mean_ret_t, self._any_failed_t,
                                                  p.viol_T, p.n_steps_t)
                self.score_t, self.score_failed_t = con.score_con_t, con.failed_con_t
                self.feasible, self.excess, self.n_violating, self.n_feasible = con.views(1)

    # ------------------------------------------------------------------------------------------------
    def encode(self, module_or_arrays):
        """theta [Ht, 1, 6] f32 on the environment's device of a trained net (MLPSpec.encode)."""
        return self.torch.as_tensor(self.spec.encode(module_or_arrays), device=self.env.device)

    def rollout(self, theta_t, record: bool = False):
        """Fork from the environment's current state and run the closed-loop rollout of every candidate policy.  theta_t holds
        [Ht, J, 6] f32 values (share="greenhouse": row b*K + k is candidate k of greenhouse b; share="all": row k is policy k); a
        contiguous float32 tensor on the environment's device is read in place.  Returns what Planner.rollout returns -- returns,
        alive, steps, violations, failed, [B, K] per (greenhouse, candidate) in either share mode -- with scenarios the aggregated ones,
        scenario_returns / scenario_failed [B, K, S] holding the single runs.  With share="all" score_t / score_failed_t [K] hold the
        policies' scores afterwards.  record=True keeps the actions of every step: actions [H, C, 6] (child c = (b*K + k)*S + s)."""
        torch, e, p = self.torch, self.env, self.plan
        self._take(theta_t)
        if record and self.actions is None:
            self.actions = torch.zeros(self.H, self.C, L.NU, dtype=torch.float32, device=e.device)
        planes = self.actions if record else self._plane_t
        p._fork_children()                                           # never with weather windows: __init__ refuses weather_sigma
        r = L.make_plan_args(L.PlanRolloutPolicyArgs, 1 if record else 0, p._rollout_args(None, None), self._net, self._theta.data_ptr(),
                             p.start_day_t.data_ptr(), self.obs_t.data_ptr(), planes.data_ptr(), e.Np, self.row_mode, self.J,
                             *p._scenario_args())
        L.check(e._lib.glgym_plan_rollout_policy(e._h, C.byref(r), e._stream()), "glgym_plan_rollout_policy")
        out = p._results()
        if self.share == "all":
            torch.mean(out[0], dim=0, out=self._mean_ret_t)
            torch.amax(out[4], dim=0, out=self._any_failed_t)
            if self._con is not None:
                self._con.run()
        return out

    def evaluate(self, theta_row, record: bool = False):
        """Run ONE policy, theta_row [Ht, 1, 6] (Ht * 6 values), as every candidate of every greenhouse: with scenarios the evaluation
        of a trained policy under crop noise.  Returns what rollout() returns."""
        if theta_row.numel() != self.Ht * L.NU:
            raise ValueError(f"theta_row must hold ceil(D / 6) x 6 = {self.Ht * L.NU} values, got {tuple(theta_row.shape)}")
        row = theta_row.to(device=self.env.device, dtype=self.torch.float32).reshape(self.Ht, 1, L.NU)
        return self.rollout(row.expand(self.Ht, self.J, L.NU).contiguous(), record=record)

    def cem(self, n_iter: int, n_elite: int, init_std: float = 0.5, min_std: float = 0.02, alpha: float = 0.1, carry: int = 0,
            seed: int = 0, mean=None) -> Dict[str, Any]:
        """Policy search: n_iter x (sample -> rollout -> elites -> refit), then select() on the last population.  mean None: start
        from theta = 0 (the policy that holds the controls); otherwise from `mean` [Ht, P, 6] or [Ht, 1, 6] -- encode(net) for a warm
        start.  The spread starts at init_std (theta units: a parameter's bound is its scale).  carry <= n_elite elites survive from
        one population into the next; nothing is carried into the first.  Every sample() takes the next draw index of this object's
        lifetime.
        Returns device tensors, overwritten by the next call: best_theta [P, Ht*6], best_return, best_k [P], mean, std [Ht, P, 6],
        elite_k [P, n_elite], n_elite [P].  No host synchronisation and, after the first call, no allocation: a whole cem() can be
        captured in a graph (add n_iter to plan.draw_base_t between replays for fresh noise)."""
        return self._cem_search(n_iter, n_elite, init_std, min_std, alpha, carry, seed, mean)

    def es(self, n_iter: int, lr: float, lr_std: float = 0.1, init_std: float = 0.1, min_std: float = 0.01, max_std: float = 1.0,
           std_decay: float = 1.0, optimizer: str = "adam", betas=(0.9, 0.999), eps: float = 1e-8, seed: int = 0, mean=None,
           resume: bool = False) -> Dict[str, Any]:
        return self._es().run(n_iter, lr, lr_std, init_std, min_std, max_std, std_decay, optimizer, betas, eps, seed, mean, resume)

    es.__doc__ = _ES_DOC

    def best_theta(self, b: int = 0):
        """theta [Ht, 1, 6] of the best candidate of the last select() / cem(): greenhouse b's with share="greenhouse", the one best
        policy with share="all" (b is ignored).  A copy: pass it to evaluate(), or to MLPSpec.decode after .cpu()."""
        b = int(b) if self.share == "greenhouse" else 0
        if not 0 <= b < self.P:
            raise ValueError(f"b must be in 0 .. {self.P - 1}")
        return self.best_theta_t[b].clone().view(self.Ht, 1, L.NU)
