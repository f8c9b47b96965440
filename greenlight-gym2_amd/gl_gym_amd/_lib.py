"""ctypes binding of libglgym.so (include/glgym.h).  No CPU fallback: a missing library or a missing
HIP device raises -- the product path never routes through the oracle or any host implementation."""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("GLGYM_LIB", _HERE / "libglgym.so"))

NX, NU, ND, NP, NCROP, NINFO, NMETRIC = 28, 6, 10, 208, 34, 11, 14
METRIC_REPLICAS, METRIC_STRIDE = 64, 32          # glgym.h: the metric accumulators are replicated per cache line
F32, F64 = 0, 1
ODE, ODE_PIPE = 0, 1
SCHEME_RK4, SCHEME_RK2 = 0, 1
SCHEME_RK3 = 2
SCHEME_LS5 = 3
SCHEMES = {"rk4": SCHEME_RK4, "rk2": SCHEME_RK2, "rk3": SCHEME_RK3, "ls5": SCHEME_LS5}
ABI_VERSION = 7                                           # include/glgym.h GLGYM_ABI_VERSION
# integrator of glgym_evalF (include/glgym.h glgym_integrator): the explicit sub-steppers (default) or the adaptive variable-order BDF
INTEGRATORS = {"explicit": 0, "bdf": 1}
NSOLVER_STAT = 5                                          # glgym_get_solver_stats: steps, rhs evals, Jacobians, factorisations, order
SOLVER_STAT_KEYS = ("steps", "rhs_evals", "jacobians", "factorisations", "order")
LAYOUTS = {"auto": 0, "one": 1, "quad": 2}                # glgym_layout
# NOMINAL sub-steps per 900 s env-step.  RK4 (round 4): the conduction between the two faces of the cover glass -- the 0.65 1/s
# mode that kept every explicit scheme at >= 224 sub-steps -- is integrated exactly (gl_model.hpp rk_delta, COVEXP), so the nominal
# sub-step is set by the top compartment's air exchange: 240 covers rates up to 0.68 1/s (exceeded in 2e-5 of random-action
# env-steps on the synthetic weather year; median 0.19, 99.9 % 0.55).  The kernels are stability-controlled per environment: an
# environment whose rate bound at the start of the env-step asks for more gets proportionally more windows (its own sub-step
# length), and what changes inside the env-step is followed window by window.  "rk3" is the three-stage member of the same
# exponential family (stability interval 2.513: 270 covers 0.69 1/s), "rk2" its midpoint rule (2.0: 336 covers 0.69 1/s).
# "ls5" (round 5, the default): the five-stage fourth-order 2N-storage scheme (stability interval 5.009: 1.00 per right-hand side
# against RK4's 0.70; cover conduction exact as in the others): 128 covers 0.655 1/s, two sub-steps per window (14 s; RK4-240: 15 s)
# -- 640 right-hand sides per env-step for RK4-240's 960 at the same accuracy on every fixture.
DEFAULT_N_SUB = {"rk4": 240, "rk2": 336, "rk3": 270, "ls5": 128}
DEFAULT_SCHEME = "ls5"
VERIFY_MODES = {"auto": 0, "always": 1, "never": 2}     # glgym_verify (include/glgym.h)
N_SUB_MULTIPLE = {"rk4": 4, "rk2": 4, "rk3": 3, "ls5": 2}          # tier-2b window of the scheme
# PRESETS.  "throughput": the scheme's nominal count with its own window (max scaled error on the tight one-step tuples 5.4e-5 for
# ls5, 6.1e-5 for rk4, 10-day rollout 1.5e-5 fp64 / 2.9e-5 fp32; bar 1e-4).  "parity": inside the 1.3e-5 band a BDF solve at the reference's
# tolerances (greenlight_model.cpp:51-52) keeps from the tight solution -- ls5: n_sub 192 with ONE sub-step per window (1.0e-5), the
# others: n_sub x 8/3 with their own window (rk4 640: 8.7e-6).  (n_sub, window) at dt = 900 s; window 0 = the scheme's own.
PRESETS = {"throughput": {k: (v, 0) for k, v in DEFAULT_N_SUB.items()},
           "parity": {"ls5": (192, 1), "rk4": (640, 0), "rk3": (720, 0), "rk2": (896, 0)}}


def preset_n_sub(scheme: str, dt: float, preset: str = "throughput"):
    """-> (n_sub, window) of `preset` for `scheme`, n_sub scaled with dt so that the nominal sub-step h = dt / n_sub stays the same
    (e.g. ls5: 7.03 s, 44 sub-steps at the dt = 300 s of experiments/run_time.py) and rounded up to a multiple of the window."""
    n0, window = PRESETS[preset][scheme]
    n = n0 * float(dt) / 900.0
    mult = window if window > 0 else N_SUB_MULTIPLE[scheme]
    return max(mult, int(-(-n // mult) * mult)), window


def resolve_scheme(scheme, variant: str = "ode") -> str:
    """The scheme a constructor ends up with.  None = the default: "ls5" for the default ODE; "rk4" for variant "ode_pipe", whose
    kernels are instantiated for GLGYM_SCHEME_RK4 only (glgym_step / glgym_evalF return GLGYM_EINVAL for any other scheme with
    GLGYM_ODE_PIPE) -- so TomatoVecEnv(model_variant="ode_pipe") and GreenLight(variant="ode_pipe") work with default arguments.
    An explicit other scheme with ode_pipe is refused here, by name, instead of at the first step."""
    if variant not in ("ode", "ode_pipe"):
        raise ValueError("variant must be 'ode' or 'ode_pipe'")
    if scheme is None:
        return "rk4" if variant == "ode_pipe" else DEFAULT_SCHEME
    if scheme not in SCHEMES:
        raise ValueError("scheme must be 'ls5', 'rk4', 'rk3' or 'rk2'")
    if variant == "ode_pipe" and scheme != "rk4":
        raise ValueError(f"variant 'ode_pipe' is built for scheme 'rk4' only (got {scheme!r}): leave scheme unset or pass scheme='rk4'")
    return scheme


def default_n_sub(scheme: str, dt: float) -> int:
    """Nominal sub-steps per env-step of the throughput preset (see preset_n_sub)."""
    return preset_n_sub(scheme, dt, "throughput")[0]
OK, EINVAL, ENODEV, EHIP, ENOMEM, EODE = 0, -1, -2, -3, -4, -5

INFO_KEYS = ("EPI", "revenue", "variable_costs", "fixed_costs", "co2_cost", "heat_cost", "elec_cost",
             "temp_violation", "co2_violation", "rh_violation", "lamp_violation")      # tomato_env.py:208-222
METRIC_KEYS = ("sum_reward", "sum_EPI", "n_done", "n_ode_fail", "sum_co2_violation", "sum_temp_violation",
               "sum_rh_violation", "n_env_steps", "n_guard_retries", "n_refined_substeps", "n_flag_err", "n_flag_branch",
               "n_flag_cap", "n_flag_heavy")


class GlgymError(RuntimeError):
    pass


class GlgymOdeError(GlgymError):
    """glgym_evalF: the integration failed for at least one row (GLGYM_EODE) -- the counterpart of the RuntimeError the
    reference's evalF raises when CVODES fails (greenlight_model.cpp:110, caught at tomato_env.py:119-123)."""


class RewardCfg(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "elec_price", "heating_price", "co2_price", "fruit_price", "dmfm", "fixed_greenhouse_cost", "fixed_co2_cost",
        "fixed_lamp_cost", "fixed_screen_cost", "pen_lamp", "co2_min", "co2_max", "temp_min", "temp_max", "rh_min",
        "rh_max")]


class StepArgs(C.Structure):
    # struct_size first (since ABI 5): glgym_step refuses a struct of another size; make_step_args() fills it
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("ld", C.c_int32), ("x", C.c_void_p), ("u", C.c_void_p), ("action", C.c_void_p),
                ("control", C.c_void_p), ("weather", C.c_void_p), ("weather_rows", C.c_int32), ("w_off", C.c_void_p),
                ("timestep", C.c_void_p), ("crop_p", C.c_void_p), ("N", C.c_int32), ("reward", C.c_void_p),
                ("info", C.c_void_p), ("done", C.c_void_p), ("metrics", C.c_void_p), ("step_flags", C.c_void_p)]


def make_step_args(*args, **kw):
    """StepArgs(...) without the leading struct_size, which is filled in here."""
    return StepArgs(C.sizeof(StepArgs), *args, **kw)


# step_flags bits (include/glgym.h GLGYM_SF_*)
SF_FIRST_MASK, SF_ACCEPT_AGREE_FLAGGED, SF_ACCEPT_LAST_ALONE, SF_FAILED = 31, 32, 64, 128
SF_BDF = 2048                    # the env-step ran the BDF integrator; its steps are in bits 16..30
# metric slots of BDF env-steps (glgym.h GLGYM_METRIC_BDF): sums of steps, rhs evals, Jacobians, factorisations
METRIC_BDF = 14
BDF_METRIC_KEYS = ("bdf_steps", "bdf_rhs_evals", "bdf_jacobians", "bdf_factorisations")


class ObsArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("ld", C.c_int32), ("x", C.c_void_p), ("u", C.c_void_p), ("weather", C.c_void_p),
                ("weather_rows", C.c_int32), ("w_off", C.c_void_p), ("timestep", C.c_void_p), ("start_day", C.c_void_p),
                ("Np", C.c_int32), ("obs", C.c_void_p), ("mask", C.c_void_p), ("term_obs", C.c_void_p)]


class ResetArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("ld", C.c_int32), ("mask", C.c_void_p), ("x", C.c_void_p), ("u", C.c_void_p),
                ("timestep", C.c_void_p), ("weather", C.c_void_p), ("weather_rows", C.c_int32), ("w_off", C.c_void_p),
                ("start_rows", C.c_void_p), ("start_days", C.c_void_p), ("n_starts", C.c_int32),
                ("start_day", C.c_void_p), ("episode", C.c_void_p), ("seed", C.c_uint64)]


class VecNormArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("dim", C.c_int32), ("obs", C.c_void_p), ("obs_out", C.c_void_p),
                ("reward", C.c_void_p), ("reward_out", C.c_void_p), ("done", C.c_void_p), ("obs_mean", C.c_void_p),
                ("obs_var", C.c_void_p), ("obs_count", C.c_void_p), ("ret_stats", C.c_void_p), ("returns", C.c_void_p),
                ("workspace", C.c_void_p), ("gamma", C.c_double), ("epsilon", C.c_double), ("clip_obs", C.c_float),
                ("clip_reward", C.c_float), ("training", C.c_int32), ("norm_obs", C.c_int32),
                ("norm_reward", C.c_int32)]


# device-side planning (include/glgym.h glgym_plan_*): every struct starts with struct_size; make_plan_args() fills it
class PlanForkArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_children", C.c_int32), ("n_parents", C.c_int32), ("K", C.c_int32),
                ("ld_parent", C.c_int32), ("ld_child", C.c_int32), ("parent", C.c_void_p), ("x_parent", C.c_void_p),
                ("u_parent", C.c_void_p), ("timestep_parent", C.c_void_p), ("w_off_parent", C.c_void_p),
                ("start_day_parent", C.c_void_p), ("crop_parent", C.c_void_p), ("x", C.c_void_p), ("u", C.c_void_p),
                ("timestep", C.c_void_p), ("w_off", C.c_void_p), ("start_day", C.c_void_p), ("crop", C.c_void_p),
                ("ret", C.c_void_p), ("viol", C.c_void_p), ("n_steps", C.c_void_p), ("alive", C.c_void_p), ("failed", C.c_void_p)]


class PlanAccumulateArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("ld", C.c_int32), ("w", C.c_double), ("reward", C.c_void_p),
                ("info", C.c_void_p), ("done", C.c_void_p), ("step_flags", C.c_void_p), ("ret", C.c_void_p), ("viol", C.c_void_p),
                ("n_steps", C.c_void_p), ("alive", C.c_void_p), ("failed", C.c_void_p)]


class PlanRolloutArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("H", C.c_int32), ("gamma", C.c_double), ("step", StepArgs), ("actions", C.c_void_p),
                ("controls", C.c_void_p), ("ret", C.c_void_p), ("viol", C.c_void_p), ("n_steps", C.c_void_p), ("alive", C.c_void_p),
                ("failed", C.c_void_p)]


class PlanSelectArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("H", C.c_int32), ("ret", C.c_void_p),
                ("failed", C.c_void_p), ("actions", C.c_void_p), ("best_k", C.c_void_p), ("best_ret", C.c_void_p),
                ("best_action", C.c_void_p), ("best_sequence", C.c_void_p), ("temperature", C.c_double),
                ("mean_sequence", C.c_void_p)]


class PlanSampleArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("H", C.c_int32), ("mean", C.c_void_p),
                ("std", C.c_void_p), ("beta", C.c_double), ("seed", C.c_uint64), ("draw_index", C.c_uint64), ("draw_base", C.c_void_p),
                ("actions", C.c_void_p), ("carry", C.c_int32), ("prev_E", C.c_int32), ("prev_actions", C.c_void_p),
                ("prev_elite_k", C.c_void_p), ("prev_n_elite", C.c_void_p)]


class PlanElitesArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("E", C.c_int32), ("ret", C.c_void_p),
                ("failed", C.c_void_p), ("elite_k", C.c_void_p), ("n_elite", C.c_void_p)]


class PlanRefitArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("H", C.c_int32), ("E", C.c_int32),
                ("actions", C.c_void_p), ("elite_k", C.c_void_p), ("n_elite", C.c_void_p), ("alpha", C.c_double),
                ("min_std", C.c_double), ("mean", C.c_void_p), ("std", C.c_void_p), ("mean_out", C.c_void_p), ("std_out", C.c_void_p)]


# evolution strategy (include/glgym.h glgym_plan_es_sample / _es_utilities / _es_update)
ES_OPTIMIZERS = {"sgd": 0, "adam": 1}


class PlanEsSampleArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("H", C.c_int32), ("mean", C.c_void_p),
                ("std", C.c_void_p), ("seed", C.c_uint64), ("draw_index", C.c_uint64), ("draw_base", C.c_void_p),
                ("actions", C.c_void_p)]


class PlanEsUtilitiesArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("ret", C.c_void_p), ("failed", C.c_void_p),
                ("u", C.c_void_p), ("n_adm", C.c_void_p)]


class PlanEsUpdateArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("H", C.c_int32), ("optimizer", C.c_int32),
                ("actions", C.c_void_p), ("u", C.c_void_p), ("n_adm", C.c_void_p), ("lr", C.c_double), ("lr_std", C.c_double),
                ("std_decay", C.c_double), ("min_std", C.c_double), ("max_std", C.c_double), ("beta1", C.c_double),
                ("beta2", C.c_double), ("eps", C.c_double), ("t_index", C.c_uint64), ("t_base", C.c_void_p), ("m1", C.c_void_p),
                ("m2", C.c_void_p), ("mean", C.c_void_p), ("std", C.c_void_p), ("mean_out", C.c_void_p), ("std_out", C.c_void_p)]


# CMA-ES with a full covariance matrix (include/glgym.h glgym_plan_cma_sample / _cma_update)
CMA_NMAX = 32
CMA_CONSTANTS = ("mu_eff", "c_sigma", "d_sigma", "c_c", "c_1", "c_mu", "chi_n")
CMA_STATUS = {0: "updated", 1: "too few elites", 2: "not finite", 3: "not positive definite", 4: "t = 0"}


class PlanCmaSampleArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("N", C.c_int32), ("mean", C.c_void_p),
                ("sigma", C.c_void_p), ("chol", C.c_void_p), ("seed", C.c_uint64), ("draw_index", C.c_uint64), ("draw_base", C.c_void_p),
                ("theta", C.c_void_p)]


class PlanCmaUpdateArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("N", C.c_int32), ("E", C.c_int32),
                ("theta", C.c_void_p), ("elite_k", C.c_void_p), ("n_elite", C.c_void_p), ("w", C.c_void_p), ("w_dev", C.c_void_p),
                ("mu_eff", C.c_double), ("c_sigma", C.c_double), ("d_sigma", C.c_double), ("c_c", C.c_double), ("c_1", C.c_double),
                ("c_mu", C.c_double), ("chi_n", C.c_double), ("min_sigma", C.c_double), ("max_sigma", C.c_double),
                ("t_index", C.c_uint64), ("t_base", C.c_void_p), ("mean", C.c_void_p), ("sigma", C.c_void_p), ("cov", C.c_void_p),
                ("chol", C.c_void_p), ("p_sigma", C.c_void_p), ("p_c", C.c_void_p), ("status", C.c_void_p)]


# robust planning (include/glgym.h glgym_plan_scenario / _rollout_scenarios / _aggregate)
MAX_SCENARIOS = 256


class PlanScenarioArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("S", C.c_int32), ("ld", C.c_int32), ("h_step", C.c_int32),
                ("hold", C.c_int32), ("scale", C.c_double), ("seed", C.c_uint64), ("draw_index", C.c_uint64), ("draw_base", C.c_void_p),
                ("crop", C.c_void_p), ("actions_in", C.c_void_p), ("actions_out", C.c_void_p)]


class PlanRolloutScenariosArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("S", C.c_int32), ("hold", C.c_int32), ("scale", C.c_double),
                ("seed", C.c_uint64), ("draw_index", C.c_uint64), ("draw_base", C.c_void_p), ("staging", C.c_void_p),
                ("rollout", PlanRolloutArgs)]


class PlanAggregateArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("J", C.c_int32), ("S", C.c_int32), ("m", C.c_int32), ("ld", C.c_int32), ("ld_cand", C.c_int32),
                ("ret", C.c_void_p), ("failed", C.c_void_p), ("viol", C.c_void_p), ("n_steps", C.c_void_p), ("ret_cand", C.c_void_p),
                ("failed_cand", C.c_void_p), ("viol_cand", C.c_void_p), ("steps_cand", C.c_void_p)]


# constrained ranking (include/glgym.h glgym_plan_constrain)
CONSTRAIN_MODES = {"penalty": 0, "feasible_first": 1}


class PlanConstrainArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("O", C.c_int32), ("K", C.c_int32), ("S", C.c_int32), ("ld", C.c_int32),
                ("per_step", C.c_int32), ("n_allow", C.c_int32), ("mode", C.c_int32), ("budget", C.c_double * 3),
                ("weight", C.c_double * 3), ("rho", C.c_double), ("ret_cand", C.c_void_p), ("failed_cand", C.c_void_p),
                ("viol", C.c_void_p), ("n_steps", C.c_void_p), ("score", C.c_void_p), ("failed_out", C.c_void_p),
                ("feasible", C.c_void_p), ("excess", C.c_void_p), ("n_viol", C.c_void_p), ("n_feasible", C.c_void_p)]


# weather-forecast scenarios (include/glgym.h glgym_plan_weather)
WEATHER_COLUMNS = ("iGlob", "tOut", "vpOut", "co2Out", "wind", "tSky", "tSoOut")


class PlanWeatherArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("S", C.c_int32), ("H", C.c_int32), ("weather_rows", C.c_int32),
                ("weather", C.c_void_p), ("w_off_parent", C.c_void_p), ("timestep_parent", C.c_void_p), ("sigma", C.c_double * 7),
                ("phi", C.c_double), ("seed", C.c_uint64), ("draw_index", C.c_uint64), ("draw_base", C.c_void_p), ("window", C.c_void_p),
                ("w_off_child", C.c_void_p)]


def make_plan_args(cls, *args, **kw):
    """cls(...) of one of the Plan*Args structs without the leading struct_size, which is filled in here."""
    return cls(C.sizeof(cls), *args, **kw)


RULE_FIELDS = ("lamps_on", "lamps_off", "lamps_day_start", "lamps_day_stop", "lamps_off_sun", "lamp_rad_sum_limit",
               "temp_setpoint_day", "temp_setpoint_night", "heat_correction", "heat_deadzone", "co2_day",
               "vent_heat_Pband", "rh_max", "mech_dehumid_Pband", "vent_rh_Pband", "t_vent_off", "vent_cold_Pband",
               "thScrSpDay", "thScrSpNight", "thScrPband", "thScrDeadZone", "thScrRh", "thScrRhPband", "lampExtraHeat",
               "blScrExtraRh", "rhMax", "tHeatBand", "co2Band", "useBlScr")


class RuleCfg(C.Structure):
    _fields_ = [(n, C.c_double) for n in RULE_FIELDS]


class RuleArgs(C.Structure):
    _fields_ = [("B", C.c_int32), ("ld", C.c_int32), ("x", C.c_void_p), ("weather", C.c_void_p),
                ("weather_rows", C.c_int32), ("w_off", C.c_void_p), ("timestep", C.c_void_p), ("start_day", C.c_void_p),
                ("hour", C.c_void_p), ("doy", C.c_void_p), ("control", C.c_void_p)]


# closed-loop rule-based rollouts (include/glgym.h glgym_rule_rows / glgym_plan_rollout_rule)
RULE_BANDS = ("vent_heat_Pband", "vent_rh_Pband", "vent_cold_Pband", "thScrPband", "thScrRhPband", "tHeatBand", "co2Band")


class RuleSpace(C.Structure):
    _fields_ = [("base", RuleCfg), ("D", C.c_int32), ("field", C.c_int32 * 29), ("lo", C.c_double * 29), ("hi", C.c_double * 29)]


class RuleRowsArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("J", C.c_int32), ("S", C.c_int32), ("rule", RuleArgs), ("space", RuleSpace),
                ("theta", C.c_void_p)]


class PlanRolloutRuleArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("record", C.c_int32), ("rollout", PlanRolloutArgs), ("space", RuleSpace),
                ("theta", C.c_void_p), ("start_day", C.c_void_p), ("J", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("S", C.c_int32),
                ("hold", C.c_int32), ("scale", C.c_double), ("seed", C.c_uint64), ("draw_index", C.c_uint64), ("draw_base", C.c_void_p)]


# closed-loop neural-policy rollouts (include/glgym.h glgym_policy_rows / glgym_plan_rollout_policy)
MLP_ACTIVATIONS = {"relu": 0, "tanh": 1, "silu": 2}
MLP_SQUASHES = {"clip": 0, "tanh": 1}
MLP_MAX_HIDDEN, MLP_MAX_WIDTH, MLP_MAX_IN, MLP_MAX_HT = 3, 64, 1024, 65535
POLICY_ROW_CHILD, POLICY_ROW_CANDIDATE = 0, 1


class MlpNet(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("n_hidden", C.c_int32), ("width", C.c_int32 * 3), ("activation", C.c_int32), ("squash", C.c_int32),
                ("scale", C.c_float * 8), ("clip_obs", C.c_float), ("mean", C.c_void_p), ("inv_std", C.c_void_p)]


class PolicyRowsArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("J", C.c_int32), ("S", C.c_int32), ("row_mode", C.c_int32), ("net", MlpNet),
                ("obs", C.c_void_p), ("theta", C.c_void_p), ("action", C.c_void_p)]


class PlanRolloutPolicyArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("record", C.c_int32), ("rollout", PlanRolloutArgs), ("net", MlpNet), ("theta", C.c_void_p),
                ("start_day", C.c_void_p), ("obs", C.c_void_p), ("actions", C.c_void_p), ("Np", C.c_int32), ("row_mode", C.c_int32),
                ("J", C.c_int32), ("P", C.c_int32), ("K", C.c_int32), ("S", C.c_int32), ("hold", C.c_int32), ("scale", C.c_double),
                ("seed", C.c_uint64), ("draw_index", C.c_uint64), ("draw_base", C.c_void_p)]


# rollout collection (include/glgym.h glgym_ac_rows / glgym_gae)
AC_KEY_TAG = 0x41435431                                   # "ACT1": xor-ed into the high word of the noise key


class AcRowsArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("B", C.c_int32), ("in_dim", C.c_int32), ("step", C.c_int32), ("deterministic", C.c_int32),
                ("value_only", C.c_int32), ("mean_in", C.c_void_p), ("value_in", C.c_void_p), ("log_std", C.c_void_p), ("std", C.c_void_p),
                ("seed", C.c_uint64), ("draw_index", C.c_uint64), ("draw_base", C.c_void_p), ("obs", C.c_void_p), ("obs_out", C.c_void_p),
                ("action", C.c_void_p), ("action_env", C.c_void_p), ("eps", C.c_void_p), ("logp", C.c_void_p), ("value", C.c_void_p)]


class GaeArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("T", C.c_int32), ("B", C.c_int32), ("reward", C.c_void_p), ("done", C.c_void_p),
                ("value", C.c_void_p), ("last_value", C.c_void_p), ("gamma", C.c_double), ("lambda_", C.c_double),
                ("advantage", C.c_void_p), ("returns", C.c_void_p)]


# PPO update (include/glgym.h glgym_ppo_batch / glgym_ppo_loss)
PPO_KEY_TAG = 0x50524D31                                  # "PRM1": xor-ed into the high word of the permutation's key
PPO_MAX_BLOCKS, PPO_N_SUM, PPO_N_ADV = 1024, 11, 2
PPO_BATCH_WS_BYTES, PPO_LOSS_WS_BYTES = PPO_MAX_BLOCKS * PPO_N_ADV * 8, PPO_MAX_BLOCKS * PPO_N_SUM * 8
PPO_STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "max_ratio", "n")


class PpoBatchArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("N", C.c_int32), ("M", C.c_int32), ("offset", C.c_int32), ("in_dim", C.c_int32),
                ("seed", C.c_uint64), ("draw_index", C.c_uint64), ("draw_base", C.c_void_p), ("obs", C.c_void_p), ("action", C.c_void_p),
                ("logp", C.c_void_p), ("advantage", C.c_void_p), ("returns", C.c_void_p), ("value", C.c_void_p), ("mb_obs", C.c_void_p),
                ("mb_action", C.c_void_p), ("mb_logp", C.c_void_p), ("mb_adv", C.c_void_p), ("mb_ret", C.c_void_p), ("mb_value", C.c_void_p),
                ("mb_index", C.c_void_p), ("adv_stats", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class PpoLossArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("M", C.c_int32), ("mean", C.c_void_p), ("value", C.c_void_p), ("log_std", C.c_void_p),
                ("inv_std", C.c_void_p), ("mb_action", C.c_void_p), ("mb_logp", C.c_void_p), ("mb_adv", C.c_void_p), ("mb_ret", C.c_void_p),
                ("mb_value", C.c_void_p), ("adv_stats", C.c_void_p), ("clip_range", C.c_double), ("clip_range_vf", C.c_double),
                ("vf_coef", C.c_double), ("ent_coef", C.c_double), ("grad_mean", C.c_void_p), ("grad_value", C.c_void_p),
                ("grad_log_std", C.c_void_p), ("stats", C.c_void_p), ("ratio_out", C.c_void_p), ("logp_out", C.c_void_p),
                ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


# soft actor-critic (include/glgym.h glgym_sac_rows / glgym_sac_rows_grad / glgym_sac_batch / glgym_sac_loss / glgym_polyak)
SAC_KEY_TAG, SAC_SAMPLE_TAG = 0x53414331, 0x534D5031      # "SAC1", "SMP1": xor-ed into the high word of the noise and the sampling key
SAC_N_SUM, SAC_MAX_TENSORS = 5, 64
SAC_LOSS_WS_BYTES = PPO_MAX_BLOCKS * SAC_N_SUM * 8
SAC_CRITIC, SAC_ACTOR = 0, 1
SAC_CRITIC_STATS = ("critic_loss", "q1_mse", "q2_mse", "q1_mean", "q2_mean", "target_mean", "alpha", "n")
SAC_ACTOR_STATS = ("actor_loss", "ent_coef_loss", "grad_log_alpha", "logp_mean", "alpha", "log_alpha", "unused", "n")
# one row of SAC.update's stats_t
SAC_STATS = ("critic_loss", "actor_loss", "ent_coef_loss", "alpha", "logp_mean", "q1_mean", "target_mean", "n")


class SacRowsArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("M", C.c_int32), ("in_dim", C.c_int32), ("step", C.c_int32), ("deterministic", C.c_int32),
                ("uniform", C.c_int32), ("row0", C.c_int64), ("mean_in", C.c_void_p), ("log_std_in", C.c_void_p), ("seed", C.c_uint64),
                ("draw_index", C.c_uint64), ("draw_base", C.c_void_p), ("action_noise_sigma", C.c_double), ("obs", C.c_void_p),
                ("obs_out", C.c_void_p), ("action", C.c_void_p), ("action_env", C.c_void_p), ("action_slot", C.c_void_p), ("logp", C.c_void_p),
                ("eps", C.c_void_p), ("eps2", C.c_void_p), ("std", C.c_void_p), ("tanh", C.c_void_p), ("corr", C.c_void_p)]


class SacRowsGradArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("M", C.c_int32), ("grad_action", C.c_void_p), ("grad_logp", C.c_void_p), ("eps", C.c_void_p),
                ("std", C.c_void_p), ("tanh", C.c_void_p), ("log_std_in", C.c_void_p), ("grad_mean", C.c_void_p), ("grad_log_std", C.c_void_p)]


class SacBatchArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("S", C.c_int32), ("B", C.c_int32), ("in_dim", C.c_int32), ("M", C.c_int32), ("head", C.c_int32),
                ("n_valid", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("draw_index", C.c_uint64), ("draw_base", C.c_void_p),
                ("obs", C.c_void_p), ("action", C.c_void_p), ("reward", C.c_void_p), ("done", C.c_void_p), ("mb_obs", C.c_void_p),
                ("mb_next_obs", C.c_void_p), ("mb_action", C.c_void_p), ("mb_reward", C.c_void_p), ("mb_done", C.c_void_p),
                ("index_out", C.c_void_p)]


class SacLossArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("M", C.c_int32), ("stage", C.c_int32), ("reserved", C.c_int32), ("q1", C.c_void_p),
                ("q2", C.c_void_p), ("logp", C.c_void_p), ("q1_next", C.c_void_p), ("q2_next", C.c_void_p), ("reward", C.c_void_p),
                ("done", C.c_void_p), ("alpha", C.c_void_p), ("log_alpha", C.c_void_p), ("gamma", C.c_double), ("target_entropy", C.c_double),
                ("grad_q1", C.c_void_p), ("grad_q2", C.c_void_p), ("grad_logp", C.c_void_p), ("target_out", C.c_void_p),
                ("grad_log_alpha", C.c_void_p), ("stats", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class PolyakArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n", C.c_int32), ("dst", C.c_void_p), ("src", C.c_void_p), ("count", C.c_void_p),
                ("max_count", C.c_int64), ("tau", C.c_double)]


# recurrent PPO (include/glgym.h glgym_lstm_cell / glgym_lstm_cell_grad / glgym_seq_batch)
LSTM_MAX_H, LSTM_MAX_BLOCKS, LSTM_N_ACT, SEQ_MAX_STATE = 1024, 2048, 5, 4
SEQ_BATCH_WS_BYTES = PPO_BATCH_WS_BYTES


class LstmCellArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("M", C.c_int32), ("H", C.c_int32), ("gx", C.c_void_p), ("gh", C.c_void_p), ("c_prev", C.c_void_p),
                ("start", C.c_void_p), ("h", C.c_void_p), ("c", C.c_void_p), ("act", C.c_void_p)]


class LstmCellGradArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("M", C.c_int32), ("H", C.c_int32), ("dh", C.c_void_p), ("dc", C.c_void_p), ("act", C.c_void_p),
                ("c_prev", C.c_void_p), ("start", C.c_void_p), ("d_gx", C.c_void_p), ("d_gh", C.c_void_p), ("d_c_prev", C.c_void_p)]


class SeqBatchArgs(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("T", C.c_int32), ("B", C.c_int32), ("L", C.c_int32), ("S", C.c_int32), ("offset", C.c_int32),
                ("in_dim", C.c_int32), ("n_state", C.c_int32), ("state_dim", C.c_int32 * 4), ("seed", C.c_uint64), ("draw_index", C.c_uint64),
                ("draw_base", C.c_void_p), ("obs", C.c_void_p), ("action", C.c_void_p), ("logp", C.c_void_p), ("advantage", C.c_void_p),
                ("returns", C.c_void_p), ("value", C.c_void_p), ("episode_starts", C.c_void_p), ("state_src", C.c_void_p * 4),
                ("mb_obs", C.c_void_p), ("mb_action", C.c_void_p), ("mb_logp", C.c_void_p), ("mb_adv", C.c_void_p), ("mb_ret", C.c_void_p),
                ("mb_value", C.c_void_p), ("mb_start", C.c_void_p), ("state_out", C.c_void_p * 4), ("mb_index", C.c_void_p),
                ("adv_stats", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_int64)]


class WeatherArgs(C.Structure):
    _fields_ = [("n_raw", C.c_int32), ("time", C.c_void_p), ("i_glob", C.c_void_p), ("t_out", C.c_void_p),
                ("rh", C.c_void_p), ("wind", C.c_void_p), ("t_sky", C.c_void_p), ("co2_ppm", C.c_double),
                ("n_out", C.c_int32), ("nd", C.c_int32), ("out", C.c_void_p), ("workspace", C.c_void_p)]


# every symbol include/glgym.h declares, with its prototype
_DP = C.POINTER(C.c_double)
PROTOTYPES = {
    "glgym_version": (C.c_char_p, []),
    "glgym_abi_version": (C.c_int, []),
    "glgym_set_window": (C.c_int, [C.c_void_p, C.c_int]),
    "glgym_set_layout": (C.c_int, [C.c_void_p, C.c_int]),
    "glgym_set_occupancy": (C.c_int, [C.c_void_p, C.c_int]),
    "glgym_set_ladder_parallel": (C.c_int, [C.c_void_p, C.c_int]),
    "glgym_last_error": (C.c_char_p, []),
    "glgym_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, _DP, C.c_int, C.c_int, C.c_int,
                               C.POINTER(C.c_void_p)]),
    "glgym_destroy": (C.c_int, [C.c_void_p]),
    "glgym_set_params": (C.c_int, [C.c_void_p, _DP]),
    "glgym_set_params_keep_reward_scale": (C.c_int, [C.c_void_p, _DP]),
    "glgym_set_n_sub": (C.c_int, [C.c_void_p, C.c_int]),
    "glgym_set_model_variant": (C.c_int, [C.c_void_p, C.c_int]),
    "glgym_set_scheme": (C.c_int, [C.c_void_p, C.c_int]),
    "glgym_set_verify": (C.c_int, [C.c_void_p, C.c_int]),
    "glgym_set_reward": (C.c_int, [C.c_void_p, C.POINTER(RewardCfg)]),
    "glgym_get_reward_scale": (C.c_int, [C.c_void_p, _DP, _DP, _DP]),
    "glgym_evalF": (C.c_int, [C.c_void_p, _DP, _DP, _DP, _DP, C.c_int, C.c_int, _DP]),
    "glgym_rhs": (C.c_int, [C.c_void_p, _DP, _DP, _DP, C.c_int, _DP]),
    "glgym_set_integrator": (C.c_int, [C.c_void_p, C.c_int]),
    "glgym_set_tolerances": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int]),
    "glgym_get_solver_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "glgym_set_step_integrator": (C.c_int, [C.c_void_p, C.c_int]),
    "glgym_step": (C.c_int, [C.c_void_p, C.POINTER(StepArgs), C.c_void_p]),
    "glgym_obs": (C.c_int, [C.c_void_p, C.POINTER(ObsArgs), C.c_void_p]),
    "glgym_step_obs": (C.c_int, [C.c_void_p, C.POINTER(StepArgs), C.POINTER(ObsArgs), C.c_void_p]),
    "glgym_step_obs_reset": (C.c_int, [C.c_void_p, C.POINTER(StepArgs), C.POINTER(ObsArgs), C.POINTER(ResetArgs), C.c_void_p,
                             C.POINTER(C.c_int32)]),
    "glgym_last_step_build": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "glgym_last_evalf_build": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "glgym_set_obs_modules": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "glgym_obs_dim": (C.c_int, [C.c_void_p, C.c_int]),
    "glgym_set_control_limits": (C.c_int, [C.c_void_p, _DP, _DP, C.c_double]),
    "glgym_reset": (C.c_int, [C.c_void_p, C.POINTER(ResetArgs), C.c_void_p]),
    "glgym_crop_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_uint64, C.c_uint64,
                                   C.c_void_p]),
    "glgym_rng_crop_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]),
    "glgym_rng_reset_draw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "glgym_plan_fork": (C.c_int, [C.c_void_p, C.POINTER(PlanForkArgs), C.c_void_p]),
    "glgym_plan_accumulate": (C.c_int, [C.c_void_p, C.POINTER(PlanAccumulateArgs), C.c_void_p]),
    "glgym_plan_rollout": (C.c_int, [C.c_void_p, C.POINTER(PlanRolloutArgs), C.c_void_p]),
    "glgym_plan_select": (C.c_int, [C.c_void_p, C.POINTER(PlanSelectArgs), C.c_void_p]),
    "glgym_plan_sample": (C.c_int, [C.c_void_p, C.POINTER(PlanSampleArgs), C.c_void_p]),
    "glgym_plan_elites": (C.c_int, [C.c_void_p, C.POINTER(PlanElitesArgs), C.c_void_p]),
    "glgym_plan_refit": (C.c_int, [C.c_void_p, C.POINTER(PlanRefitArgs), C.c_void_p]),
    "glgym_plan_es_sample": (C.c_int, [C.c_void_p, C.POINTER(PlanEsSampleArgs), C.c_void_p]),
    "glgym_plan_es_utilities": (C.c_int, [C.c_void_p, C.POINTER(PlanEsUtilitiesArgs), C.c_void_p]),
    "glgym_plan_es_update": (C.c_int, [C.c_void_p, C.POINTER(PlanEsUpdateArgs), C.c_void_p]),
    "glgym_plan_cma_sample": (C.c_int, [C.c_void_p, C.POINTER(PlanCmaSampleArgs), C.c_void_p]),
    "glgym_plan_cma_update": (C.c_int, [C.c_void_p, C.POINTER(PlanCmaUpdateArgs), C.c_void_p]),
    "glgym_plan_scenario": (C.c_int, [C.c_void_p, C.POINTER(PlanScenarioArgs), C.c_void_p]),
    "glgym_plan_rollout_scenarios": (C.c_int, [C.c_void_p, C.POINTER(PlanRolloutScenariosArgs), C.c_void_p]),
    "glgym_plan_aggregate": (C.c_int, [C.c_void_p, C.POINTER(PlanAggregateArgs), C.c_void_p]),
    "glgym_plan_constrain": (C.c_int, [C.c_void_p, C.POINTER(PlanConstrainArgs), C.c_void_p]),
    "glgym_plan_weather": (C.c_int, [C.c_void_p, C.POINTER(PlanWeatherArgs), C.c_void_p]),
    "glgym_rule_based": (C.c_int, [C.c_void_p, C.POINTER(RuleCfg), C.POINTER(RuleArgs), C.c_void_p]),
    "glgym_rule_rows": (C.c_int, [C.c_void_p, C.POINTER(RuleRowsArgs), C.c_void_p]),
    "glgym_plan_rollout_rule": (C.c_int, [C.c_void_p, C.POINTER(PlanRolloutRuleArgs), C.c_void_p]),
    "glgym_policy_rows": (C.c_int, [C.c_void_p, C.POINTER(PolicyRowsArgs), C.c_void_p]),
    "glgym_plan_rollout_policy": (C.c_int, [C.c_void_p, C.POINTER(PlanRolloutPolicyArgs), C.c_void_p]),
    "glgym_ac_rows": (C.c_int, [C.c_void_p, C.POINTER(AcRowsArgs), C.c_void_p]),
    "glgym_gae": (C.c_int, [C.c_void_p, C.POINTER(GaeArgs), C.c_void_p]),
    "glgym_ppo_batch": (C.c_int, [C.c_void_p, C.POINTER(PpoBatchArgs), C.c_void_p]),
    "glgym_ppo_loss": (C.c_int, [C.c_void_p, C.POINTER(PpoLossArgs), C.c_void_p]),
    "glgym_sac_rows": (C.c_int, [C.c_void_p, C.POINTER(SacRowsArgs), C.c_void_p]),
    "glgym_sac_rows_grad": (C.c_int, [C.c_void_p, C.POINTER(SacRowsGradArgs), C.c_void_p]),
    "glgym_sac_batch": (C.c_int, [C.c_void_p, C.POINTER(SacBatchArgs), C.c_void_p]),
    "glgym_sac_loss": (C.c_int, [C.c_void_p, C.POINTER(SacLossArgs), C.c_void_p]),
    "glgym_polyak": (C.c_int, [C.c_void_p, C.POINTER(PolyakArgs), C.c_void_p]),
    "glgym_lstm_cell": (C.c_int, [C.c_void_p, C.POINTER(LstmCellArgs), C.c_void_p]),
    "glgym_lstm_cell_grad": (C.c_int, [C.c_void_p, C.POINTER(LstmCellGradArgs), C.c_void_p]),
    "glgym_seq_batch": (C.c_int, [C.c_void_p, C.POINTER(SeqBatchArgs), C.c_void_p]),
    "glgym_vecnorm": (C.c_int, [C.c_void_p, C.POINTER(VecNormArgs), C.c_void_p]),
    "glgym_weather": (C.c_int, [C.c_void_p, C.POINTER(WeatherArgs), C.c_void_p]),
    "glgym_timer_start": (C.c_int, [C.c_void_p, C.c_void_p]),
    "glgym_timer_stop": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_float)]),
}

_lib = None


def load():
    """dlopen libglgym.so and bind every prototype.  Raises GlgymError if the HIP extension is missing."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise GlgymError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                             "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        try:
            # PyTorch-ROCm bundles its own HIP runtime; it must be the first one the process loads, otherwise
            # torch.cuda.is_available() turns False once /opt/rocm's copy (our DT_NEEDED) is already resident.
            import torch  # noqa: F401
        except Exception:  # torch is plumbing only; GreenLight.evalF works without it
            pass
        lib = C.CDLL(str(LIB_PATH))
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)          # AttributeError here = ABI mismatch with include/glgym.h
            fn.restype, fn.argtypes = res, args
        if lib.glgym_abi_version() != ABI_VERSION:
            raise GlgymError(f"{LIB_PATH} has ABI {lib.glgym_abi_version()}, this binding expects {ABI_VERSION}: rebuild the library")
        _lib = lib
    return _lib


def check(rc: int, what: str = "glgym"):
    if rc != OK:
        msg = load().glgym_last_error().decode() or {EINVAL: "invalid argument", ENODEV: "no HIP device",
                                                       EHIP: "HIP error", ENOMEM: "out of memory"}.get(rc, "")
        raise (GlgymOdeError if rc == EODE else GlgymError)(f"{what} failed (status {rc}): {msg}")
