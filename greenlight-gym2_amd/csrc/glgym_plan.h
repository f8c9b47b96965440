// glgym_plan.h -- internal interface between the C ABI (glgym.hip) and the planning kernels (glgym_plan.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glgym.h"

// All launches: on `stream`, no host copy, allocation or synchronisation (capturable).  T = float | double (instantiated in
// glgym_plan.hip); the arguments have been checked by the caller.
template <class T>
hipError_t plan_fork_launch(const glgym_plan_fork_args& a, hipStream_t stream);
template <class T>
hipError_t plan_accumulate_launch(const glgym_plan_accumulate_args& a, hipStream_t stream);
hipError_t plan_select_launch(const glgym_plan_select_args& a, hipStream_t stream);
// The cross-entropy method's stages (gl_cem.hpp): independent of the handle's dtype (the action block is f32, the returns double).
hipError_t plan_sample_launch(const glgym_plan_sample_args& a, hipStream_t stream);
hipError_t plan_elites_launch(const glgym_plan_elites_args& a, hipStream_t stream);
hipError_t plan_refit_launch(const glgym_plan_refit_args& a, hipStream_t stream);
// Robust planning (gl_scen.hpp).  p0_crop: the handle's float32 p[128..161] on the device; a.P * a.K * a.S <= INT32_MAX.
template <class T>
hipError_t plan_scenario_launch(const glgym_plan_scenario_args& a, const float* p0_crop, hipStream_t stream);
hipError_t plan_aggregate_launch(const glgym_plan_aggregate_args& a, hipStream_t stream);   // the returns are double: no T
// Weather-forecast scenarios (gl_wscen.hpp).  nd: the handle's column count; sqrt(1 - phi^2) is taken on the host here; the shape
// has been checked (a.P * a.S * a.H and a.P * a.K * a.S <= INT32_MAX).  Two launches: the window, then (if asked for) the child offsets.
template <class T>
hipError_t plan_weather_launch(const glgym_plan_weather_args& a, int nd, hipStream_t stream);
