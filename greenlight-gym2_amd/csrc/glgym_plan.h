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
