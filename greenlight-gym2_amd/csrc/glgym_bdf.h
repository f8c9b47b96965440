// glgym_bdf.h -- internal interface between the C ABI (glgym.hip) and the BDF integrator's kernels (glgym_bdf.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gl_bdf_env.hpp"

// Launches one wavefront per row on the default stream: x_next = x(dt) for rows of device arrays x[B][28], u[B][6], d[B][nd] and,
// when crop != nullptr, each row's own crop block crop[B][34] (p[128..161]).  Failed rows are NaN and counted in *n_failed;
// stats[B][5] = steps, right-hand sides, Jacobians, LU factorisations, final order.  Returns the launch's hipError_t.
hipError_t bdf_launch(const double* x, const double* u, const double* d, const double* crop, int B, int nd, double dt, double rtol,
                      double atol, int max_steps, const glm::ModelConst<double>& m, double gasR, double tCanMin, double* out,
                      int32_t* stats, int* n_failed);

// glgym_step with GLGYM_INTEGRATOR_BDF: one wavefront per environment on `stream`, no host copy, allocation or synchronisation
// (capturable).  metrics: glgym_step_args.metrics or nullptr.  T = float | double (instantiated in glgym_bdf.hip).
template <class T>
hipError_t bdf_env_launch(const glbdf::BdfEnvArgs<T>& a, int B, const glm::ModelConst<double>& m, const glm::RewardConstBase<T>& rw,
                          float* metrics, hipStream_t stream);
