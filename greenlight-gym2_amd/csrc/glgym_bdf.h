// glgym_bdf.h -- internal interface between the C ABI (glgym.hip) and the BDF integrator's kernel (glgym_bdf.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gl_model.hpp"

// Launches one wavefront per row on the default stream: x_next = x(dt) for rows of device arrays x[B][28], u[B][6], d[B][nd] and,
// when crop != nullptr, each row's own crop block crop[B][34] (p[128..161]).  Failed rows are NaN and counted in *n_failed;
// stats[B][5] = steps, right-hand sides, Jacobians, LU factorisations, final order.  Returns the launch's hipError_t.
hipError_t bdf_launch(const double* x, const double* u, const double* d, const double* crop, int B, int nd, double dt, double rtol,
                      double atol, int max_steps, const glm::ModelConst<double>& m, double gasR, double tCanMin, double* out,
                      int32_t* stats, int* n_failed);
