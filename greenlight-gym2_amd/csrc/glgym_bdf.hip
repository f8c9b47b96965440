// glgym_bdf.hip -- the BDF integrator of glgym_evalF (GLGYM_INTEGRATOR_BDF): gl_bdf.hpp on a team of one wavefront per row.
//
// Layout: one 64-lane workgroup integrates one row.  The handle's ModelConst, the row's CropConst and StepCoef, the difference
// array, the Jacobian and the LU factors live in LDS; lane i < 28 owns state i in the vector work.  A trajectory evaluation of the
// right-hand side runs in lane 0; the 28 finite-difference columns of a Jacobian (and the base point of a re-evaluated one) run in
// lanes 0..28 side by side from the same call site, so a Jacobian costs one right-hand-side latency.  fp64 throughout, for either
// handle dtype.  No MFMA, no scalar-memory stores.
// bdf_row_kernel is glgym_evalF's (GLGYM_INTEGRATOR_BDF); bdf_env_kernel is glgym_step's (glgym_set_step_integrator): the same row
// integrator (gl_bdf_env.hpp bdf_row) inside the env-step's controls and reward epilogue, one wavefront per environment.
#include "glgym_bdf.h"

#include "gl_bdf_env.hpp"
#include "gl_bdf_wave.hpp"

using namespace glm;

namespace {

using glbdf::WAVE;

// the wavefront team (gl_bdf_wave.hpp) over the model's right-hand side
using WaveTeam = glbdf::WaveTeam<glbdf::ModelRhs>;

__global__ __launch_bounds__(WAVE) void bdf_row_kernel(const double* __restrict__ x, const double* __restrict__ u,
                                                       const double* __restrict__ d, const double* __restrict__ crop, int nd, double dt,
                                                       double rtol, double atol, int max_steps, ModelConst<double> m_arg, double gasR,
                                                       double tCanMin, double* __restrict__ out, int32_t* __restrict__ stats,
                                                       int* __restrict__ n_failed)
{
    __shared__ glbdf::BdfScratch sh;
    __shared__ ModelConst<double> sh_m[1];
    __shared__ CropConst<double> sh_cr[1];
    __shared__ StepCoef<double> sh_s[1];
    const int b = blockIdx.x, ln = threadIdx.x;
    {
        // the parameter block in LDS (broadcast reads; as a kernel argument its ~180 doubles would not fit the SGPRs)
        static_assert(sizeof(ModelConst<double>) % 4 == 0, "word copy");
        const unsigned* src = reinterpret_cast<const unsigned*>(&m_arg);
        unsigned* dst = reinterpret_cast<unsigned*>(&sh_m[0]);
        for (int i = ln; i < (int)(sizeof(ModelConst<double>) / 4); i += WAVE) dst[i] = src[i];
    }
    double bad = 0.0;
    if (ln < NX) {
        const double v = x[(size_t)b * NX + ln];
        sh.D[0][ln] = v;
        if (!__builtin_isfinite(v)) bad = 1.0;
    }
    if (ln < NU && !__builtin_isfinite(u[(size_t)b * NU + ln])) bad = 1.0;
    if (ln < 7 && !__builtin_isfinite(d[(size_t)b * nd + ln])) bad = 1.0;
    __syncthreads();
    const WaveTeam tm{ln, {sh_m[0], sh_cr[0], sh_s[0]}};
    int32_t st[glbdf::NSTAT] = {0, 0, 0, 0, 0};
    const int rc = glbdf::bdf_row(tm, sh, sh_m[0], sh_cr[0], sh_s[0], crop ? crop + (size_t)b * NCROP : nullptr, gasR, tCanMin,
                                  u + (size_t)b * NU, d + (size_t)b * nd, bad, dt, rtol, atol, max_steps, st);
    if (ln < NX) out[(size_t)b * NX + ln] = rc == glbdf::BDF_OK ? sh.D[0][ln] : __builtin_nan("");
    if (ln < glbdf::NSTAT) {
        int32_t v = st[0];
#pragma unroll
        for (int i = 1; i < glbdf::NSTAT; ++i) v = ln == i ? st[i] : v;
        stats[(size_t)b * glbdf::NSTAT + ln] = v;
    }
    if (ln == 0 && rc != glbdf::BDF_OK) atomicAdd(n_failed, 1);
}

// One env-step of environment blockIdx.x (gl_bdf_env.hpp bdf_env_row); lane 0 adds its metrics to the replica of its block.
template <class T>
__global__ __launch_bounds__(WAVE) void bdf_env_kernel(glbdf::BdfEnvArgs<T> a, ModelConst<double> m_arg, RewardConstBase<T> rw,
                                                       float* __restrict__ metrics)
{
    __shared__ glbdf::BdfEnvScratch sh;
    __shared__ ModelConst<double> sh_m[1];
    __shared__ CropConst<double> sh_cr[1];
    __shared__ StepCoef<double> sh_s[1];
    const int b = blockIdx.x, ln = threadIdx.x;
    {
        static_assert(sizeof(ModelConst<double>) % 4 == 0, "word copy");
        const unsigned* src = reinterpret_cast<const unsigned*>(&m_arg);
        unsigned* dst = reinterpret_cast<unsigned*>(&sh_m[0]);
        for (int i = ln; i < (int)(sizeof(ModelConst<double>) / 4); i += WAVE) dst[i] = src[i];
    }
    __syncthreads();
    const WaveTeam tm{ln, {sh_m[0], sh_cr[0], sh_s[0]}};
    const glbdf::BdfEnvResult<T> r = glbdf::bdf_env_row<T>(tm, sh, sh_m[0], sh_cr[0], sh_s[0], rw, a, b);
    if (metrics && ln == 0) {      // GLGYM_NMETRIC order for slots 0..7 (8..13 belong to the explicit ladder), then GLGYM_METRIC_BDF
        float* mrep = metrics + (size_t)(b % GLGYM_METRIC_REPLICAS) * GLGYM_METRIC_STRIDE;
        const float mv[8] = {(float)r.reward, (float)r.profit, r.done ? 1.f : 0.f, r.failed ? 1.f : 0.f,
                             (float)r.viol[0], (float)r.viol[1], (float)r.viol[2], 1.f};
#pragma unroll
        for (int i = 0; i < 8; ++i) atomicAdd(mrep + i, mv[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i) atomicAdd(mrep + GLGYM_METRIC_BDF + i, (float)r.stats[i]);
    }
}

}  // namespace

hipError_t bdf_launch(const double* x, const double* u, const double* d, const double* crop, int B, int nd, double dt, double rtol,
                      double atol, int max_steps, const ModelConst<double>& m, double gasR, double tCanMin, double* out,
                      int32_t* stats, int* n_failed)
{
    hipLaunchKernelGGL(bdf_row_kernel, dim3(B), dim3(WAVE), 0, (hipStream_t)0, x, u, d, crop, nd, dt, rtol, atol, max_steps, m, gasR,
                       tCanMin, out, stats, n_failed);
    return hipGetLastError();
}

template <class T>
hipError_t bdf_env_launch(const glbdf::BdfEnvArgs<T>& a, int B, const ModelConst<double>& m, const RewardConstBase<T>& rw, float* metrics,
                          hipStream_t stream)
{
    hipLaunchKernelGGL(bdf_env_kernel<T>, dim3(B), dim3(WAVE), 0, stream, a, m, rw, metrics);
    return hipGetLastError();
}

template hipError_t bdf_env_launch<float>(const glbdf::BdfEnvArgs<float>&, int, const ModelConst<double>&, const RewardConstBase<float>&,
                                          float*, hipStream_t);
template hipError_t bdf_env_launch<double>(const glbdf::BdfEnvArgs<double>&, int, const ModelConst<double>&,
                                           const RewardConstBase<double>&, float*, hipStream_t);
