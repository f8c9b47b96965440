// TESTS ONLY.  The pieces of the BDF integrator's wavefront team (greenlight-gym2_amd/csrc/gl_bdf_wave.hpp, gl_bdf.hpp) behind entry
// points a test can call: one 64-lane workgroup per problem, the geometry of bdf_row_kernel / bdf_env_kernel, running the product's
// own source.  Every pointer is a device pointer of n problems unless stated; every call returns the hipError_t of its launch.
// The product library (libglgym.so) never links or loads this file.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "bdfwave_common.hpp"
#include "gl_bdf_wave.hpp"

using namespace glm;
using glbdf::WAVE;

namespace {

__global__ __launch_bounds__(WAVE) void reduce_kernel(const double* __restrict__ v, const int* __restrict__ idx,
                                                      const double* __restrict__ rv, const double* __restrict__ rs,
                                                      double* __restrict__ sum_out, double* __restrict__ amax_v, int* __restrict__ amax_i,
                                                      double* __restrict__ rms_out)
{
    __shared__ glbdf::BdfScratch sh;
    const size_t b = blockIdx.x;
    const int ln = threadIdx.x;
    const glbdf::WaveTeam<bdfwave::NoRhs> tm{ln, {}};
    const double x = v[b * WAVE + ln];
    sum_out[b * WAVE + ln] = tm.sum(x);
    double a = x;
    int i = idx[b * WAVE + ln];
    tm.argmax(a, i);
    amax_v[b * WAVE + ln] = a;
    amax_i[b * WAVE + ln] = i;
    rms_out[b * WAVE + ln] = bdfwave::rms_problem(tm, sh, rv + b * NX, rs + b * NX);
}

__global__ __launch_bounds__(WAVE) void lu_kernel(const double* __restrict__ J, const double* __restrict__ c, const double* __restrict__ rhs_b,
                                                  int* __restrict__ ok, double* __restrict__ LU, int* __restrict__ piv,
                                                  int* __restrict__ perm, double* __restrict__ x)
{
    __shared__ glbdf::BdfScratch sh;
    const size_t b = blockIdx.x;
    const glbdf::WaveTeam<bdfwave::NoRhs> tm{(int)threadIdx.x, {}};
    bdfwave::lu_problem(tm, sh, J + b * NX * NX, c[b], rhs_b + b * NX, ok + b, LU + b * NX * NX, piv + b * NX, perm + b * NX, x + b * NX);
}

__global__ __launch_bounds__(WAVE) void change_D_kernel(const double* __restrict__ D, const int* __restrict__ order,
                                                        const double* __restrict__ factor, double* __restrict__ Dout)
{
    __shared__ glbdf::BdfScratch sh;
    const size_t b = blockIdx.x, nd = (glbdf::MAXORD + 3) * NX;
    const glbdf::WaveTeam<bdfwave::NoRhs> tm{(int)threadIdx.x, {}};
    bdfwave::change_D_problem(tm, sh, D + b * nd, order[b], factor[b], Dout + b * nd);
}

__global__ __launch_bounds__(WAVE) void step_kernel(const int* __restrict__ kind, const double* __restrict__ y0,
                                                    const double* __restrict__ A, const double* __restrict__ g,
                                                    const double* __restrict__ mu, const double* __restrict__ dt,
                                                    const double* __restrict__ rtol, const double* __restrict__ atol,
                                                    const int* __restrict__ max_steps, double* __restrict__ y, int32_t* __restrict__ stats,
                                                    int* __restrict__ rc)
{
    __shared__ glbdf::BdfScratch sh;
    const size_t b = blockIdx.x;
    const glbdf::WaveTeam<bdfwave::SynthRhs> tm{(int)threadIdx.x, {kind[b], A + b * NX * NX, g + b * NX, mu[b]}};
    bdfwave::step_problem(tm, sh, y0 + b * NX, dt[b], rtol[b], atol[b], max_steps[b], y + b * NX, stats + b * glbdf::NSTAT, rc + b);
}

// the library's team on a model row: ModelConst of the row from global memory into LDS as the library's kernels stage their argument,
// the row's StepCoef by lane 0 as gl_bdf_env.hpp bdf_row
__global__ __launch_bounds__(WAVE) void model_jac_kernel(const double* __restrict__ x, const double* __restrict__ u,
                                                         const double* __restrict__ d, const ModelConst<double>* __restrict__ mc,
                                                         int need_f0, double* __restrict__ f, double* __restrict__ f0,
                                                         double* __restrict__ J)
{
    __shared__ glbdf::BdfScratch sh;
    __shared__ ModelConst<double> sh_m[1];
    __shared__ StepCoef<double> sh_s[1];
    const size_t b = blockIdx.x;
    const int ln = threadIdx.x;
    {
        static_assert(sizeof(ModelConst<double>) % 4 == 0, "word copy");
        const unsigned* src = reinterpret_cast<const unsigned*>(mc + b);
        unsigned* dst = reinterpret_cast<unsigned*>(&sh_m[0]);
        for (int i = ln; i < (int)(sizeof(ModelConst<double>) / 4); i += WAVE) dst[i] = src[i];
    }
    __syncthreads();
    if (ln == 0) {
        double uu[NU], dd[7];
        for (int i = 0; i < NU; ++i) uu[i] = u[b * NU + i];
        for (int i = 0; i < 7; ++i) dd[i] = d[b * 7 + i];
        StepCoef<double> c;
        precompute(uu, dd, sh_m[0], sh_m[0].crop, c);
        sh_s[0] = c;
    }
    __syncthreads();
    const glbdf::WaveTeam<glbdf::ModelRhs> tm{ln, {sh_m[0], sh_m[0].crop, sh_s[0]}};
    bdfwave::jac_problem(tm, sh, x + b * NX, need_f0, f + b * NX, f0 + b * NX, J + b * NX * NX);
}

}  // namespace

extern "C" {

// v[n][64], idx[n][64] (the index each lane brings to argmax), rv[n][28], rs[n][28] -> per lane: sum, argmax value and index, bdf_rms
int bdfwave_reduce(const double* v, const int* idx, const double* rv, const double* rs, int n, double* sum_out, double* amax_v,
                   int* amax_i, double* rms_out, hipStream_t stream)
{
    hipLaunchKernelGGL(reduce_kernel, dim3(n), dim3(WAVE), 0, stream, v, idx, rv, rs, sum_out, amax_v, amax_i, rms_out);
    return (int)hipGetLastError();
}

// J[n][28][28], c[n], b[n][28] -> ok[n], LU[n][28][28], piv[n][28], perm[n][28], x[n][28]
int bdfwave_lu(const double* J, const double* c, const double* b, int n, int* ok, double* LU, int* piv, int* perm, double* x,
               hipStream_t stream)
{
    hipLaunchKernelGGL(lu_kernel, dim3(n), dim3(WAVE), 0, stream, J, c, b, ok, LU, piv, perm, x);
    return (int)hipGetLastError();
}

// D[n][8][28], order[n] in 1..5, factor[n] -> Dout[n][8][28]
int bdfwave_change_D(const double* D, const int* order, const double* factor, int n, double* Dout, hipStream_t stream)
{
    hipLaunchKernelGGL(change_D_kernel, dim3(n), dim3(WAVE), 0, stream, D, order, factor, Dout);
    return (int)hipGetLastError();
}

// kind[n], y0[n][28], A[n][28][28], g[n][28], mu[n], dt[n], rtol[n], atol[n], max_steps[n] -> y[n][28], stats[n][5], rc[n]
int bdfwave_step(const int* kind, const double* y0, const double* A, const double* g, const double* mu, const double* dt,
                 const double* rtol, const double* atol, const int* max_steps, int n, double* y, int32_t* stats, int* rc,
                 hipStream_t stream)
{
    hipLaunchKernelGGL(step_kernel, dim3(n), dim3(WAVE), 0, stream, kind, y0, A, g, mu, dt, rtol, atol, max_steps, y, stats, rc);
    return (int)hipGetLastError();
}

// x[n][28], u[n][6], d[n][7] on the device; p[n][208] on the HOST (ModelConst is built here, as glgym_create builds the handle's);
// f0[n][28] is read when need_f0 == 0 and written otherwise -> f[n][28] (eval1), f0, J[n][28][28].  Synchronises the stream.
int bdfwave_model_jac(const double* x, const double* u, const double* d, const double* p_host, int need_f0, int n, double* f, double* f0,
                      double* J, hipStream_t stream)
{
    std::vector<ModelConst<double>> mc((size_t)n);
    for (int b = 0; b < n; ++b) {
        std::memset(&mc[b], 0, sizeof(ModelConst<double>));
        make_model_const<double>(p_host + (size_t)b * NP, mc[b]);
    }
    ModelConst<double>* dmc = nullptr;
    hipError_t e = hipMalloc(&dmc, mc.size() * sizeof(ModelConst<double>));
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(dmc, mc.data(), mc.size() * sizeof(ModelConst<double>), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(model_jac_kernel, dim3(n), dim3(WAVE), 0, stream, x, u, d, dmc, need_f0, f, f0, J);
        e = hipGetLastError();
        const hipError_t e2 = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = e2;
    }
    (void)hipFree(dmc);
    return (int)e;
}

}  // extern "C"
