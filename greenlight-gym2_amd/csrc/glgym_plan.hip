// glgym_plan.hip -- the kernels of device-side planning (include/glgym.h glgym_plan_*): fork children from parent environments,
// accumulate a step's reward into the children's returns, pick the best of K candidates per parent and the MPPI-weighted mean.
// The scalar logic is gl_plan.hpp's (instantiated on the host by tests/planhost/planhost.cpp); the env-steps in between are
// glgym_step's own kernels, launched by the C ABI -- nothing of them is instantiated or fused here.
//
// Layouts.  fork / accumulate: one lane per child; every child-side access is coalesced (SoA planes, lane c at base[i*ld + c]), the
// parent side of a fork is a broadcast read (the K children of a parent sit in adjacent lanes and read one address).  select: one
// wavefront per parent, lanes stride over the candidates k, partial (value, index) pairs and sums are combined with butterfly
// shuffles; the action block [H][P*K][6] f32 is read with lanes over k, 6 consecutive floats each, so a wavefront touches 1 536
// contiguous bytes per load round.  The MPPI mean runs one wavefront per (parent, horizon step): the K returns are re-read from L2 by
// each (9 bytes per candidate against the 24 bytes of its action row), which keeps the call free of workspace and allocation.
// No LDS, no atomics, plain vector stores.
#include "glgym_plan.h"

#include "gl_plan.hpp"

namespace {

constexpr int NX = GLGYM_NX, NU = GLGYM_NU, NCROP = GLGYM_NCROP;
constexpr int WAVE = glplan::WAVE;

template <class T>
__global__ __launch_bounds__(256) void plan_fork_kernel(glgym_plan_fork_args a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n_children) return;
    int p = a.parent ? a.parent[c] : c / a.K;
    const bool bad = p < 0 || p >= a.n_parents;
    if (bad) p = 0;
    const size_t ldp = (size_t)a.ld_parent, ldc = (size_t)a.ld_child;
    const T* xp = (const T*)a.x_parent;
    T* x = (T*)a.x;
    for (int i = 0; i < NX; ++i) x[i * ldc + c] = xp[i * ldp + p];
    const T* up = (const T*)a.u_parent;
    T* u = (T*)a.u;
    for (int i = 0; i < NU; ++i) u[i * ldc + c] = up[i * ldp + p];
    if (a.crop && a.crop_parent) {
        const T* cp = (const T*)a.crop_parent;
        T* cc = (T*)a.crop;
        for (int i = 0; i < NCROP; ++i) cc[i * ldc + c] = cp[i * ldp + p];
    }
    a.timestep[c] = a.timestep_parent[p];
    a.w_off[c] = a.w_off_parent[p];
    if (a.start_day && a.start_day_parent) a.start_day[c] = a.start_day_parent[p];
    a.ret[c] = 0.0;
    for (int i = 0; i < 3; ++i) a.viol[i * ldc + c] = 0.0;
    a.n_steps[c] = 0;
    a.alive[c] = bad ? 0 : 1;
    a.failed[c] = bad ? 1 : 0;
}

template <class T>
__global__ __launch_bounds__(256) void plan_accumulate_kernel(glgym_plan_accumulate_args a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.B) return;
    uint8_t alive = a.alive[c];
    if (!alive) return;
    const size_t ld = (size_t)a.ld;
    const T* info = (const T*)a.info;
    double ret = a.ret[c], v0 = a.viol[c], v1 = a.viol[ld + c], v2 = a.viol[2 * ld + c];
    int32_t n = a.n_steps[c];
    uint8_t failed = a.failed[c];
    glplan::accumulate(ret, v0, v1, v2, n, alive, failed, a.w, (double)((const T*)a.reward)[c],
                       (double)info[glplan::INFO_CO2 * ld + c], (double)info[glplan::INFO_TEMP * ld + c],
                       (double)info[glplan::INFO_RH * ld + c], a.done[c], a.step_flags ? a.step_flags[c] : 0);
    a.ret[c] = ret;
    a.viol[c] = v0; a.viol[ld + c] = v1; a.viol[2 * ld + c] = v2;
    a.n_steps[c] = n;
    a.alive[c] = alive;
    a.failed[c] = failed;
}

__device__ __forceinline__ glplan::Cand wave_best(glplan::Cand c)
{
    for (int m = WAVE / 2; m > 0; m >>= 1) {
        glplan::Cand o;
        o.v = __shfl_xor(c.v, m, WAVE);
        o.k = __shfl_xor(c.k, m, WAVE);
        c = glplan::combine(c, o);
    }
    return c;
}

__device__ __forceinline__ double wave_sum(double v)
{
    for (int m = WAVE / 2; m > 0; m >>= 1) v = v + __shfl_xor(v, m, WAVE);
    return v;
}

// grid = P, one wavefront each
__global__ __launch_bounds__(WAVE) void plan_select_kernel(glgym_plan_select_args a)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const size_t first = (size_t)p * a.K;               // the parent's first child
    const glplan::Cand c = wave_best(glplan::lane_best(lane, a.K, a.ret + first, a.failed + first));
    const bool none = c.k == glplan::NONE;
    if (lane == 0) {
        a.best_k[p] = none ? -1 : c.k;
        a.best_ret[p] = none ? __builtin_nan("") : c.v;
    }
    if (!a.actions) return;
    const size_t n_child = (size_t)a.P * a.K;
    if (a.best_action && lane < NU) a.best_action[(size_t)p * NU + lane] = none ? 0.f : a.actions[(first + c.k) * NU + lane];
    if (a.best_sequence)
        for (int i = lane; i < a.H * NU; i += WAVE) {
            const int h = i / NU, j = i - h * NU;
            a.best_sequence[((size_t)h * a.P + p) * NU + j] = none ? 0.f : a.actions[((size_t)h * n_child + first + c.k) * NU + j];
        }
}

// grid = (P, H), one wavefront each
__global__ __launch_bounds__(WAVE) void plan_mean_kernel(glgym_plan_select_args a)
{
    const int p = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const size_t first = (size_t)p * a.K;
    const double* ret = a.ret + first;
    const uint8_t* failed = a.failed + first;
    const glplan::Cand c = wave_best(glplan::lane_best(lane, a.K, ret, failed));
    double acc[NU] = {0, 0, 0, 0, 0, 0};
    if (c.k != glplan::NONE) {                          // wave-uniform
        const double inv_t = 1.0 / a.temperature;
        const double z = wave_sum(glplan::lane_weight_sum(lane, a.K, ret, failed, c.v, inv_t));
        glplan::lane_mean(lane, a.K, ret, failed, c.v, inv_t, z, a.actions + ((size_t)h * a.P * a.K + first) * NU, acc);
        for (int j = 0; j < NU; ++j) acc[j] = wave_sum(acc[j]);
    }
    if (lane == 0) {
        float* out = a.mean_sequence + ((size_t)h * a.P + p) * NU;
        for (int j = 0; j < NU; ++j) out[j] = (float)acc[j];
    }
}

}  // namespace

template <class T>
hipError_t plan_fork_launch(const glgym_plan_fork_args& a, hipStream_t stream)
{
    hipLaunchKernelGGL(plan_fork_kernel<T>, dim3((a.n_children + 255) / 256), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template <class T>
hipError_t plan_accumulate_launch(const glgym_plan_accumulate_args& a, hipStream_t stream)
{
    hipLaunchKernelGGL(plan_accumulate_kernel<T>, dim3((a.B + 255) / 256), dim3(256), 0, stream, a);
    return hipGetLastError();
}

template hipError_t plan_fork_launch<float>(const glgym_plan_fork_args&, hipStream_t);
template hipError_t plan_fork_launch<double>(const glgym_plan_fork_args&, hipStream_t);
template hipError_t plan_accumulate_launch<float>(const glgym_plan_accumulate_args&, hipStream_t);
template hipError_t plan_accumulate_launch<double>(const glgym_plan_accumulate_args&, hipStream_t);

hipError_t plan_select_launch(const glgym_plan_select_args& a, hipStream_t stream)
{
    hipLaunchKernelGGL(plan_select_kernel, dim3(a.P), dim3(WAVE), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.mean_sequence) {
        hipLaunchKernelGGL(plan_mean_kernel, dim3(a.P, a.H), dim3(WAVE), 0, stream, a);
        e = hipGetLastError();
    }
    return e;
}
