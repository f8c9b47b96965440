// glgym_collect.hip -- rollout collection on the device (include/glgym.h glgym_ac_rows, glgym_gae), kernels and C entry points: the
// Gaussian sampling stage between two env-steps, fed by heads the caller evaluated, and the generalised advantage estimate after the
// last one.  The scalar logic is gl_actor.hpp's (instantiated on the host by tests/achost/achost.cpp); the env-steps in between are the
// caller's -- nothing of a step kernel is instantiated or touched here.
//
// ac_rows: lane = row, 256 per block, everything in registers: six means and a value in, Philox and three Box-Muller pairs, the sample,
// the clip and the log-probability, then 6 + 6 (+ 6) + 1 + 1 floats out per row.  The observation copy is the block's own: its 256
// rows are one contiguous span, copied with lane stride 1.  gae: lane = environment, 256 per block, the backward recurrence over t in
// registers, every access coalesced along b.  No LDS, no barrier, plain vector stores, no atomics.
#include <cmath>
#include <string>

#include "glgym_internal.h"

#include "gl_actor.hpp"

namespace {

constexpr int NU = GLGYM_NU;
constexpr int BLOCK = 256;

// grid = ceil(B / 256), lane = row b
__global__ __launch_bounds__(BLOCK) void ac_rows_kernel(glgym_ac_rows_args a)
{
    const int64_t b0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t b64 = b0 + threadIdx.x;
    if (a.value_only) {
        if (b64 < a.B) a.value[b64] = a.value_in[b64];
        return;
    }
    if (a.obs_out) {
        const int64_t n_row = a.B - b0 < BLOCK ? a.B - b0 : BLOCK;
        const size_t base = (size_t)b0 * (size_t)a.in_dim;
        const int n = (int)n_row * a.in_dim;                           // <= 256 * 1024
        for (int i = threadIdx.x; i < n; i += BLOCK) a.obs_out[base + i] = a.obs[base + i];
    }
    if (b64 >= a.B) return;
    const size_t b = (size_t)b64;
    float mean[NU], e[NU], sd[NU], ls[NU], act[NU], env[NU], logp;
#pragma unroll
    for (int j = 0; j < NU; ++j) { mean[j] = a.mean_in[b * NU + j]; sd[j] = a.std[j]; ls[j] = a.log_std[j]; }
    if (a.deterministic) {
#pragma unroll
        for (int j = 0; j < NU; ++j) e[j] = 0.0f;
    } else {
        const uint64_t D = a.draw_index + (a.draw_base ? *a.draw_base : 0ull);
        glactor::noise((uint32_t)b, (uint32_t)a.step, D, a.seed, e);
    }
    glactor::sample(mean, sd, ls, e, act, env, &logp);
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        a.action[b * NU + j] = act[j];
        a.action_env[b * NU + j] = env[j];
    }
    if (a.eps) {
#pragma unroll
        for (int j = 0; j < NU; ++j) a.eps[b * NU + j] = e[j];
    }
    a.logp[b] = logp;
    a.value[b] = a.value_in[b];
}

// grid = ceil(B / 256), lane = environment b
__global__ __launch_bounds__(256) void gae_kernel(glgym_gae_args a, float gamma, float lambda)
{
    const int64_t b64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b64 >= a.B) return;
    const size_t b = (size_t)b64;
    glactor::gae_env(a.T, (size_t)a.B, a.reward + b, a.done + b, a.value + b, a.last_value[b], gamma, lambda, a.advantage + b, a.returns + b);
}

// [p, p + n) and [q, q + m) share a byte
bool overlaps(const void* p, size_t n, const void* q, size_t m)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + m && b < a + n;
}

}  // namespace

extern "C" {

int glgym_ac_rows(glgym_handle h, const glgym_ac_rows_args* a, void* stream)
{
    if (!a) { g_err = "glgym_ac_rows: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_ac_rows", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->B < 1) { g_err = "glgym_ac_rows: B < 1"; return GLGYM_EINVAL; }
    if (a->B > INT32_MAX - (BLOCK - 1)) { g_err = "glgym_ac_rows: more than 2^31 - 256 rows"; return GLGYM_EINVAL; }
    if (a->step < 0) { g_err = "glgym_ac_rows: step < 0"; return GLGYM_EINVAL; }
    if ((a->deterministic != 0 && a->deterministic != 1) || (a->value_only != 0 && a->value_only != 1))
        return refuse("glgym_ac_rows: deterministic and value_only must be 0 or 1");
    if (!a->value_in || !a->value) { g_err = "glgym_ac_rows: null value_in or value"; return GLGYM_EINVAL; }
    if (!a->value_only) {
        if (!a->mean_in || !a->log_std || !a->std || !a->action || !a->action_env || !a->logp)
            return refuse("glgym_ac_rows: null mean_in, log_std, std, action, action_env or logp");
        if (a->obs_out) {
            if (a->in_dim < 1 || a->in_dim > glactor::MAX_IN) { g_err = "glgym_ac_rows: in_dim outside 1..1024"; return GLGYM_EINVAL; }
            if (!a->obs) { g_err = "glgym_ac_rows: null obs (obs_out copies it)"; return GLGYM_EINVAL; }
            const size_t obs_bytes = (size_t)a->B * (size_t)a->in_dim * sizeof(float);
            if (overlaps(a->obs_out, obs_bytes, a->obs, obs_bytes)) { g_err = "glgym_ac_rows: obs_out == obs, or overlaps it"; return GLGYM_EINVAL; }
        }
    }
    if (!h) { g_err = "glgym_ac_rows: null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    hipLaunchKernelGGL(ac_rows_kernel, dim3((unsigned)(((int64_t)a->B + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_gae(glgym_handle h, const glgym_gae_args* a, void* stream)
{
    if (!a) { g_err = "glgym_gae: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_gae", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->T < 1) { g_err = "glgym_gae: T < 1"; return GLGYM_EINVAL; }
    if (a->B < 1) { g_err = "glgym_gae: B < 1"; return GLGYM_EINVAL; }
    if (!(a->gamma >= 0.0 && a->gamma <= 1.0)) { g_err = "glgym_gae: gamma outside [0, 1] or not finite"; return GLGYM_EINVAL; }
    if (!(a->lambda >= 0.0 && a->lambda <= 1.0)) { g_err = "glgym_gae: lambda outside [0, 1] or not finite"; return GLGYM_EINVAL; }
    if (!a->reward || !a->done || !a->value || !a->last_value || !a->advantage || !a->returns)
        return refuse("glgym_gae: null reward, done, value, last_value, advantage or returns");
    const size_t n = (size_t)a->T * (size_t)a->B, nf = n * sizeof(float);
    const void* outs[2] = {a->advantage, a->returns};
    for (const void* o : outs)
        if (overlaps(o, nf, a->reward, nf) || overlaps(o, nf, a->done, n) || overlaps(o, nf, a->value, nf) ||
            overlaps(o, nf, a->last_value, (size_t)a->B * sizeof(float)))
            return refuse("glgym_gae: an output overlaps an input");
    if (overlaps(a->advantage, nf, a->returns, nf)) { g_err = "glgym_gae: advantage overlaps returns"; return GLGYM_EINVAL; }
    if (!h) { g_err = "glgym_gae: null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    hipLaunchKernelGGL(gae_kernel, dim3((unsigned)(((int64_t)a->B + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *a, (float)a->gamma, (float)a->lambda);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

}  // extern "C"
