// glgym_rng.hip -- the kernels of rng = "numpy" and their C entry points (glgym_rng_crop_noise, glgym_rng_reset_draw): each
// environment's own PCG64 stream (gl_pcg64.hpp) on the device, drawing what the reference's TomatoEnv draws from its NumPy generator,
// in the same order and bit for bit.
//
// Layout: one lane per environment.  The stream state is the caller's SoA buffer uint64 [5][ld] (state lo / hi, inc lo / hi, buffer
// word), so adjacent lanes read adjacent addresses; the increment is read only.  All arithmetic is 64-bit integer and fp64 on the
// vector unit; no LDS, no atomics, no scalar-memory stores.
#include "glgym_internal.h"

#include "gl_pcg64.hpp"

namespace {

constexpr int NCROP = glpcg::NDRAW_STEP, CROP0 = 128;

// parametric_crop_uncertainty (noise.py:16-22) for every environment: 34 uniforms, p_i <- float32(double(p_i) + noise_i * double(p_i)),
// then cLeafMax = laiMax / sla in float32.  Entries are written as they are drawn (no per-lane array): 141 and 142 are kept for 144.
template <class T>
__global__ __launch_bounds__(256) void rng_crop_noise_kernel(T* __restrict__ crop_p, int B, int ld, const float* __restrict__ p0,
                                                             double scale, uint64_t* __restrict__ rng_state)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    glpcg::Pcg64 g;
    g.load(rng_state, (size_t)ld, (size_t)b);
    if (crop_p == nullptr) {                    // uncertainty_scale == 0: the reference draws all the same (tomato_env.py:118)
        constexpr glpcg::AdvanceConsts jump = glpcg::advance_consts(glpcg::NDRAW_STEP);      // a^34 and 1 + a + .. + a^33
        g.advance(jump);
        g.store(rng_state, (size_t)ld, (size_t)b);
        return;
    }
    const double lo = -scale / 2, hi = scale / 2;
    float lai_max = 0.f, sla = 1.f;
    for (int i = 0; i < NCROP; ++i) {
        const float v = glpcg::crop_entry(g, p0[i], lo, hi);
        if (i == 141 - CROP0) lai_max = v;
        if (i == 142 - CROP0) sla = v;
        if (i != 144 - CROP0) crop_p[(size_t)i * ld + b] = T(v);
    }
    crop_p[(size_t)(144 - CROP0) * ld + b] = T(lai_max / sla);
    g.store(rng_state, (size_t)ld, (size_t)b);
}

// TomatoEnv.reset's draws (tomato_env.py:236-241): choice(years), then choice(days); the start table is year-major.
__global__ __launch_bounds__(256) void rng_reset_draw_kernel(int B, int ld, const unsigned char* __restrict__ mask,
                                                             uint64_t* __restrict__ rng_state, int n_years, int n_days,
                                                             const int* __restrict__ start_rows, const float* __restrict__ start_days,
                                                             int* __restrict__ w_off, float* __restrict__ start_day)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (mask && !mask[b])) return;
    glpcg::Pcg64 g;
    g.load(rng_state, (size_t)ld, (size_t)b);
    const uint32_t iy = g.bounded((uint64_t)n_years);
    const uint32_t id = g.bounded((uint64_t)n_days);
    g.store(rng_state, (size_t)ld, (size_t)b);
    const size_t j = (size_t)iy * (size_t)n_days + id;
    w_off[b] = start_rows[j];
    if (start_day && start_days) start_day[b] = start_days[j];
}

}  // namespace

extern "C" {

int glgym_rng_crop_noise(glgym_handle h, void* crop_p, int B, int ld, double scale, uint64_t* rng_state, void* stream)
{
    DeviceGuard dev_guard(h);
    if (!h || !rng_state || B < 1 || ld < B || !(scale >= 0.0)) {
        g_err = "glgym_rng_crop_noise: bad arguments (null handle or stream buffer, ld < B, or a negative scale)";
        return GLGYM_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    with_dtype(h->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(rng_crop_noise_kernel<T>, dim3((B + 255) / 256), dim3(256), 0, st, (T*)crop_p, B, ld, h->p0_crop_dev, scale, rng_state);
    });
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_rng_reset_draw(glgym_handle h, int B, int ld, const unsigned char* mask, uint64_t* rng_state, int n_years, int n_days,
                         const int32_t* start_rows, const float* start_days, int32_t* w_off, float* start_day, void* stream)
{
    DeviceGuard dev_guard(h);
    if (!h || !rng_state || B < 1 || ld < B || n_years < 1 || n_days < 1 || !start_rows || !w_off) {
        g_err = "glgym_rng_reset_draw: bad arguments (null pointer, ld < B, or an empty start grid)";
        return GLGYM_EINVAL;
    }
    hipLaunchKernelGGL(rng_reset_draw_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, B, ld, mask, rng_state, n_years, n_days,
                       start_rows, start_days, w_off, start_day);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

}  // extern "C"
