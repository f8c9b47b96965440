// gl_envlayer.hpp -- the device functions of the env layer that TWO translation units inline: glgym_env.hip (obs_kernel, reset_kernel,
// crop_noise_kernel) and glgym.hip (the observation and auto-reset epilogues of step_kernel).  ONE definition each, so that both produce
// the same bits.  An edit in here changes the step kernels and owes their instruction-for-instruction comparison.
#pragma once
#include <hip/hip_runtime.h>

#include "gl_model.hpp"

namespace glenv {

using namespace glm;

// ---------------------------------------------------------------------------------------------------
// the 23 core observation features (observations.py:70-161), shared by obs_kernel and the observation epilogue of step_kernel
// ---------------------------------------------------------------------------------------------------
// j: 0 co2_ppm(x0,x2) 1 x2 2 RH(x15,x2) 3 x9 | 4 x21 5 x25 6 x26 | 7..12 u | 13 d0 14 d1 15 RH(d2,d1)
//    16 co2_ppm(d3,d1) 17 d4 | 18 timestep 19..22 sin/cos clocks
// prim: the feature's own input (x, u or weather column; unused from j = 18), aux: tAir (j < 13) or tOut.  ts: the env's timestep AFTER
// the step's increment; the row / "timestep" the reference shows is the pre-increment one, k = ts - 1 (0 for a freshly reset env).
// Straight-line selects: with a run-time j (obs_kernel) no branch per feature, with a compile-time j (step_kernel) everything but the
// feature's own arithmetic folds away.  ONE definition, so that both kernels produce the same bits.
constexpr int OBS_NCORE = 23;
__device__ __forceinline__ float obs_core_feature(int j, float prim, float aux, float sday, int ts, double doy_inc, double hod_inc)
{
    // No implicit contraction in here: which products the compiler fuses into a following add depends on the caller -- with a
    // compile-time j it turned rev - floor(rev) into fma(t, c, -floor(t * c)), which is not 0 where rev is a whole number (step 96 of
    // an episode), with a run-time j it did not.  The one fused operation obs_kernel has always had is written out.
#pragma clang fp contract(off)
    const float kPpm = (float)(8.3144598 / (101325.0 * 44.01e-3));
    const int k = ts > 0 ? ts - 1 : 0;
    // fp32 hardware transcendentals: the observation block is float32 (observation_space dtype)
    const float sat = 610.78f * __builtin_amdgcn_exp2f(1.44269504f * 17.2694f * aux * __builtin_amdgcn_rcpf(aux + 238.3f));
    const float rh = fminf(fmaxf(100.0f * prim * __builtin_amdgcn_rcpf(sat), 0.0f), 100.0f);
    const float ppm = kPpm * (aux + 273.15f) * prim;
    // v_sin_f32 / v_cos_f32 take revolutions: sin(2*pi*x)   (tomato_env.py:126-128)
    const int c = j - 18;
    const double rev = (c <= 2) ? __builtin_fma((double)ts, doy_inc, (double)sday) * (1.0 / 365.0)
                                : (double)ts * hod_inc * (1.0 / 24.0);
    const float fr = (float)(rev - floor(rev));
    const float clk = (c == 1 || c == 3) ? __builtin_amdgcn_sinf(fr) : __builtin_amdgcn_cosf(fr);
    float v = prim;
    v = (j == 0 || j == 16) ? ppm : v;
    v = (j == 2 || j == 15) ? rh : v;
    v = (j == 18) ? (float)k : v;
    v = (j > 18) ? clk : v;
    return v;
}
// module (GLGYM_OBS_*) and column inside it of core feature j
__device__ __forceinline__ constexpr int obs_core_module(int j) { return j < 4 ? 0 : j < 7 ? 1 : j < 13 ? 2 : j < 18 ? 3 : 4; }
__device__ __forceinline__ constexpr int obs_core_col(int j) { return j < 4 ? j : j < 7 ? j - 4 : j < 13 ? j - 7 : j < 18 ? j - 13 : j - 18; }

// counter-based generator shared by the reset (episode start draw) and crop-noise kernels
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned* out)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ---------------------------------------------------------------------------------------------------
// one environment's reset: the episode start draw and init_state (utils.py:13-46) -- reset_kernel's body, shared with the auto-reset
// epilogue of step_kernel.  ONE definition, so that both produce the same bits.
// ---------------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void reset_env(int b, int ld, T* x, T* u, int* timestep, const T* weather, int weather_rows, int* w_off,
                                          const int* start_rows, const float* start_days, int n_starts, float* start_day, int* episode,
                                          unsigned long long seed, int nd)
{
    // No implicit contraction in here (obs_core_feature): the two fused operations reset_kernel has always had are written out.
#pragma clang fp contract(off)
    if (start_rows && n_starts > 0) {            // draw this episode's start (tomato_env.py:236-244)
        const int ep = episode ? episode[b] : 0;
        unsigned rnd[4];
        philox4x32_10((unsigned)b, (unsigned)ep, 0x5eedu, 0u, (unsigned)seed, (unsigned)(seed >> 32), rnd);
        const int j = (int)(rnd[0] % (unsigned)n_starts);
        w_off[b] = start_rows[j];
        if (start_day && start_days) start_day[b] = start_days[j];
        if (episode) episode[b] = ep + 1;
    }
    int r = w_off[b];
    r = r < 0 ? 0 : (r >= weather_rows ? weather_rows - 1 : r);
    const double co2Out = (double)weather[(size_t)r * nd + 3], tSoOut = (double)weather[(size_t)r * nd + 6];
    const double tAir = 16.5;
    double xi[NX];
    xi[0] = xi[1] = co2Out;
    for (int i = 2; i <= 10; ++i) xi[i] = tAir;
    xi[4] = tAir + 4;
    xi[11] = 0.25 * (3.0 * tAir + tSoOut);
    xi[12] = 0.25 * __builtin_fma(2.0, tSoOut, 2.0 * tAir);
    xi[13] = 0.25 * __builtin_fma(3.0, tSoOut, tAir);
    xi[14] = tSoOut;
    xi[15] = xi[16] = 90.0 / 100.0 * (610.78 * exp(17.2694 * tAir / (tAir + 238.3)));
    xi[17] = xi[18] = xi[19] = xi[20] = tAir;
    xi[21] = xi[4];
    xi[22] = 0.0; xi[23] = 9.5283e4; xi[24] = 2.5107e5; xi[25] = 5.5338e4; xi[26] = 3.0978e3; xi[27] = 0.0;
    for (int i = 0; i < NX; ++i) x[(size_t)i * ld + b] = T(xi[i]);
    for (int j = 0; j < NU; ++j) u[(size_t)j * ld + b] = T(0);
    timestep[b] = 0;
}

#ifndef GL_OBS_ROWS
#define GL_OBS_ROWS 16
#endif
constexpr int OBS_ROWS = GL_OBS_ROWS;      // env rows per span: obs_kernel and the step kernels' observation epilogue

}  // namespace glenv
