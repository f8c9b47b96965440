// gl_actor.hpp -- the scalar logic of rollout collection (include/glgym.h glgym_ac_rows, glgym_gae), for host and device code alike: the
// Gaussian sampling stage for ONE row, given the means and the value its heads produced, and the generalised advantage estimate of ONE
// environment.
//   noise           e[0..5] of row b at step `step` of draw D: Philox4x32-10 (glcem::philox4x32_10), counter (b, 2 step + blk, lo32(D),
//                   hi32(D)) for blk = 0 | 1, key (lo32(seed), hi32(seed) ^ KEY_TAG); the eight words -> three Box-Muller pairs in
//                   double (glcem::normals: words 0..5), each rounded once to float32.  Nothing in it depends on the number of rows.
//   sample          a_j = mean_j + std_j * e_j; env_j = fminf(fmaxf(a_j, -1), 1) (a NaN reads as -1, as gl_mlp.hpp's squash);
//                   logp = s after s = 0 and, for j ascending, s = s + (((-0.5f * e_j) * e_j - log_std_j) - 0.9189385f).  Every
//                   operation a float32 operation of its own, in the order the brackets give.  No transcendental: std = exp(log_std)
//                   is the caller's.
//   gae_env         for t = T-1 .. 0:  nnt = 1 - (done[t] != 0);  nv = t == T-1 ? last_value : value[t+1];
//                       delta = (r[t] + (gamma * nv) * nnt) - value[t]
//                       adv   = delta + ((gamma * lambda) * nnt) * adv            (adv = 0 before t = T-1)
//                       ret[t] = adv + value[t]
//                   float32 throughout with gamma and lambda cast to float once; gamma * lambda is ONE float32 product, formed once;
//                   every other product and sum is rounded on its own, left to right inside the brackets as written.  This is
//                   stable_baselines3's RolloutBuffer.compute_returns_and_advantage with episode_starts[t+1] == done[t].
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "glgym.h"
#include "gl_cem.hpp"
#include "gl_plan.hpp"

namespace glactor {

using glplan::NU;
constexpr uint32_t KEY_TAG = 0x41435431u;        // "ACT1": apart from the CEM, scenario and weather-scenario streams
constexpr float HALF_LOG_2PI = 0.9189385f;       // 0.5 * log(2 pi) rounded to float32
constexpr int MAX_IN = 1024;                     // widest observation row obs_out copies

GLPLAN_HD void noise(uint32_t b, uint32_t step, uint64_t D, uint64_t seed, float e[NU])
{
    uint32_t r[8];
    for (uint32_t blk = 0; blk < 2; ++blk)
        glcem::philox4x32_10(b, 2u * step + blk, (uint32_t)D, (uint32_t)(D >> 32), (uint32_t)seed, (uint32_t)(seed >> 32) ^ KEY_TAG, r + 4 * blk);
    double d[NU];
    glcem::normals(r, d);
    for (int j = 0; j < NU; ++j) e[j] = (float)d[j];
}

GLPLAN_HD void sample(const float mean[NU], const float std_[NU], const float log_std[NU], const float e[NU], float a[NU], float a_env[NU],
                      float* logp)
{
#pragma clang fp contract(off)
    float s = 0.0f;
    for (int j = 0; j < NU; ++j) {
        const float prod = std_[j] * e[j];
        a[j] = mean[j] + prod;
        a_env[j] = fminf(fmaxf(a[j], -1.0f), 1.0f);          // a NaN reads as -1
        const float t0 = -0.5f * e[j];
        const float t1 = t0 * e[j];
        const float t2 = t1 - log_std[j];
        const float t3 = t2 - HALF_LOG_2PI;
        s = s + t3;
    }
    *logp = s;
}

// One environment: element t of a column is at [t * ld].  adv and ret must not alias an input.
GLPLAN_HD void gae_env(int T, size_t ld, const float* reward, const uint8_t* done, const float* value, float last_value, float gamma,
                       float lambda, float* adv_out, float* ret)
{
#pragma clang fp contract(off)
    const float gl = gamma * lambda;
    float adv = 0.0f, nv = last_value;               // nv: value[t+1], carried from the iteration before
    for (int t = T - 1; t >= 0; --t) {
        const float nnt = 1.0f - (done[(size_t)t * ld] ? 1.0f : 0.0f);
        const float v = value[(size_t)t * ld];
        const float p0 = gamma * nv;
        const float p1 = p0 * nnt;
        const float s0 = reward[(size_t)t * ld] + p1;
        const float delta = s0 - v;
        const float q0 = gl * nnt;
        const float q1 = q0 * adv;
        adv = delta + q1;
        adv_out[(size_t)t * ld] = adv;
        ret[(size_t)t * ld] = adv + v;
        nv = v;
    }
}

}  // namespace glactor
