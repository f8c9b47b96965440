// gl_sac.hpp -- the scalar logic of soft actor-critic (include/glgym.h glgym_sac_rows, glgym_sac_rows_grad, glgym_sac_batch,
// glgym_sac_loss, glgym_polyak), for host and device code alike: the tanh-squashed Gaussian of ONE row with its reparameterised backward
// pass, the replay ring's sampling index, the critic and actor terms of ONE row, the Polyak update of ONE element, and (gl_ppo.hpp's) the
// order in which a lane, a wavefront, a block and the finishing launch add up the rows' terms.  tests/sachost/sachost.cpp instantiates it
// on the host.
//   noise           e[0..5] (and e2[0..5]) of row key k = (uint32)(row0 + r) at step `step` of draw D: Philox4x32-10, counter
//                   (k, 4 step + blk, lo32(D), hi32(D)), key (lo32(seed), hi32(seed) ^ KEY_TAG); blk = 0 | 1 -> e as glactor::noise
//                   (glcem::normals on the eight words, words 0..5, each rounded once to float32), blk = 2 | 3 -> e2 the same way.
//   uniform         a_j = (float)(2.0 * ((double) r_j + 0.5) * 2^-32 - 1.0), r_0..r_5 the first six words of blocks 0 and 1.
//   squash          float32, every operation rounded on its own, j ascending:
//                     ls = fminf(fmaxf(log_std_j, -20), 2);  std = (float) exp((double) ls)
//                     u  = mean + std * e;                     a   = (float) tanh((double) u)
//                     c  = (1 - a * a) + 1e-6f;                l   = (float) log((double) c)
//                     logp = s after s = 0, j ascending s = s + (((-0.5f * e) * e - ls) - 0.9189385f), then j ascending s = s - l_j
//                     env = fminf(fmaxf(a, -1), 1), or with sigma > 0 fminf(fmaxf(a + sigma * e2, -1), 1): a NaN reads as -1
//   squash_grad     g = 1 - a * a;  grad_u = grad_action * g + grad_logp * (((2 * a) * g) / (g + 1e-6f))
//                   grad_mean = grad_u;  grad_log_std = (grad_u * (std * e)) - grad_logp where -20 <= log_std_in <= 2, else 0
//   sample_index    w = word0 * 2^32 + word1 of counter (p, 0, lo32(D), hi32(D)) under key (lo32(seed), hi32(seed) ^ SAMPLE_TAG);
//                   idx = the high 64 bits of w * n, n = n_valid * B;  slot = (head + idx / B) mod S;  b = idx mod B
//   critic_row, actor_row, finish_*: see include/glgym.h; alpha = exp(log_alpha) is the caller's.
//   polyak          t = ((1 - tau) * t) + (tau * s), 1 - tau one float32 difference formed once, the products rounded separately.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "glgym.h"
#include "gl_actor.hpp"
#include "gl_cem.hpp"
#include "gl_plan.hpp"
#include "gl_ppo.hpp"

namespace glsac {

using glplan::NU;
using glplan::WAVE;
using glactor::HALF_LOG_2PI;
using glppo::BLOCK;
using glppo::MAX_BLOCKS;
using glppo::N_WAVE;
using glppo::n_blocks;

constexpr uint32_t KEY_TAG = 0x53414331u;        // "SAC1": the squashed actor's noise
constexpr uint32_t SAMPLE_TAG = 0x534d5031u;     // "SMP1": the replay ring's sampling
constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f, SQUASH_EPS = 1e-6f;
constexpr int MAX_IN = glactor::MAX_IN;
constexpr int MAX_TENSORS = 64;
constexpr int N_SUM = 5;                         // critic: (q1-y)^2, (q2-y)^2, q1, q2, y; actor: alpha logp - min q, logp + target entropy, logp
enum { C_SQ1 = 0, C_SQ2, C_Q1, C_Q2, C_Y, A_LOSS = 0, A_ENT = 1, A_LOGP = 2 };
constexpr size_t LOSS_WS_BYTES = (size_t)MAX_BLOCKS * N_SUM * sizeof(double);        // 40 960

// ---- noise --------------------------------------------------------------------------------------------------------------------------------
GLPLAN_HD void words(uint32_t k, uint32_t step, uint32_t blk0, uint64_t D, uint64_t seed, uint32_t r[8])
{
    for (uint32_t blk = 0; blk < 2; ++blk)
        glcem::philox4x32_10(k, 4u * step + blk0 + blk, (uint32_t)D, (uint32_t)(D >> 32), (uint32_t)seed, (uint32_t)(seed >> 32) ^ KEY_TAG,
                             r + 4 * blk);
}

// blk0 = 0: e, blk0 = 2: e2
GLPLAN_HD void noise(uint32_t k, uint32_t step, uint32_t blk0, uint64_t D, uint64_t seed, float e[NU])
{
    uint32_t r[8];
    words(k, step, blk0, D, seed, r);
    double d[NU];
    glcem::normals(r, d);
    for (int j = 0; j < NU; ++j) e[j] = (float)d[j];
}

GLPLAN_HD void uniform(uint32_t k, uint32_t step, uint64_t D, uint64_t seed, float a[NU])
{
#pragma clang fp contract(off)
    uint32_t r[8];
    words(k, step, 0, D, seed, r);
    for (int j = 0; j < NU; ++j) {
        const double u = ((double)r[j] + 0.5) * glcem::TWO_M32;
        const double t = 2.0 * u;
        a[j] = (float)(t - 1.0);
    }
}

// ---- the squashed Gaussian -------------------------------------------------------------------------------------------------------------
GLPLAN_HD float clamp_ls(float log_std) { return fminf(fmaxf(log_std, LOG_STD_MIN), LOG_STD_MAX); }
GLPLAN_HD float std_of(float ls) { return (float)std::exp((double)ls); }
GLPLAN_HD float tanh_of(float u) { return (float)std::tanh((double)u); }
GLPLAN_HD float log_of(float c) { return (float)std::log((double)c); }

GLPLAN_HD float u_of(float mean, float sd, float e)
{
#pragma clang fp contract(off)
    const float p = sd * e;
    return mean + p;
}

GLPLAN_HD float c_of(float a)
{
#pragma clang fp contract(off)
    const float aa = a * a;
    const float g = 1.0f - aa;
    return g + SQUASH_EPS;
}

GLPLAN_HD float logp_of(const float e[NU], const float ls[NU], const float l[NU])
{
#pragma clang fp contract(off)
    float s = 0.0f;
    for (int j = 0; j < NU; ++j) {
        const float t0 = -0.5f * e[j];
        const float t1 = t0 * e[j];
        const float t2 = t1 - ls[j];
        const float t3 = t2 - HALF_LOG_2PI;
        s = s + t3;
    }
    for (int j = 0; j < NU; ++j) s = s - l[j];
    return s;
}

// sigma > 0: a + sigma * e2, then the clip; a NaN reads as -1
GLPLAN_HD float env_of(float a, float sigma, float e2)
{
#pragma clang fp contract(off)
    float v = a;
    if (sigma > 0.0f) {
        const float p = sigma * e2;
        v = a + p;
    }
    return fminf(fmaxf(v, -1.0f), 1.0f);
}

GLPLAN_HD void squash_grad(float grad_action, float grad_logp, float e, float sd, float a, float log_std_in, float* grad_mean, float* grad_log_std)
{
#pragma clang fp contract(off)
    const float aa = a * a;
    const float g = 1.0f - aa;
    const float t0 = grad_action * g;
    const float t1 = 2.0f * a;
    const float t2 = t1 * g;
    const float t3 = g + SQUASH_EPS;
    const float t4 = t2 / t3;
    const float t5 = grad_logp * t4;
    const float gu = t0 + t5;
    *grad_mean = gu;
    const float p = sd * e;
    const float q = gu * p;
    const float r = q - grad_logp;
    *grad_log_std = (log_std_in >= LOG_STD_MIN && log_std_in <= LOG_STD_MAX) ? r : 0.0f;
}

// ---- the replay ring ---------------------------------------------------------------------------------------------------------------------
GLPLAN_HD uint64_t mulhi64(uint64_t a, uint64_t b)
{
    const uint64_t a0 = a & 0xffffffffull, a1 = a >> 32, b0 = b & 0xffffffffull, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// position p of draw D -> idx in [0, n)
GLPLAN_HD uint64_t sample_index(uint32_t p, uint64_t n, uint64_t D, uint64_t seed)
{
    uint32_t f[4];
    glcem::philox4x32_10(p, 0u, (uint32_t)D, (uint32_t)(D >> 32), (uint32_t)seed, (uint32_t)(seed >> 32) ^ SAMPLE_TAG, f);
    const uint64_t w = ((uint64_t)f[0] << 32) | (uint64_t)f[1];
    return mulhi64(w, n);
}

// idx -> the flat rows (slot * B + b) of the transition and of its successor observation
GLPLAN_HD void ring_rows(uint64_t idx, int S, int B, int head, uint32_t* row, uint32_t* next_row)
{
    const uint64_t q = idx / (uint64_t)B, b = idx - q * (uint64_t)B;
    const uint64_t slot = ((uint64_t)head + q) % (uint64_t)S;
    const uint64_t nxt = (slot + 1) % (uint64_t)S;
    *row = (uint32_t)(slot * (uint64_t)B + b);
    *next_row = (uint32_t)(nxt * (uint64_t)B + b);
}

// ---- the losses --------------------------------------------------------------------------------------------------------------------------
struct Sums {
    double s[N_SUM];
};

GLPLAN_HD void sums_init(Sums& a)
{
    for (int k = 0; k < N_SUM; ++k) a.s[k] = 0.0;
}

struct Hyper {
    float w, nw, gamma, te;
};

GLPLAN_HD Hyper hyper(int M, double gamma, double target_entropy)
{
    Hyper h;
    h.w = (float)(1.0 / (double)M);
    h.nw = -h.w;
    h.gamma = (float)gamma;
    h.te = (float)target_entropy;
    return h;
}

struct CriticRow {
    float y, g1, g2;
};

GLPLAN_HD void critic_row(const Hyper& h, float alpha, float q1, float q2, float q1n, float q2n, float logp_n, float r, uint8_t done, CriticRow& o,
                          Sums& acc)
{
#pragma clang fp contract(off)
    const float m = fminf(q1n, q2n);
    const float t0 = alpha * logp_n;
    const float t1 = m - t0;
    const float nd = 1.0f - (done ? 1.0f : 0.0f);
    const float k = nd * h.gamma;
    const float t2 = k * t1;
    o.y = r + t2;
    const float d1 = q1 - o.y, d2 = q2 - o.y;
    o.g1 = h.w * d1;
    o.g2 = h.w * d2;
    const float s1 = d1 * d1, s2 = d2 * d2;
    acc.s[C_SQ1] = acc.s[C_SQ1] + (double)s1;
    acc.s[C_SQ2] = acc.s[C_SQ2] + (double)s2;
    acc.s[C_Q1] = acc.s[C_Q1] + (double)q1;
    acc.s[C_Q2] = acc.s[C_Q2] + (double)q2;
    acc.s[C_Y] = acc.s[C_Y] + (double)o.y;
}

struct ActorRow {
    float g1, g2;
};

GLPLAN_HD void actor_row(const Hyper& h, float alpha, float q1p, float q2p, float logp, ActorRow& o, Sums& acc)
{
#pragma clang fp contract(off)
    const bool first = q1p <= q2p;
    o.g1 = first ? h.nw : 0.0f;
    o.g2 = first ? 0.0f : h.nw;
    const float t0 = alpha * logp;
    const float mn = fminf(q1p, q2p);
    const float ta = t0 - mn;
    const float te = logp + h.te;
    acc.s[A_LOSS] = acc.s[A_LOSS] + (double)ta;
    acc.s[A_ENT] = acc.s[A_ENT] + (double)te;
    acc.s[A_LOGP] = acc.s[A_LOGP] + (double)logp;
}

// stats [8] of the critic stage from the finished sums
GLPLAN_HD void critic_stats(const double* S, int M, float alpha, double stats[8])
{
#pragma clang fp contract(off)
    const double m = (double)M;
    const double both = S[C_SQ1] + S[C_SQ2];
    const double half = 0.5 * both;
    stats[0] = half / m;
    stats[1] = S[C_SQ1] / m;
    stats[2] = S[C_SQ2] / m;
    stats[3] = S[C_Q1] / m;
    stats[4] = S[C_Q2] / m;
    stats[5] = S[C_Y] / m;
    stats[6] = (double)alpha;
    stats[7] = m;
}

// stats [8] of the actor stage and the gradient of the entropy coefficient's loss with respect to log_alpha
GLPLAN_HD void actor_stats(const double* S, int M, float alpha, float log_alpha, double stats[8], float* grad_log_alpha)
{
#pragma clang fp contract(off)
    const double m = (double)M;
    const double mean_e = S[A_ENT] / m;
    const double prod = (double)log_alpha * mean_e;
    stats[0] = S[A_LOSS] / m;
    stats[1] = -prod;
    stats[2] = -mean_e;
    stats[3] = S[A_LOGP] / m;
    stats[4] = (double)alpha;
    stats[5] = (double)log_alpha;
    stats[6] = 0.0;
    stats[7] = m;
    *grad_log_alpha = (float)(-mean_e);
}

// ---- Polyak --------------------------------------------------------------------------------------------------------------------------------
GLPLAN_HD float polyak(float t, float s, float tau, float omt)
{
#pragma clang fp contract(off)
    const float p0 = omt * t;
    const float p1 = tau * s;
    return p0 + p1;
}

}  // namespace glsac
