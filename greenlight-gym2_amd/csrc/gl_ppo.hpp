// gl_ppo.hpp -- the scalar logic of the PPO update (include/glgym.h glgym_ppo_batch, glgym_ppo_loss), for host and device code alike:
// the seeded permutation behind a minibatch, the clipped-surrogate loss of ONE row with its gradients, and the order in which a lane,
// a wavefront, a block and the finishing launch add up the rows' terms.  tests/ppohost/ppohost.cpp instantiates it on the host: a lane is
// a pass of a loop, a butterfly a loop over an array of 64.
//   perm            position p in [0, N) -> flat transition index in [0, N).  w = the smallest even bit count >= 2 with 2^w >= N, half =
//                   w / 2, mask = 2^half - 1.  P(x) on [0, 2^w): L = x >> half, R = x & mask; four rounds r = 0..3 of
//                   (L, R) = (R, L ^ (F(r, R) & mask)); P = (L << half) | R.  F(r, R) = word 0 of glcem::philox4x32_10 with counter
//                   (R, r, lo32(D), hi32(D)) and key (lo32(seed), hi32(seed) ^ KEY_TAG).  perm(p): y = P(p); while y >= N: y = P(y)
//                   (cycle walking: P is a bijection, so the walk ends, and 2^w < 4 N keeps the expected number of walks below 4).
//                   It depends on (seed, D, N) only.
//   logp_of, ratio_of, finish_row
//                   float32, every operation rounded on its own, in this order (c = clip_range, cv = clip_range_vf, w = (float)(1.0 / M)):
//                     z_j    = (a_j - mean_j) * inv_std_j
//                     logp   = s after s = 0 and, j ascending, s = s + (((-0.5f * z_j) * z_j - log_std_j) - 0.9189385f)   (glactor::sample)
//                     d      = logp - old_logp;  ratio = (float) exp((double) d)            -- the one transcendental, in double
//                     A      = adv, or (adv - (float) mu) / ((float) sd + 1e-8f)             -- one float32 division
//                     s1     = ratio * A;  rc = fminf(fmaxf(ratio, 1 - c), 1 + c);  s2 = rc * A;  surrogate = fminf(s1, s2)
//                     q      = s1 <= s2 ? (-w) * s1 : 0                                      -- what min's and clamp's backward add up to
//                     grad_mean_j = q * (z_j * inv_std_j);  log_std term_j = q * (z_j * z_j - 1)
//                     vp     = value, or old_v + fminf(fmaxf(value - old_v, -cv), cv);  value term = (ret - vp) * (ret - vp)
//                     grad_value = ((vf_coef * 2) * w) * (vp - ret), or 0 where value - old_v lies outside [-cv, cv]
//                     kl term = (ratio - 1) - d;  clip term = |ratio - 1| > c ? 1 : 0
//                   fminf / fmaxf return their other operand for a NaN: a row whose ratio is NaN has NaN gradients, NaN kl and ratio terms,
//                   and the surrogate (1 - c) * A.
//   n_blocks, Sums  the reduction.  Rows are cut into chunks of 256; nb = min(ceil(M / 256), 1024) blocks; block b takes chunks b, b + nb,
//                   ...; lane t of the block takes row 256 chunk + t of each of them, ascending, and adds its terms in double from 0.  The
//                   64 lanes of a wavefront combine by the butterfly of gl_plan.hpp (xor 32, 16, .. 1: v = v + other), the four
//                   wavefronts of a block in index order ((w0 + w1) + w2) + w3, and the finishing launch adds the blocks' partials in block
//                   order from block 0.  The largest ratio goes the same way with max in place of + (a NaN wins).  Nothing depends on the
//                   device: the host build and NumPy reproduce every sum to the last bit.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

#include "glgym.h"
#include "gl_actor.hpp"
#include "gl_cem.hpp"
#include "gl_plan.hpp"

namespace glppo {

using glplan::NU;
using glplan::WAVE;
using glactor::HALF_LOG_2PI;

constexpr uint32_t KEY_TAG = 0x50524d31u;        // "PRM1": apart from the CEM, scenario, weather-scenario and ACT1 streams
constexpr int BLOCK = 256;                       // rows of a chunk = lanes of a block
constexpr int N_WAVE = BLOCK / WAVE;
constexpr int MAX_BLOCKS = 1024;                 // the grid's cap: beyond 262 144 rows a block takes more than one chunk
constexpr int MAX_IN = glactor::MAX_IN;
// the loss's sums: a block's partials are ws[block][N_SUM], the batch's ws[block][N_ADV]
enum { S_SURR = 0, S_VALUE, S_KL, S_CLIP, S_MAXRATIO, S_LS0, N_SUM = S_LS0 + NU };
constexpr int N_ADV = 2;
constexpr size_t LOSS_WS_BYTES = (size_t)MAX_BLOCKS * N_SUM * sizeof(double);        // 90 112
constexpr size_t BATCH_WS_BYTES = (size_t)MAX_BLOCKS * N_ADV * sizeof(double);       // 16 384

// ---- the permutation -------------------------------------------------------------------------------------------------------------------
GLPLAN_HD int half_bits(uint32_t N)
{
    int w = 2;
    while (((uint64_t)1 << w) < (uint64_t)N) w += 2;
    return w / 2;
}

GLPLAN_HD uint32_t feistel(uint32_t x, int half, uint64_t D, uint64_t seed, uint32_t tag)
{
    const uint32_t mask = ((uint32_t)1 << half) - 1u;
    uint32_t L = x >> half, R = x & mask;
    for (uint32_t r = 0; r < 4; ++r) {
        uint32_t f[4];
        glcem::philox4x32_10(R, r, (uint32_t)D, (uint32_t)(D >> 32), (uint32_t)seed, (uint32_t)(seed >> 32) ^ tag, f);
        const uint32_t nr = L ^ (f[0] & mask);
        L = R;
        R = nr;
    }
    return (L << half) | R;
}

GLPLAN_HD uint32_t perm(uint32_t p, uint32_t N, int half, uint64_t D, uint64_t seed, uint32_t tag = KEY_TAG)
{
    uint32_t y = feistel(p, half, D, seed, tag);
    while (y >= N) y = feistel(y, half, D, seed, tag);
    return y;
}

// ---- the reduction's shape ---------------------------------------------------------------------------------------------------------------
GLPLAN_HD int n_blocks(int64_t M)
{
    const int64_t c = (M + BLOCK - 1) / BLOCK;
    return (int)(c < MAX_BLOCKS ? c : MAX_BLOCKS);
}

// a NaN wins, otherwise the larger: symmetric, so every lane of a butterfly ends with the same value
GLPLAN_HD double nanmax(double a, double b)
{
    if (a != a) return a;
    if (b != b) return b;
    return a > b ? a : b;
}

struct Sums {
    double s[N_SUM];
};

GLPLAN_HD void sums_init(Sums& a)
{
    for (int k = 0; k < N_SUM; ++k) a.s[k] = 0.0;
    a.s[S_MAXRATIO] = -std::numeric_limits<double>::infinity();
}

GLPLAN_HD double combine(int k, double a, double b) { return k == S_MAXRATIO ? nanmax(a, b) : a + b; }

// ---- advantage statistics ----------------------------------------------------------------------------------------------------------------
// what a row adds to S1 and S2
GLPLAN_HD void adv_terms(float adv, double t[N_ADV])
{
#pragma clang fp contract(off)
    const double a = (double)adv;
    t[0] = a;
    t[1] = a * a;
}

// mean and unbiased standard deviation from the finished sums
GLPLAN_HD void adv_stats_of(double S1, double S2, int M, double out[2])
{
#pragma clang fp contract(off)
    const double m = (double)M;
    const double sq = S1 * S1;
    const double corr = sq / m;
    const double num = S2 - corr;
    double var = num / (m - 1.0);
    if (var < 0.0) var = 0.0;
    out[0] = S1 / m;
    out[1] = std::sqrt(var);
}

// ---- the loss -----------------------------------------------------------------------------------------------------------------------------
struct Hyper {
    float w, nw, c, lo, hi, cv, ncv, kv, ent, vf;
    int vclip;
};

GLPLAN_HD Hyper hyper(int M, double clip_range, double clip_range_vf, double vf_coef, double ent_coef)
{
#pragma clang fp contract(off)
    Hyper h;
    h.w = (float)(1.0 / (double)M);
    h.nw = -h.w;
    h.c = (float)clip_range;
    h.lo = 1.0f - h.c;
    h.hi = 1.0f + h.c;
    h.vclip = clip_range_vf > 0.0 ? 1 : 0;
    h.cv = h.vclip ? (float)clip_range_vf : 0.0f;
    h.ncv = -h.cv;
    h.vf = (float)vf_coef;
    h.ent = (float)ent_coef;
    const float vf2 = h.vf * 2.0f;
    h.kv = vf2 * h.w;
    return h;
}

// the advantage normalisation of a call: A = (adv - mu) / sdp
struct Norm {
    int on;
    float mu, sdp;
};

GLPLAN_HD Norm norm_of(const double* adv_stats)
{
#pragma clang fp contract(off)
    Norm n{0, 0.0f, 1.0f};
    if (adv_stats) {
        n.on = 1;
        n.mu = (float)adv_stats[0];
        n.sdp = (float)adv_stats[1] + 1e-8f;
    }
    return n;
}

GLPLAN_HD float logp_of(const float mean[NU], const float act[NU], const float inv_std[NU], const float log_std[NU], float z[NU])
{
#pragma clang fp contract(off)
    float s = 0.0f;
    for (int j = 0; j < NU; ++j) {
        const float d0 = act[j] - mean[j];
        z[j] = d0 * inv_std[j];
        const float t0 = -0.5f * z[j];
        const float t1 = t0 * z[j];
        const float t2 = t1 - log_std[j];
        const float t3 = t2 - HALF_LOG_2PI;
        s = s + t3;
    }
    return s;
}

GLPLAN_HD float ratio_of(float logp, float old_logp)
{
#pragma clang fp contract(off)
    const float d = logp - old_logp;
    return (float)std::exp((double)d);
}

struct Row {
    float grad_mean[NU], ls_term[NU], grad_value, surr, vterm, kl, clipped;
};

// everything of a row behind its ratio.  old_v is looked at only with h.vclip.
GLPLAN_HD void finish_row(const Hyper& h, const Norm& n, const float z[NU], const float inv_std[NU], float logp, float old_logp, float ratio,
                          float adv, float value, float old_v, float ret, Row& o)
{
#pragma clang fp contract(off)
    const float d = logp - old_logp;
    float A = adv;
    if (n.on) {
        const float c0 = adv - n.mu;
        A = c0 / n.sdp;
    }
    const float s1 = ratio * A;
    const float rc = fminf(fmaxf(ratio, h.lo), h.hi);
    const float s2 = rc * A;
    o.surr = fminf(s1, s2);
    float q = 0.0f;
    if (s1 <= s2) q = h.nw * s1;
    for (int j = 0; j < NU; ++j) {
        const float g0 = z[j] * inv_std[j];
        o.grad_mean[j] = q * g0;
        const float l0 = z[j] * z[j];
        const float l1 = l0 - 1.0f;
        o.ls_term[j] = q * l1;
    }
    float vp = value;
    bool pass = true;
    if (h.vclip) {
        const float dv = value - old_v;
        pass = dv >= h.ncv && dv <= h.cv;
        const float cl = fminf(fmaxf(dv, h.ncv), h.cv);
        vp = old_v + cl;
    }
    const float e0 = ret - vp;
    o.vterm = e0 * e0;
    const float e1 = vp - ret;
    o.grad_value = pass ? h.kv * e1 : 0.0f;
    const float r1 = ratio - 1.0f;
    o.kl = r1 - d;
    o.clipped = fabsf(r1) > h.c ? 1.0f : 0.0f;
}

// what a lane adds for one row
GLPLAN_HD void sums_add(Sums& a, const Row& o, float ratio)
{
    a.s[S_SURR] = a.s[S_SURR] + (double)o.surr;
    a.s[S_VALUE] = a.s[S_VALUE] + (double)o.vterm;
    a.s[S_KL] = a.s[S_KL] + (double)o.kl;
    a.s[S_CLIP] = a.s[S_CLIP] + (double)o.clipped;
    a.s[S_MAXRATIO] = nanmax(a.s[S_MAXRATIO], (double)ratio);
    for (int j = 0; j < NU; ++j) a.s[S_LS0 + j] = a.s[S_LS0 + j] + (double)o.ls_term[j];
}

// stats [8] and grad_log_std [6] from the finished sums S [N_SUM]
GLPLAN_HD void loss_stats(const double* S, int M, const Hyper& h, const float log_std[NU], double stats[8], float grad_log_std[NU])
{
#pragma clang fp contract(off)
    const double m = (double)M;
    const double mean_surr = S[S_SURR] / m;
    const double policy = -mean_surr;
    const double value_loss = S[S_VALUE] / m;
    float e = 0.0f;
    for (int j = 0; j < NU; ++j) {
        const float k0 = 0.5f + HALF_LOG_2PI;
        const float k1 = k0 + log_std[j];
        e = e + k1;
    }
    const double entropy_loss = (double)(-e);
    const double t0 = (double)h.ent * entropy_loss;
    const double t1 = (double)h.vf * value_loss;
    const double l0 = policy + t0;
    stats[0] = l0 + t1;
    stats[1] = policy;
    stats[2] = value_loss;
    stats[3] = entropy_loss;
    stats[4] = S[S_KL] / m;
    stats[5] = S[S_CLIP] / m;
    stats[6] = S[S_MAXRATIO];
    stats[7] = m;
    for (int j = 0; j < NU; ++j) {
        const float g = (float)S[S_LS0 + j];
        grad_log_std[j] = g - h.ent;
    }
}

}  // namespace glppo
