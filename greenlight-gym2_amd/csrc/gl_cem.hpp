// gl_cem.hpp -- the scalar logic of the cross-entropy method's stages between two rollouts (include/glgym.h glgym_plan_sample,
// glgym_plan_elites, glgym_plan_refit), for host and device code alike:
//   normals_of, colour, reserved, write_row, sample_child
//                   one child c = p*K + k: Philox words -> Box-Muller normals e_h -> coloured noise n_h -> clip(mean + std * n), or
//                   the reserved candidates (k = 0: the clipped mean; 1 <= k <= carry: a copy of the previous population's elite
//                   k-1); sample_child is the whole sequence in step order, which the kernel reproduces chain by chain
//   key, count_chunk, store_rank
//                   rank by counting: what ONE thread adds to its candidate's rank from one chunk of the parent's staged returns
//   lane_sum, lane_sqdev, blend_mean, blend_std
//                   what ONE lane of the refitting wavefront sums over its elites e = lane, lane + 64, ...; the wavefront combines
//                   the 64 partial sums with gl_plan.hpp's butterfly (tests/cemhost/cemhost.cpp: a loop over an array of 64)
// Everything is double with products and sums rounded separately, as in gl_plan.hpp.
#pragma once
#include <limits>

#include "gl_plan.hpp"

namespace glcem {

using glplan::NU;
using glplan::WAVE;

constexpr int TILE = 256;                        // candidates staged per round of glgym_plan_elites = its block size
constexpr uint32_t KEY_TAG = 0x43454d31u;        // "CEM1": xor-ed into the key's high word, apart from the crop-noise stream
constexpr double TWO_PI = 6.283185307179586;     // 2 * pi rounded to double
constexpr double TWO_M32 = 1.0 / 4294967296.0;   // 2^-32

GLPLAN_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// r0..r7 of child c at step h of draw D: counter (c, 2h + blk, lo32(D), hi32(D)), key (lo32(seed), hi32(seed) ^ KEY_TAG)
GLPLAN_HD void words(uint32_t c, uint32_t h, uint64_t D, uint64_t seed, uint32_t r[8])
{
    for (uint32_t blk = 0; blk < 2; ++blk)
        philox4x32_10(c, 2u * h + blk, (uint32_t)D, (uint32_t)(D >> 32), (uint32_t)seed, (uint32_t)(seed >> 32) ^ KEY_TAG, r + 4 * blk);
}

// three Box-Muller pairs from r0..r5 (r6, r7 unused); u = (r + 0.5) * 2^-32 is never 0 and never 1
GLPLAN_HD void normals(const uint32_t r[8], double e[NU])
{
#pragma clang fp contract(off)
    for (int m = 0; m < 3; ++m) {
        const double u0 = ((double)r[2 * m] + 0.5) * TWO_M32, u1 = ((double)r[2 * m + 1] + 0.5) * TWO_M32;
        const double rad = std::sqrt(-2.0 * std::log(u0)), ang = TWO_PI * u1;
        e[2 * m] = rad * std::cos(ang);
        e[2 * m + 1] = rad * std::sin(ang);
    }
}

GLPLAN_HD double clip1(double v) { return v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v); }

// n_h = beta * n_{h-1} + sqrt(1 - beta^2) * e_h (n_0 = e_0); sb = sqrt(1 - beta^2)
GLPLAN_HD void colour(int h, double beta, double sb, const double e[NU], double n[NU])
{
#pragma clang fp contract(off)
    for (int j = 0; j < NU; ++j) {
        if (h == 0) { n[j] = e[j]; continue; }
        const double t0 = beta * n[j], t1 = sb * e[j];
        n[j] = t0 + t1;
    }
}

// sqrt(1 - beta^2), the product and the difference rounded separately
GLPLAN_HD double sb_of(double beta)
{
#pragma clang fp contract(off)
    const double b2 = beta * beta;
    return std::sqrt(1.0 - b2);
}

GLPLAN_HD float action(float mean, float std_, double n)
{
#pragma clang fp contract(off)
    const double t = (double)std_ * n;
    return (float)clip1((double)mean + t);
}

// Reserved candidates.  -> 0: sampled; 1: candidate 0, the clipped mean; 2: a copy of the previous population's child *src (carry;
// prev_elite_k [P][prev_E], prev_n_elite [P]; an elite index outside 0..K-1 is not followed: the candidate is sampled)
GLPLAN_HD int reserved(int p, int k, int K, int carry, int prev_E, const int32_t* prev_elite_k, const int32_t* prev_n_elite, int* src)
{
    if (k == 0) return 1;
    if (k <= carry && k - 1 < prev_E && k - 1 < prev_n_elite[p]) {
        const int e = prev_elite_k[(size_t)p * prev_E + (k - 1)];
        if (e >= 0 && e < K) { *src = e; return 2; }
    }
    return 0;
}

// The six values actions[h][c][0..5] of child c = p*K + k, given its kind (reserved()) and, if sampled, its noise n_h.
GLPLAN_HD void write_row(int kind, int src, int h, int p, int c, int P, int K, const float* mean, const float* std_, const double n[NU],
                         const float* prev_actions, float* actions)
{
    const size_t n_child = (size_t)P * K, row = ((size_t)h * P + p) * NU;
    float* out = actions + ((size_t)h * n_child + c) * NU;
    for (int j = 0; j < NU; ++j)
        out[j] = kind == 1 ? (float)clip1((double)mean[row + j])
                 : kind == 2 ? prev_actions[((size_t)h * n_child + (size_t)p * K + src) * NU + j]
                             : action(mean[row + j], std_[row + j], n[j]);
}

// e_h of child c: the six normals of step h
GLPLAN_HD void normals_of(int c, int h, uint64_t D, uint64_t seed, double e[NU])
{
    uint32_t r[8];
    words((uint32_t)c, (uint32_t)h, D, seed, r);
    normals(r, e);
}

// The whole action sequence of child c, step after step: what the kernel computes with the steps spread over the waves of a block
// (each wave draws e_h for its steps, every lane then runs this recurrence over the staged e in the same order).
GLPLAN_HD void sample_child(int c, int P, int K, int H, const float* mean, const float* std_, double beta, uint64_t seed, uint64_t D,
                            int carry, int prev_E, const float* prev_actions, const int32_t* prev_elite_k, const int32_t* prev_n_elite,
                            float* actions)
{
#pragma clang fp contract(off)
    const int p = c / K, k = c - p * K;
    int src = 0;
    const int kind = reserved(p, k, K, carry, prev_E, prev_elite_k, prev_n_elite, &src);
    const double sb = sb_of(beta);
    double n[NU] = {0, 0, 0, 0, 0, 0};
    for (int h = 0; h < H; ++h) {
        double e[NU];
        if (kind == 0) {
            normals_of(c, h, D, seed, e);
            colour(h, beta, sb, e, n);
        }
        write_row(kind, src, h, p, c, P, K, mean, std_, n, prev_actions, actions);
    }
}

// ---- elites: rank by counting ----------------------------------------------------------------------------------------------
constexpr int CHUNK = WAVE;                      // candidates ranked per block, and the share of a staged tile one wave counts

// what is staged for candidate j: its return, or NaN if it is not admissible -- a NaN compares false and is never counted
GLPLAN_HD double key(double ret, uint8_t failed) { return glplan::admissible(ret, failed) ? ret : std::numeric_limits<double>::quiet_NaN(); }

// candidate j comes before candidate k: higher return, ties to the lower index (np.argsort(-ret, kind="stable"))
GLPLAN_HD bool outranks(double rj, int j, double rk, int k) { return rj > rk || (rj == rk && j < k); }

// One thread (candidate k with key rk) over one chunk of staged keys, candidates j0 .. j0+n-1: how many of them come before k.
// k0 = the first candidate of k's own chunk (chunks are aligned): a chunk before it wins ties, a chunk after it loses them.
GLPLAN_HD int count_chunk(const double* keys, int j0, int n, double rk, int k, int k0)
{
    int rank = 0;
    if (j0 < k0) {
        for (int i = 0; i < n; ++i) rank += keys[i] >= rk ? 1 : 0;
    } else if (j0 > k0) {
        for (int i = 0; i < n; ++i) rank += keys[i] > rk ? 1 : 0;
    } else {
        for (int i = 0; i < n; ++i) rank += outranks(keys[i], j0 + i, rk, k) ? 1 : 0;
    }
    return rank;
}

// What thread t of a parent (candidate t if t < K) stores once its counts are complete: plain stores, every slot written by one thread.
GLPLAN_HD void store_rank(int t, int K, int E, bool adm, int rank, int n_adm, int32_t* elite_row, int32_t* n_elite)
{
    if (t < K && adm && rank < E) elite_row[rank] = t;
    if (t < E && t >= n_adm) elite_row[t] = -1;        // E <= K: some thread t exists for every slot of the row
    if (t == 0) *n_elite = n_adm < E ? n_adm : E;
}

// ---- refit -----------------------------------------------------------------------------------------------------------------
// this lane's share of sum_e a[elite_e][0..5]; rows = the parent's K rows of one horizon step, [K][6] f32.  Returns false if an elite
// index lies outside 0..K-1 (the wavefront then leaves the parent's mean and std alone).
GLPLAN_HD bool lane_sum(int lane, int n, const int32_t* elite_k, int K, const float* rows, double acc[NU])
{
    bool ok = true;
    for (int j = 0; j < NU; ++j) acc[j] = 0.0;
    for (int e = lane; e < n; e += WAVE) {
        const int k = elite_k[e];
        if (k < 0 || k >= K) { ok = false; continue; }
        const float* row = rows + (size_t)k * NU;
        for (int j = 0; j < NU; ++j) acc[j] = acc[j] + (double)row[j];
    }
    return ok;
}

// this lane's share of sum_e (a - m)^2; call only after lane_sum returned true on every lane
GLPLAN_HD void lane_sqdev(int lane, int n, const int32_t* elite_k, const float* rows, const double m[NU], double acc[NU])
{
#pragma clang fp contract(off)
    for (int j = 0; j < NU; ++j) acc[j] = 0.0;
    for (int e = lane; e < n; e += WAVE) {
        const float* row = rows + (size_t)elite_k[e] * NU;
        for (int j = 0; j < NU; ++j) {
            const double d = (double)row[j] - m[j];
            const double d2 = d * d;
            acc[j] = acc[j] + d2;
        }
    }
}

GLPLAN_HD double blend_mean(double alpha, float mean, double m)
{
#pragma clang fp contract(off)
    const double t0 = alpha * (double)mean, t1 = (1.0 - alpha) * m;
    return t0 + t1;
}

GLPLAN_HD double blend_std(double alpha, float std_, double s, double min_std)
{
#pragma clang fp contract(off)
    const double t0 = alpha * (double)std_, t1 = (1.0 - alpha) * s;
    const double v = t0 + t1;
    return v > min_std ? v : min_std;              // NaN falls to min_std
}

}  // namespace glcem
