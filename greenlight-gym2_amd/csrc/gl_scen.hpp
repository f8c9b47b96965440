// gl_scen.hpp -- the scalar logic of robust planning (include/glgym.h glgym_plan_scenario, glgym_plan_rollout_scenarios,
// glgym_plan_aggregate), for host and device code alike:
//   words, crop_block
//                   one child c = (p*K + k)*S + s at horizon step h: Philox words keyed by (greenhouse, scenario) -- NOT by the
//                   candidate k: scenario s of greenhouse p is the same future for all K candidates (common random numbers) -- ->
//                   the 34 crop parameters p[128..161] * (1 + U(-scale/2, scale/2)), cLeafMax = laiMax / sla recomputed
//   bad, rank_asc, tail_mean, seq_mean, min_steps
//                   the risk score of one candidate over its S scenario returns: what ONE lane contributes to the ascending rank by
//                   counting over the staged returns, and the sequential sums one lane performs once the ranks are known
// Everything is double with products and sums rounded separately, as in gl_plan.hpp and gl_cem.hpp.
#pragma once
#include <limits>

#include "gl_cem.hpp"

namespace glscen {

constexpr int NCROP = 34;                        // p[128..161]
constexpr int N_BLK = 9;                         // Philox blocks per crop block: 36 words, 34 used
constexpr int LAI_MAX = 13, SLA = 14, C_LEAF_MAX = 16;   // rows of the crop block: p[141], p[142], p[144]
constexpr uint32_t KEY_TAG = 0x5343454eu;        // "SCEN": xor-ed into the key's high word, apart from the CEM and crop-noise streams
constexpr int MAX_S = glcem::TILE;               // scenarios per candidate staged in LDS by glgym_plan_aggregate

// the horizon step that keys the draw: hold = 1 is one parametric draw held over the horizon, hold = 0 a fresh draw at every step
GLPLAN_HD uint32_t step_key(int h, int hold) { return hold ? 0u : (uint32_t)h; }

// r[4*blk .. 4*blk+3] of scenario s of greenhouse p (ps = p*S + s) at step hh of draw D: counter (ps, lo32(D), hi32(D), 16*hh + blk),
// key (lo32(seed), hi32(seed) ^ KEY_TAG)
GLPLAN_HD void words(uint32_t ps, uint32_t hh, uint32_t blk, uint64_t D, uint64_t seed, uint32_t r[4])
{
    glcem::philox4x32_10(ps, (uint32_t)D, (uint32_t)(D >> 32), 16u * hh + blk, (uint32_t)seed, (uint32_t)(seed >> 32) ^ KEY_TAG, r);
}

// u - 0.5 with u = (r + 0.5) * 2^-32 in (0, 1): uniform on (-1/2, 1/2)
GLPLAN_HD double centred(uint32_t r)
{
#pragma clang fp contract(off)
    const double u = ((double)r + 0.5) * glcem::TWO_M32;
    return u - 0.5;
}

// one parameter: v = (float)(p_i + ((u - 0.5) * scale) * p_i)
GLPLAN_HD float perturb(uint32_t r, double scale, float p_i)
{
#pragma clang fp contract(off)
    const double z = centred(r) * scale;
    const double t = z * (double)p_i;
    return (float)((double)p_i + t);
}

// The 34 values of one child at one step.  p0 = the handle's float32 p[128..161].
GLPLAN_HD void crop_block(uint32_t ps, int h, int hold, uint64_t D, uint64_t seed, double scale, const float* p0, float v[NCROP])
{
    const uint32_t hh = step_key(h, hold);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int blk = 0; blk < N_BLK; ++blk) {
        uint32_t r[4];
        words(ps, hh, (uint32_t)blk, D, seed, r);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int q = 0; q < 4; ++q) {
            const int i = 4 * blk + q;
            if (i < NCROP) v[i] = perturb(r[q], scale, p0[i]);
        }
    }
    v[C_LEAF_MAX] = v[LAI_MAX] / v[SLA];           // cLeafMax = laiMax / sla, in float32
}

// child c = (p*K + k)*S + s -> its greenhouse-scenario index p*S + s and its candidate p*K + k
GLPLAN_HD void split_child(int c, int K, int S, uint32_t* ps, int* cand)
{
    const int j = c / S, s = c - j * S, p = j / K;
    *cand = j;
    *ps = (uint32_t)p * (uint32_t)S + (uint32_t)s;
}

// ---- aggregate: the risk score of one candidate -------------------------------------------------------------------------------
// a scenario that makes its candidate inadmissible
GLPLAN_HD bool bad(double ret, uint8_t failed) { return !glplan::admissible(ret, failed); }

// ascending rank of scenario s among the candidate's S staged returns, ties to the lower index: the slot of r_s in the sorted row.
// Only meaningful when no return is NaN (a candidate with one is NaN whatever the order).
GLPLAN_HD int rank_asc(const double* r, int S, int s)
{
    const double rs = r[s];
    int rank = 0;
    for (int j = 0; j < S; ++j) rank += (r[j] < rs || (r[j] == rs && j < s)) ? 1 : 0;
    return rank;
}

// (((0.0 + a_0) + a_1) + ... + a_{m-1}) / m over the ascending row: m = S the mean, m = 1 the worst case, between a tail mean
GLPLAN_HD double tail_mean(const double* sorted, int m)
{
    double acc = 0.0;
    for (int i = 0; i < m; ++i) acc = acc + sorted[i];
    return acc / (double)m;
}

// (sum in index order, from 0.0) / S
GLPLAN_HD double seq_mean(const double* v, int S)
{
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc = acc + v[s];
    return acc / (double)S;
}

GLPLAN_HD int32_t min_steps(const int32_t* n, int S)
{
    int32_t m = n[0];
    for (int s = 1; s < S; ++s) m = n[s] < m ? n[s] : m;
    return m;
}

GLPLAN_HD double nan_value() { return std::numeric_limits<double>::quiet_NaN(); }

}  // namespace glscen
