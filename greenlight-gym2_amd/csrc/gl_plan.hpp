// gl_plan.hpp -- the scalar logic of device-side planning (include/glgym.h glgym_plan_*), for host and device code alike:
//   accumulate      one env-step's reward / violations / flags into a child's accumulators, with the season-end latch
//   Cand, combine   the (value, index) pair of the argmax over candidates and its associative, commutative combination
//   lane_best, lane_weight_sum, lane_mean
//                   what ONE lane of the selecting wavefront computes over its candidates k = lane, lane + 64, ...; the wavefront
//                   then combines the 64 partial results with butterfly exchanges (xor 32, 16, .. 1) -- __shfl_xor on the device,
//                   a loop over an array of 64 on the host (tests/planhost/planhost.cpp), the same operations in the same order.
// Products and sums are rounded separately (no fused multiply-add) so that a NumPy restatement of the returns is bit-exact.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GLPLAN_HD __host__ __device__ __forceinline__
#else
#define GLPLAN_HD inline
#endif

namespace glplan {

constexpr int WAVE = 64;
constexpr int NU = 6;
constexpr int INFO_CO2 = 8, INFO_TEMP = 7, INFO_RH = 9;      // rows of the info block (GLGYM_NINFO order) behind viol[0..2]
constexpr int SF_FAILED = 128;                               // GLGYM_SF_FAILED
constexpr int NONE = 0x7fffffff;                             // index of "no admissible candidate"

// One env-step of one child.  `alive` is the value BEFORE the step: the step that reports done is counted, nothing after it.
GLPLAN_HD void accumulate(double& ret, double& v_co2, double& v_temp, double& v_rh, int32_t& n_steps, uint8_t& alive, uint8_t& failed,
                          double w, double reward, double i_co2, double i_temp, double i_rh, uint8_t done, int32_t flags)
{
#pragma clang fp contract(off)
    if (!alive) return;
    const double wr = w * reward;
    ret = ret + wr;
    v_co2 = v_co2 + i_co2;
    v_temp = v_temp + i_temp;
    v_rh = v_rh + i_rh;
    n_steps += 1;
    if (flags & SF_FAILED) failed = 1;
    if (done) alive = 0;
}

struct Cand {
    double v;
    int k;              // NONE: no admissible candidate behind this value
};

GLPLAN_HD bool admissible(double ret, uint8_t failed) { return !failed && std::isfinite(ret); }

// the better of two: higher value, ties to the lower index.  Symmetric, so every lane of a butterfly ends with the same pair.
GLPLAN_HD Cand combine(Cand a, Cand b)
{
    if (b.k == NONE) return a;
    if (a.k == NONE) return b;
    if (b.v > a.v || (b.v == a.v && b.k < a.k)) return b;
    return a;
}

GLPLAN_HD Cand lane_best(int lane, int K, const double* ret, const uint8_t* failed)
{
    Cand c{0.0, NONE};
    for (int k = lane; k < K; k += WAVE)
        if (admissible(ret[k], failed[k])) c = combine(c, Cand{ret[k], k});
    return c;
}

// unnormalised MPPI weight of candidate k given the parent's maximum
GLPLAN_HD double weight(double ret, uint8_t failed, double vmax, double inv_temperature)
{
#pragma clang fp contract(off)
    return admissible(ret, failed) ? std::exp((ret - vmax) * inv_temperature) : 0.0;
}

GLPLAN_HD double lane_weight_sum(int lane, int K, const double* ret, const uint8_t* failed, double vmax, double inv_temperature)
{
    double z = 0.0;
    for (int k = lane; k < K; k += WAVE) z = z + weight(ret[k], failed[k], vmax, inv_temperature);
    return z;
}

// this lane's share of sum_k (w_k / Z) * a[k][0..5]; a = the parent's K rows of one horizon step, [K][6] f32
GLPLAN_HD void lane_mean(int lane, int K, const double* ret, const uint8_t* failed, double vmax, double inv_temperature, double z,
                         const float* a, double acc[NU])
{
#pragma clang fp contract(off)
    for (int j = 0; j < NU; ++j) acc[j] = 0.0;
    for (int k = lane; k < K; k += WAVE) {
        const double wn = weight(ret[k], failed[k], vmax, inv_temperature) / z;
        if (wn == 0.0) continue;            // the action rows of inadmissible candidates are not read
        const float* row = a + (size_t)k * NU;
        for (int j = 0; j < NU; ++j) {
            const double t = wn * (double)row[j];
            acc[j] = acc[j] + t;
        }
    }
}

}  // namespace glplan
