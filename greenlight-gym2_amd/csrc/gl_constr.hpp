// gl_constr.hpp -- the scalar logic of constrained candidate ranking (include/glgym.h glgym_plan_constrain), for host and device code
// alike:
//   child           the child index c = ((p*O + o)*K + k)*S + s of run r = o*S + s of candidate (p, k)
//   run_excess      g_r of one run from its three accumulated violations, and whether an active one is not finite
//   lane_runs       what ONE lane of the candidate's wavefront contributes: the runs r = lane, lane + 64, ... in ascending r, summed
//                   from 0.0, with the number of violating runs and the non-finite flag
//   combine         the 64 lane sums added in lane order from 0.0 -- THE summation order of G, fixed so that host and device agree
//                   bit for bit whatever R is
//   finish          G = sum / R, feasible = n_viol <= n_allow, failed_out
//   floor_of, score_of
//                   the group's floor (smallest admissible feasible return, or 0.0 without one, minus 1.0) and a candidate's score
// Everything is double with products, quotients and sums rounded separately, as in gl_plan.hpp and gl_scen.hpp.
//
// Why floor - 1.  In feasibility-first mode a feasible candidate scores its return r >= m, m the smallest admissible feasible return
// of its group; an infeasible admissible one scores (m - 1.0) - G with G >= 0, hence at most m - 1.0 (subtraction is monotone under
// rounding).  m - 1.0 < m for every finite m below 2^53 in magnitude, and the gap between the two classes is 1 up to one rounding of
// m - 1.0: ranks, argmax and centred ranks see the lexicographic order, and a mean weighted by exp(score / temperature) sees the
// infeasible class at least (about) 1 / temperature e-folds below the worst feasible candidate.
#pragma once
#include <limits>

#include "gl_plan.hpp"

namespace glconstr {

constexpr int WAVE = glplan::WAVE;
constexpr int GROUP_THREADS = 256;               // threads of the workgroup that scores one ranking group
constexpr int MODE_PENALTY = 0, MODE_FEASIBLE_FIRST = 1;     // GLGYM_CONSTRAIN_PENALTY, GLGYM_CONSTRAIN_FEASIBLE_FIRST
constexpr uint8_t FLAG_FAILED = 1, FLAG_INFEASIBLE = 2;      // bits of failed_out between the two kernels; only bit 0 is left afterwards

struct Spec {
    int O, K, S;                                 // runs per candidate R = O*S; the stride of o is K*S children
    int per_step;
    double budget[3], weight[3];
};

GLPLAN_HD size_t child(int p, int o, int k, int s, int O, int K, int S)
{
    return (((size_t)p * (size_t)O + (size_t)o) * (size_t)K + (size_t)k) * (size_t)S + (size_t)s;
}

GLPLAN_HD bool active(double budget) { return budget != std::numeric_limits<double>::infinity(); }

// e_i = max(0.0, v / d - budget); +0.0 when the budget is +inf (whatever v is) and when v is not finite under an active budget
// (*nonfinite is set then: the candidate fails)
GLPLAN_HD double excess_term(double v, double d, double budget, bool* nonfinite)
{
#pragma clang fp contract(off)
    if (!active(budget)) return 0.0;
    if (!std::isfinite(v)) { *nonfinite = true; return 0.0; }
    const double q = v / d;
    const double e = q - budget;
    return e > 0.0 ? e : 0.0;
}

// g_r = ((0.0 + w_0 e_0) + w_1 e_1) + w_2 e_2 of child c
GLPLAN_HD double run_excess(const Spec& sp, const double* viol, size_t ld, const int32_t* n_steps, size_t c, bool* nonfinite)
{
#pragma clang fp contract(off)
    double d = 1.0;
    if (sp.per_step) {
        const int32_t n = n_steps[c];
        d = (double)(n > 1 ? n : 1);
    }
    double g = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double t = sp.weight[i] * excess_term(viol[(size_t)i * ld + c], d, sp.budget[i], nonfinite);
        g = g + t;
    }
    return g;
}

struct Part {
    double sum;
    int n_viol;
    bool nonfinite;
};

// lane `lane` of candidate (p, k): its runs r = lane, lane + 64, ... < R in ascending r
GLPLAN_HD Part lane_runs(int lane, const Spec& sp, int p, int k, const double* viol, size_t ld, const int32_t* n_steps)
{
#pragma clang fp contract(off)
    Part a{0.0, 0, false};
    const int R = sp.O * sp.S;
    for (int r = lane; r < R; r += WAVE) {
        const int o = r / sp.S, s = r - o * sp.S;
        const double g = run_excess(sp, viol, ld, n_steps, child(p, o, k, s, sp.O, sp.K, sp.S), &a.nonfinite);
        a.sum = a.sum + g;
        a.n_viol += g > 0.0 ? 1 : 0;
    }
    return a;
}

// With R <= 64 every lane holds at most one run, its sum is 0.0 + g_r = g_r (g_r is never -0.0: it starts from 0.0 + ...), and the
// lane-order sum is ((0.0 + g_0) + g_1) + ... + g_{R-1}; the +0.0 of the empty lanes leaves a non-negative sum as it is.  So ONE thread
// that adds the runs in ascending r gets the defined G bit for bit; the kernels use it up to SMALL_R runs (lane = candidate).
constexpr int SMALL_R = 8;

GLPLAN_HD Part thread_runs(const Spec& sp, int p, int k, const double* viol, size_t ld, const int32_t* n_steps)
{
#pragma clang fp contract(off)
    Part a{0.0, 0, false};
    const int R = sp.O * sp.S;                   // <= SMALL_R
    for (int r = 0; r < R; ++r) {
        const int o = r / sp.S, s = r - o * sp.S;
        const double g = run_excess(sp, viol, ld, n_steps, child(p, o, k, s, sp.O, sp.K, sp.S), &a.nonfinite);
        a.sum = a.sum + g;
        a.n_viol += g > 0.0 ? 1 : 0;
    }
    return a;
}

// one step of the lane-order sum: acc starts at 0.0 and takes the lanes' sums 0, 1, ..., 63
GLPLAN_HD double combine(double acc, double lane_sum)
{
#pragma clang fp contract(off)
    return acc + lane_sum;
}

GLPLAN_HD double mean_excess(double total, int R)
{
#pragma clang fp contract(off)
    return total / (double)R;
}

// failed_out | (infeasible << 1): what the first kernel leaves for the second
GLPLAN_HD uint8_t flags_of(double ret, uint8_t failed, bool nonfinite, int n_viol, int n_allow)
{
    const bool f = failed != 0 || nonfinite || !std::isfinite(ret);
    return (uint8_t)((f ? FLAG_FAILED : 0) | (n_viol <= n_allow ? 0 : FLAG_INFEASIBLE));
}

// does candidate with these flags take part in the group's floor?
GLPLAN_HD bool counts_for_floor(uint8_t flags) { return flags == 0; }

GLPLAN_HD double floor_of(double min_ret, int n_feasible)
{
#pragma clang fp contract(off)
    return (n_feasible > 0 ? min_ret : 0.0) - 1.0;
}

GLPLAN_HD double score_of(int mode, double ret, double G, uint8_t flags, double floor_p, double rho)
{
#pragma clang fp contract(off)
    if (flags & FLAG_FAILED) return std::numeric_limits<double>::quiet_NaN();
    if (mode == MODE_PENALTY) {
        const double t = rho * G;
        return ret - t;
    }
    return (flags & FLAG_INFEASIBLE) ? floor_p - G : ret;
}

}  // namespace glconstr
