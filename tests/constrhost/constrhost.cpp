// Host (g++) instantiation of the product's csrc/gl_constr.hpp -- tests only (tests/test_plan_constr_host.py).  The wavefront of
// plan_constrain_candidates_kernel is a loop over its 64 lanes (lane_runs each), followed by the lane-order sum; up to SMALL_R runs a
// lane of plan_constrain_few_runs_kernel is one call of thread_runs; the workgroup of
// plan_constrain_groups_kernel is a loop over the group's candidates (a minimum and a count have no order).
// With -DCONSTRHOST_MAIN the file is a stand-alone program (the one a sanitizer can run on): it drives the entry below over small and
// awkward shapes with exactly sized heap buffers and prints "constrhost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "glgym.h"
#include "gl_constr.hpp"

extern "C" {

int constrhost_sizeof(void) { return (int)sizeof(glgym_plan_constrain_args); }

// glgym_plan_constrain on the host.  The optional outputs may be null; failed_out may be failed_cand.
void constrhost_constrain(int P, int O, int K, int S, int ld, int per_step, int n_allow, int mode, const double* budget, const double* weight,
                          double rho, const double* ret_cand, const uint8_t* failed_cand, const double* viol, const int32_t* n_steps,
                          double* score, uint8_t* failed_out, uint8_t* feasible, double* excess, int32_t* n_viol, int32_t* n_feasible)
{
    const glconstr::Spec sp{O, K, S, per_step, {budget[0], budget[1], budget[2]}, {weight[0], weight[1], weight[2]}};
    for (int j = 0; j < P * K; ++j) {
        const int p = j / K, k = j - p * K;
        double total = 0.0;
        int nv = 0;
        bool nonfinite = false;
        if (O * S <= glconstr::SMALL_R) {                                  // plan_constrain_few_runs_kernel: a lane is a candidate
            const glconstr::Part one = glconstr::thread_runs(sp, p, k, viol, (size_t)ld, n_steps);
            total = one.sum, nv = one.n_viol, nonfinite = one.nonfinite;
        } else {
            glconstr::Part part[glconstr::WAVE];
            for (int lane = 0; lane < glconstr::WAVE; ++lane) part[lane] = glconstr::lane_runs(lane, sp, p, k, viol, (size_t)ld, n_steps);
            for (int lane = 0; lane < glconstr::WAVE; ++lane) {
                total = glconstr::combine(total, part[lane].sum);
                nv += part[lane].n_viol;
                nonfinite = nonfinite || part[lane].nonfinite;
            }
        }
        const double G = glconstr::mean_excess(total, O * S);
        const uint8_t flags = glconstr::flags_of(ret_cand[j], failed_cand[j], nonfinite, nv, n_allow);
        score[j] = G;
        failed_out[j] = flags;
        if (excess) excess[j] = G;
        if (n_viol) n_viol[j] = nv;
        if (feasible) feasible[j] = (flags & glconstr::FLAG_INFEASIBLE) ? 0 : 1;
    }
    for (int p = 0; p < P; ++p) {
        const size_t first = (size_t)p * K;
        double mn = std::numeric_limits<double>::infinity();
        int cnt = 0;
        for (int k = 0; k < K; ++k)
            if (glconstr::counts_for_floor(failed_out[first + k])) {
                mn = ret_cand[first + k] < mn ? ret_cand[first + k] : mn;
                ++cnt;
            }
        const double floor_p = glconstr::floor_of(mn, cnt);
        for (int k = 0; k < K; ++k) {
            const uint8_t flags = failed_out[first + k];
            score[first + k] = glconstr::score_of(mode, ret_cand[first + k], score[first + k], flags, floor_p, rho);
            failed_out[first + k] = flags & glconstr::FLAG_FAILED;
        }
        if (n_feasible) n_feasible[p] = cnt;
    }
}

}  // extern "C"

#ifdef CONSTRHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

void drive(int P, int O, int K, int S, int per_step, int n_allow, int mode)
{
    const int C = P * O * K * S, J = P * K;
    std::vector<double> viol((size_t)3 * C), ret(J), score(J), excess(J);
    std::vector<int32_t> n(C), nv(J), nf(P);
    std::vector<uint8_t> failed(J, 0), fo(J), feas(J);
    for (int c = 0; c < C; ++c) {
        viol[c] = 0.5 * (c % 7);
        viol[(size_t)C + c] = 0.25 * (c % 3);
        viol[(size_t)2 * C + c] = (double)(c % 5);
        n[c] = c % 4;
    }
    for (int j = 0; j < J; ++j) ret[j] = 10.0 - (double)(j % 6);
    if (J > 1) failed[J - 1] = 1;
    if (C > 3) viol[3] = std::numeric_limits<double>::infinity();
    const double inf = std::numeric_limits<double>::infinity();
    const double budget[3] = {1.0, inf, 2.0}, weight[3] = {1.0, 2.0, 0.5};
    constrhost_constrain(P, O, K, S, C, per_step, n_allow, mode, budget, weight, 0.5, ret.data(), failed.data(), viol.data(), n.data(),
                         score.data(), fo.data(), feas.data(), excess.data(), nv.data(), nf.data());
    for (int j = 0; j < J; ++j) {
        EXPECT(fo[j] <= 1 && feas[j] <= 1 && nv[j] >= 0 && nv[j] <= O * S && excess[j] >= 0.0);
        EXPECT((fo[j] != 0) == std::isnan(score[j]));
        EXPECT(feas[j] == (nv[j] <= n_allow ? 1 : 0));
    }
    for (int p = 0; p < P; ++p) EXPECT(nf[p] >= 0 && nf[p] <= K);
    constrhost_constrain(P, O, K, S, C, per_step, n_allow, mode, budget, weight, 0.5, ret.data(), failed.data(), viol.data(), n.data(),
                         score.data(), failed.data(), nullptr, nullptr, nullptr, nullptr);
}

}  // namespace

int main()
{
    EXPECT(constrhost_sizeof() > 0);
    for (int mode = 0; mode < 2; ++mode) {
        drive(1, 1, 1, 1, 1, 0, mode);
        drive(3, 1, 5, 3, 1, 1, mode);
        drive(1, 3, 5, 2, 0, 0, mode);
        drive(2, 1, 257, 1, 1, 0, mode);
        drive(1, 65, 2, 1, 1, 65, mode);
        drive(1, 1, 3, 257, 0, 2, mode);
    }
    std::printf(failures ? "constrhost FAILED (%d)\n" : "constrhost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
