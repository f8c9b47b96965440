// Host (g++) instantiation of the product's csrc/gl_plan.hpp -- tests only (tests/test_plan_host.py).  The wavefront of
// glgym_plan.hip is an array of 64 lane values here; the butterfly exchanges (xor 32, 16, .. 1) are loops over it, the same
// operations in the same order as the kernel's __shfl_xor.
#include <cmath>
#include <cstdint>
#include <limits>

#include "glgym.h"
#include "gl_plan.hpp"

using glplan::Cand;
using glplan::NU;
using glplan::WAVE;

namespace {

Cand wave_best(Cand* c)
{
    for (int m = WAVE / 2; m > 0; m >>= 1) {
        Cand n[WAVE];
        for (int l = 0; l < WAVE; ++l) n[l] = glplan::combine(c[l], c[l ^ m]);
        for (int l = 0; l < WAVE; ++l) c[l] = n[l];
    }
    return c[0];
}

double wave_sum(double* v)
{
    for (int m = WAVE / 2; m > 0; m >>= 1) {
        double n[WAVE];
        for (int l = 0; l < WAVE; ++l) n[l] = v[l] + v[l ^ m];
        for (int l = 0; l < WAVE; ++l) v[l] = n[l];
    }
    return v[0];
}

Cand best_of(int K, const double* ret, const uint8_t* failed)
{
    Cand c[WAVE];
    for (int l = 0; l < WAVE; ++l) c[l] = glplan::lane_best(l, K, ret, failed);
    return wave_best(c);
}

}  // namespace

extern "C" {

int planhost_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(glgym_plan_fork_args);
        case 1: return (int)sizeof(glgym_plan_accumulate_args);
        case 2: return (int)sizeof(glgym_plan_rollout_args);
        case 3: return (int)sizeof(glgym_plan_select_args);
        case 4: return (int)sizeof(glgym_step_args);
    }
    return -1;
}

// n_steps env-steps of B children: reward / done / flags [n_steps][B], info [n_steps][3][B] (co2, temp, rh), weights w[n_steps]
void planhost_accumulate(int n, int B, const double* w, const double* reward, const double* info, const uint8_t* done,
                         const int32_t* flags, double* ret, double* viol /*[3][B]*/, int32_t* n_steps, uint8_t* alive, uint8_t* failed)
{
    for (int s = 0; s < n; ++s)
        for (int b = 0; b < B; ++b) {
            const size_t i = (size_t)s * B + b;
            glplan::accumulate(ret[b], viol[b], viol[B + b], viol[2 * B + b], n_steps[b], alive[b], failed[b], w[s], reward[i],
                               info[((size_t)s * 3 + 0) * B + b], info[((size_t)s * 3 + 1) * B + b], info[((size_t)s * 3 + 2) * B + b],
                               done[i], flags[i]);
        }
}

// glgym_plan_select on the host.  mean_acc: the double accumulators [H][P][6] behind mean_sequence (may be null with mean_sequence).
void planhost_select(int P, int K, int H, const double* ret, const uint8_t* failed, const float* actions, int32_t* best_k,
                     double* best_ret, float* best_action, float* best_sequence, double temperature, float* mean_sequence,
                     double* mean_acc)
{
    const size_t n_child = (size_t)P * K;
    for (int p = 0; p < P; ++p) {
        const size_t first = (size_t)p * K;
        const Cand c = best_of(K, ret + first, failed + first);
        const bool none = c.k == glplan::NONE;
        best_k[p] = none ? -1 : c.k;
        best_ret[p] = none ? std::numeric_limits<double>::quiet_NaN() : c.v;
        for (int j = 0; j < NU; ++j) best_action[(size_t)p * NU + j] = none ? 0.f : actions[(first + c.k) * NU + j];
        if (best_sequence)
            for (int h = 0; h < H; ++h)
                for (int j = 0; j < NU; ++j)
                    best_sequence[((size_t)h * P + p) * NU + j] = none ? 0.f : actions[((size_t)h * n_child + first + c.k) * NU + j];
        if (!mean_sequence) continue;
        for (int h = 0; h < H; ++h) {
            double acc[NU] = {0, 0, 0, 0, 0, 0};
            if (!none) {
                const double inv_t = 1.0 / temperature;
                double zl[WAVE];
                for (int l = 0; l < WAVE; ++l) zl[l] = glplan::lane_weight_sum(l, K, ret + first, failed + first, c.v, inv_t);
                const double z = wave_sum(zl);
                double part[WAVE][NU];
                for (int l = 0; l < WAVE; ++l)
                    glplan::lane_mean(l, K, ret + first, failed + first, c.v, inv_t, z, actions + ((size_t)h * n_child + first) * NU, part[l]);
                for (int j = 0; j < NU; ++j) {
                    double v[WAVE];
                    for (int l = 0; l < WAVE; ++l) v[l] = part[l][j];
                    acc[j] = wave_sum(v);
                }
            }
            for (int j = 0; j < NU; ++j) {
                const size_t o = ((size_t)h * P + p) * NU + j;
                mean_sequence[o] = (float)acc[j];
                if (mean_acc) mean_acc[o] = acc[j];
            }
        }
    }
}

}  // extern "C"
