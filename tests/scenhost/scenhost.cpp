// Host (g++) instantiation of the product's csrc/gl_scen.hpp -- tests only (tests/test_plan_scen_host.py).  A lane of
// plan_scenario_kernel is one call of split_child + crop_block; the wavefront of plan_aggregate_kernel is a loop over its 64 lanes
// around the same staged row: every lane ranks its scenarios lane, lane + 64, ..., lane 0 sums the ascending row, lanes 1..3 a
// violation row each, lane 4 takes the fewest steps.
// With -DSCENHOST_MAIN the file is a stand-alone program (the one the sanitizers run on): it drives the entries below over small and
// awkward shapes with exactly sized heap buffers and prints "scenhost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "glgym.h"
#include "gl_scen.hpp"

using glplan::WAVE;

extern "C" {

int scenhost_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(glgym_plan_scenario_args);
        case 1: return (int)sizeof(glgym_plan_rollout_scenarios_args);
        case 2: return (int)sizeof(glgym_plan_aggregate_args);
    }
    return -1;
}

// glgym_plan_scenario on the host at step h; D = draw_index + *draw_base.  crop: SoA [34][ld] f32 (what a float32 handle stores; a
// float64 handle stores the same values widened).  actions_in [P*K][6] -> actions_out [P*K*S][6], both or neither.
void scenhost_scenario(int P, int K, int S, int ld, int h, int hold, double scale, uint64_t seed, uint64_t D, const float* p0, float* crop,
                       const float* actions_in, float* actions_out)
{
    for (int c = 0; c < P * K * S; ++c) {
        uint32_t ps;
        int cand;
        glscen::split_child(c, K, S, &ps, &cand);
        float v[glscen::NCROP];
        glscen::crop_block(ps, h, hold, D, seed, scale, p0, v);
        for (int i = 0; i < glscen::NCROP; ++i) crop[(size_t)i * ld + c] = v[i];
        if (actions_in)
            for (int j = 0; j < glplan::NU; ++j) actions_out[(size_t)c * glplan::NU + j] = actions_in[(size_t)cand * glplan::NU + j];
    }
}

// u - 0.5 of the 34 used words of scenario ps = p*S + s at step key hh: out [34]
void scenhost_centred(uint32_t ps, uint32_t hh, uint64_t D, uint64_t seed, double* out)
{
    for (uint32_t blk = 0; blk < (uint32_t)glscen::N_BLK; ++blk) {
        uint32_t r[4];
        glscen::words(ps, hh, blk, D, seed, r);
        for (int q = 0; q < 4; ++q)
            if (4 * blk + q < (uint32_t)glscen::NCROP) out[4 * blk + q] = glscen::centred(r[q]);
    }
}

// glgym_plan_aggregate on the host: one wavefront per candidate
void scenhost_aggregate(int J, int S, int m, int ld, int ld_cand, const double* ret, const uint8_t* failed, const double* viol,
                        const int32_t* n_steps, double* ret_cand, uint8_t* failed_cand, double* viol_cand, int32_t* steps_cand)
{
    for (int j = 0; j < J; ++j) {
        double s_val[glscen::MAX_S], s_sorted[glscen::MAX_S];
        const size_t first = (size_t)j * S;
        bool is_bad = false;
        for (int lane = 0; lane < WAVE; ++lane)
            for (int s = lane; s < S; s += WAVE) {
                s_val[s] = ret[first + s];
                is_bad = is_bad || glscen::bad(s_val[s], failed[first + s]);
            }
        if (!is_bad)
            for (int lane = 0; lane < WAVE; ++lane)
                for (int s = lane; s < S; s += WAVE) s_sorted[glscen::rank_asc(s_val, S, s)] = s_val[s];
        ret_cand[j] = is_bad ? glscen::nan_value() : glscen::tail_mean(s_sorted, m);
        failed_cand[j] = is_bad ? 1 : 0;
        if (viol_cand)
            for (int i = 0; i < 3; ++i) viol_cand[(size_t)i * ld_cand + j] = glscen::seq_mean(viol + (size_t)i * ld + first, S);
        if (steps_cand) steps_cand[j] = glscen::min_steps(n_steps + first, S);
    }
}

}  // extern "C"

#ifdef SCENHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

void drive(int P, int K, int S, int H, int m)
{
    const int C = P * K * S, J = P * K;
    std::vector<float> p0(glscen::NCROP), crop((size_t)glscen::NCROP * C), a_in((size_t)J * 6), a_out((size_t)C * 6, 7.f);
    for (int i = 0; i < glscen::NCROP; ++i) p0[i] = 0.5f + (float)i;
    for (size_t i = 0; i < a_in.size(); ++i) a_in[i] = (float)i;
    for (int h = 0; h < H; ++h)
        for (int hold = 0; hold < 2; ++hold) {
            scenhost_scenario(P, K, S, C, h, hold, 0.2, 0x1234567800000009ull, (3ull << 32) | 5u, p0.data(), crop.data(), a_in.data(), a_out.data());
            for (int c = 0; c < C; ++c) {
                EXPECT(a_out[(size_t)c * 6] == a_in[(size_t)(c / S) * 6]);
                EXPECT(crop[(size_t)16 * C + c] == crop[(size_t)13 * C + c] / crop[(size_t)14 * C + c]);
                EXPECT(std::fabs(crop[c] - p0[0]) <= 0.1f * p0[0] * 1.0001f);
            }
        }
    std::vector<double> ret(C), viol((size_t)3 * C), rc(J), vc((size_t)3 * J);
    std::vector<uint8_t> failed(C, 0), fc(J);
    std::vector<int32_t> n(C), sc(J);
    for (int c = 0; c < C; ++c) {
        ret[c] = std::floor(3.0 * crop[c]) - (double)(c % 3);
        viol[c] = viol[(size_t)C + c] = viol[(size_t)2 * C + c] = 0.25 * (c % 5);
        n[c] = 1 + c % 4;
    }
    if (C > 2) { ret[1] = std::numeric_limits<double>::quiet_NaN(); failed[C - 1] = 1; }
    scenhost_aggregate(J, S, m, C, J, ret.data(), failed.data(), viol.data(), n.data(), rc.data(), fc.data(), vc.data(), sc.data());
    for (int j = 0; j < J; ++j) {
        EXPECT(fc[j] == (std::isnan(rc[j]) ? 1 : 0));
        EXPECT(sc[j] >= 1 && sc[j] <= 4 && vc[j] >= 0.0 && vc[j] <= 1.0);
    }
    scenhost_aggregate(J, S, m, C, J, ret.data(), failed.data(), nullptr, nullptr, rc.data(), fc.data(), nullptr, nullptr);
}

}  // namespace

int main()
{
    EXPECT(scenhost_sizeof(0) > 0 && scenhost_sizeof(1) > 0 && scenhost_sizeof(2) > 0);
    drive(2, 3, 5, 3, 2);
    drive(1, 1, 1, 1, 1);
    drive(3, 7, 4, 2, 4);
    drive(1, 2, 65, 1, 64);
    drive(1, 2, 256, 1, 256);
    std::printf(failures ? "scenhost FAILED (%d)\n" : "scenhost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
