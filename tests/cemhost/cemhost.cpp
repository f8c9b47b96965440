// Host (g++) instantiation of the product's csrc/gl_cem.hpp -- tests only (tests/test_plan_cem_host.py).  A child of
// plan_sample_kernel is one call of sample_child (the kernel spreads the steps' normals over four waves and runs the same recurrence
// per lane); a block of plan_elites_kernel is a loop over its 4 x 64 thread slots around the same staged tiles; the wavefront of
// plan_refit_kernel is an array of 64 lane values with the butterfly (xor 32, 16, .. 1) as loops, the same operations in the same
// order as the kernel's __shfl_xor.
// With -DCEMHOST_MAIN the file is a stand-alone program (the one the sanitizers run on): it drives every entry below over small and
// awkward shapes with exactly sized heap buffers and prints "cemhost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "glgym.h"
#include "gl_cem.hpp"

using glplan::NU;
using glplan::WAVE;

namespace {

double wave_sum(double* v)
{
    for (int m = WAVE / 2; m > 0; m >>= 1) {
        double n[WAVE];
        for (int l = 0; l < WAVE; ++l) n[l] = v[l] + v[l ^ m];
        for (int l = 0; l < WAVE; ++l) v[l] = n[l];
    }
    return v[0];
}

}  // namespace

extern "C" {

int cemhost_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(glgym_plan_sample_args);
        case 1: return (int)sizeof(glgym_plan_elites_args);
        case 2: return (int)sizeof(glgym_plan_refit_args);
    }
    return -1;
}

void cemhost_words(uint32_t c, uint32_t h, uint64_t D, uint64_t seed, uint32_t* r) { glcem::words(c, h, D, seed, r); }

// glgym_plan_sample on the host; D = draw_index + *draw_base
void cemhost_sample(int P, int K, int H, const float* mean, const float* std_, double beta, uint64_t seed, uint64_t D, int carry,
                    int prev_E, const float* prev_actions, const int32_t* prev_elite_k, const int32_t* prev_n_elite, float* actions)
{
    for (int c = 0; c < P * K; ++c)
        glcem::sample_child(c, P, K, H, mean, std_, beta, seed, D, carry, prev_E, prev_actions, prev_elite_k, prev_n_elite, actions);
}

// glgym_plan_elites on the host: a block ranks 64 candidates (lane = candidate), its four waves share each staged tile of 256 keys
void cemhost_elites(int P, int K, int E, const double* ret_all, const uint8_t* failed_all, int32_t* elite_k, int32_t* n_elite)
{
    constexpr int TILE = glcem::TILE, CHUNK = glcem::CHUNK, WAVES = TILE / CHUNK;
    const int n_chunks = (K + CHUNK - 1) / CHUNK;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int p = 0; p < P; ++p) {
        const double* ret = ret_all + (size_t)p * K;
        const uint8_t* failed = failed_all + (size_t)p * K;
        for (int blk = 0; blk < n_chunks; ++blk) {
            const int k0 = blk * CHUNK;
            double rk[CHUNK];
            int rank[WAVES][CHUNK] = {}, n_adm = 0;
            for (int lane = 0; lane < CHUNK; ++lane) rk[lane] = k0 + lane < K ? glcem::key(ret[k0 + lane], failed[k0 + lane]) : nan;
            for (int j0 = 0; j0 < K; j0 += TILE) {
                double s_key[TILE];
                for (int tid = 0; tid < TILE; ++tid) {
                    const int j = j0 + tid;
                    s_key[tid] = j < K ? glcem::key(ret[j], failed[j]) : nan;
                    n_adm += s_key[tid] == s_key[tid] ? 1 : 0;
                }
                for (int w = 0; w < WAVES; ++w) {
                    const int c0 = j0 + w * CHUNK, n = K - c0 < CHUNK ? K - c0 : CHUNK;
                    if (n <= 0) continue;
                    for (int lane = 0; lane < CHUNK; ++lane)
                        rank[w][lane] += glcem::count_chunk(s_key + w * CHUNK, c0, n, rk[lane], k0 + lane, k0);
                }
            }
            for (int lane = 0; lane < CHUNK; ++lane) {
                int r = 0;
                for (int w = 0; w < WAVES; ++w) r += rank[w][lane];
                glcem::store_rank(k0 + lane, K, E, rk[lane] == rk[lane], r, n_adm, elite_k + (size_t)p * E, n_elite + p);
            }
        }
    }
}

// glgym_plan_refit on the host.  m_acc / s_acc: the double moments [H][P][6] behind the stored values (NaN where the parent was kept)
void cemhost_refit(int P, int K, int H, int E, const float* actions, const int32_t* elite_k, const int32_t* n_elite, double alpha,
                   double min_std, const float* mean, const float* std_, float* mean_out, float* std_out, double* m_acc, double* s_acc)
{
    for (int p = 0; p < P; ++p)
        for (int h = 0; h < H; ++h) {
            int n = n_elite[p];
            n = n < 0 ? 0 : (n > E ? E : n);
            const int32_t* elite = elite_k + (size_t)p * E;
            const float* rows = actions + ((size_t)h * P + p) * K * NU;
            const size_t o = ((size_t)h * P + p) * NU;
            double part[WAVE][NU], m[NU], s[NU];
            bool ok = true;
            for (int l = 0; l < WAVE; ++l) ok = glcem::lane_sum(l, n, elite, K, rows, part[l]) && ok;
            const bool keep = n == 0 || !ok;
            for (int j = 0; j < NU; ++j) m[j] = s[j] = std::numeric_limits<double>::quiet_NaN();
            if (!keep) {
                for (int j = 0; j < NU; ++j) {
                    double v[WAVE];
                    for (int l = 0; l < WAVE; ++l) v[l] = part[l][j];
                    m[j] = wave_sum(v) / (double)n;
                }
                for (int l = 0; l < WAVE; ++l) glcem::lane_sqdev(l, n, elite, rows, m, part[l]);
                for (int j = 0; j < NU; ++j) {
                    double v[WAVE];
                    for (int l = 0; l < WAVE; ++l) v[l] = part[l][j];
                    s[j] = std::sqrt(wave_sum(v) / (double)n);
                }
            }
            for (int j = 0; j < NU; ++j) {
                const float mu = mean[o + j], sd = std_[o + j];
                mean_out[o + j] = keep ? mu : (float)glcem::blend_mean(alpha, mu, m[j]);
                std_out[o + j] = keep ? sd : (float)glcem::blend_std(alpha, sd, s[j], min_std);
                if (m_acc) m_acc[o + j] = m[j];
                if (s_acc) s_acc[o + j] = s[j];
            }
        }
}

}  // extern "C"

#ifdef CEMHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// one full iteration at (P, K, H, E) on exactly sized buffers: sample, a made-up return per child, elites, a carried second sample, refit
void drive(int P, int K, int H, int E, int carry, double beta)
{
    const size_t C = (size_t)P * K;
    std::vector<float> mean((size_t)H * P * NU), sd((size_t)H * P * NU), a0((size_t)H * C * NU, 7.f), a1((size_t)H * C * NU, 7.f);
    for (size_t i = 0; i < mean.size(); ++i) { mean[i] = 0.1f * (float)((int)(i % 7) - 3); sd[i] = i % 5 == 0 ? 10.f : 0.3f; }
    cemhost_sample(P, K, H, mean.data(), sd.data(), beta, 11u, 5u, 0, 0, nullptr, nullptr, nullptr, a0.data());
    for (float v : a0) EXPECT(v >= -1.f && v <= 1.f);
    std::vector<double> ret(C);
    std::vector<uint8_t> failed(C, 0);
    for (size_t c = 0; c < C; ++c) {
        ret[c] = std::floor(4.0 * (double)a0[c * NU]);                                   // many ties
        if (c % 5 == 3) ret[c] = std::numeric_limits<double>::quiet_NaN();
        if (c % 7 == 2) ret[c] = std::numeric_limits<double>::infinity();
        if (c % 11 == 4) failed[c] = 1;
    }
    if (P > 1) for (int k = 0; k < K; ++k) failed[(size_t)(P - 1) * K + k] = 1;          // the last parent: nothing admissible
    std::vector<int32_t> elite((size_t)P * E, 99), n_el(P, 99);
    cemhost_elites(P, K, E, ret.data(), failed.data(), elite.data(), n_el.data());
    for (int p = 0; p < P; ++p) {
        EXPECT(n_el[p] >= 0 && n_el[p] <= E);
        for (int e = 0; e < E; ++e) {
            const int k = elite[(size_t)p * E + e];
            EXPECT(e < n_el[p] ? (k >= 0 && k < K && glplan::admissible(ret[(size_t)p * K + k], failed[(size_t)p * K + k])) : k == -1);
            if (e > 0 && e < n_el[p]) {
                const int kp = elite[(size_t)p * E + e - 1];
                EXPECT(glcem::outranks(ret[(size_t)p * K + kp], kp, ret[(size_t)p * K + k], k));
            }
        }
    }
    if (P > 1) EXPECT(n_el[P - 1] == 0);
    const int cr = carry < E ? carry : E;
    cemhost_sample(P, K, H, mean.data(), sd.data(), beta, 11u, 6u, cr, E, a0.data(), elite.data(), n_el.data(), a1.data());
    for (int p = 0; p < P; ++p)
        for (int k = 1; k <= cr && k < K; ++k)
            if (k - 1 < n_el[p])
                for (int h = 0; h < H; ++h)
                    EXPECT(a1[((size_t)h * C + (size_t)p * K + k) * NU] == a0[((size_t)h * C + (size_t)p * K + elite[(size_t)p * E + k - 1]) * NU]);
    std::vector<double> m((size_t)H * P * NU), s((size_t)H * P * NU);
    cemhost_refit(P, K, H, E, a0.data(), elite.data(), n_el.data(), 0.25, 0.05, mean.data(), sd.data(), mean.data(), sd.data(), m.data(),
                  s.data());                                                             // in place
    for (size_t i = 0; i < mean.size(); ++i) EXPECT(std::isfinite(mean[i]) && sd[i] >= 0.05f);
}

}  // namespace

int main()
{
    EXPECT(cemhost_sizeof(0) > 0 && cemhost_sizeof(1) > 0 && cemhost_sizeof(2) > 0);
    drive(3, 70, 3, 7, 2, 0.5);
    drive(2, 300, 2, 300, 300, 0.0);
    drive(1, 1, 1, 1, 1, 0.9);
    drive(2, 257, 2, 64, 1, 0.3);
    drive(1, 256, 1, 256, 0, 0.0);
    std::printf(failures ? "cemhost FAILED (%d)\n" : "cemhost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
