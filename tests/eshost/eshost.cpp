// Host (g++) instantiation of the product's csrc/gl_es.hpp -- tests only (tests/test_plan_es_host.py).  A lane of plan_es_sample_kernel
// is one call of pair_rows per plane; a block of plan_es_utilities_kernel is a loop over its 4 x 64 thread slots around the same
// staged tiles as cemhost's elites; the wavefront of plan_es_update_kernel is an array of 64 lane values with the butterfly (xor 32,
// 16, .. 1) as loops, the same operations in the same order as the kernel's __shfl_xor.
// With -DESHOST_MAIN the file is a stand-alone program (the one the sanitizers run on): it drives every entry below over small and
// awkward shapes with exactly sized heap buffers and prints "eshost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "glgym.h"
#include "gl_es.hpp"

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

int eshost_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(glgym_plan_es_sample_args);
        case 1: return (int)sizeof(glgym_plan_es_utilities_args);
        case 2: return (int)sizeof(glgym_plan_es_update_args);
    }
    return -1;
}

void eshost_words(uint32_t c, uint32_t h, uint64_t D, uint64_t seed, uint32_t* r) { glcem::words(c, h, D, seed, r); }

double eshost_pow_t(double b, uint64_t t) { return gles::pow_t(b, t); }

// glgym_plan_es_sample on the host; D = draw_index + *draw_base
void eshost_sample(int P, int K, int H, const float* mean, const float* std_, uint64_t seed, uint64_t D, float* actions)
{
    const int M = K / 2;
    const size_t n_child = (size_t)P * K;
    for (int q = 0; q < P * M; ++q)
        for (int h = 0; h < H; ++h) {
            const size_t row = ((size_t)h * P + q / M) * NU;
            gles::pair_rows(q, h, D, seed, mean + row, std_ + row, actions + ((size_t)h * n_child + 2 * (size_t)q) * NU);
        }
}

// glgym_plan_es_utilities on the host: the blocks and tiles of cemhost_elites, every candidate scored
void eshost_utilities(int P, int K, const double* ret_all, const uint8_t* failed_all, double* u, int32_t* n_adm_out)
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
                const int t = k0 + lane;
                int r = 0;
                for (int w = 0; w < WAVES; ++w) r += rank[w][lane];
                if (t < K) u[(size_t)p * K + t] = gles::utility(rk[lane] == rk[lane], r, n_adm);
                if (t == 0) n_adm_out[p] = n_adm;
            }
        }
    }
}

// glgym_plan_es_update on the host.  g_acc / s_acc: the double sums / M [H][P][6] behind the stored values, or NULL
void eshost_update(int P, int K, int H, int optimizer, const float* actions, const double* u, const int32_t* n_adm, double lr,
                   double lr_std, double std_decay, double min_std, double max_std, double beta1, double beta2, double eps, uint64_t t,
                   double* m1, double* m2, const float* mean, const float* std_, float* mean_out, float* std_out, double* g_acc,
                   double* s_acc)
{
    const gles::Hyper hp{optimizer, lr, lr_std, std_decay, min_std, max_std, beta1, beta2, eps};
    const int M = K / 2;
    for (int p = 0; p < P; ++p)
        for (int h = 0; h < H; ++h) {
            const float* rows = actions + ((size_t)h * P + p) * K * NU;
            const size_t o = ((size_t)h * P + p) * NU;
            double sigma[NU], part_g[WAVE][NU], part_s[WAVE][NU], g[NU], s[NU];
            for (int j = 0; j < NU; ++j) sigma[j] = (double)std_[o + j];
            for (int l = 0; l < WAVE; ++l) gles::lane_terms(l, M, rows, u + (size_t)p * K, sigma, part_g[l], part_s[l]);
            for (int j = 0; j < NU; ++j) {
                double v[WAVE];
                for (int l = 0; l < WAVE; ++l) v[l] = part_g[l][j];
                g[j] = wave_sum(v) / (double)M;
                for (int l = 0; l < WAVE; ++l) v[l] = part_s[l][j];
                s[j] = wave_sum(v) / (double)M;
            }
            const bool keep = n_adm[p] < 2 || t == 0 || !gles::finite6(g) || !gles::finite6(s);
            gles::update_row(hp, t, keep, g, s, mean + o, std_ + o, m1 ? m1 + o : nullptr, m2 ? m2 + o : nullptr, mean_out + o, std_out + o);
            for (int j = 0; j < NU; ++j) {
                if (g_acc) g_acc[o + j] = g[j];
                if (s_acc) s_acc[o + j] = s[j];
            }
        }
}

}  // extern "C"

#ifdef ESHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// one full iteration at (P, K, H) on exactly sized buffers: sample, a made-up return per child, utilities, an in-place update
void drive(int P, int K, int H, int optimizer)
{
    const size_t C = (size_t)P * K, n = (size_t)H * P * NU;
    std::vector<float> mean(n), sd(n), a(H * C * NU, 7.f);
    for (size_t i = 0; i < n; ++i) { mean[i] = 0.1f * (float)((int)(i % 7) - 3); sd[i] = i % 5 == 0 ? 0.f : 0.3f; }
    eshost_sample(P, K, H, mean.data(), sd.data(), 11u, 5u, a.data());
    for (float v : a) EXPECT(v >= -1.f && v <= 1.f);
    std::vector<double> ret(C), u(C, 9.0);
    std::vector<uint8_t> failed(C, 0);
    for (size_t c = 0; c < C; ++c) {
        ret[c] = std::floor(4.0 * (double)a[c * NU + 1]);                                  // many ties
        if (c % 5 == 3) ret[c] = std::numeric_limits<double>::quiet_NaN();
        if (c % 7 == 2) ret[c] = std::numeric_limits<double>::infinity();
        if (c % 11 == 4) failed[c] = 1;
    }
    if (P > 1) for (int k = 0; k < K; ++k) failed[(size_t)(P - 1) * K + k] = 1;          // the last row: nothing admissible
    std::vector<int32_t> n_adm(P, 99);
    eshost_utilities(P, K, ret.data(), failed.data(), u.data(), n_adm.data());
    for (int p = 0; p < P; ++p) {
        EXPECT(n_adm[p] >= 0 && n_adm[p] <= K);
        for (int k = 0; k < K; ++k) EXPECT(u[(size_t)p * K + k] >= -0.5 && u[(size_t)p * K + k] <= 0.5);
    }
    if (P > 1) EXPECT(n_adm[P - 1] == 0);
    std::vector<double> m1(n, 0.0), m2(n, 0.0), g(n), s(n);
    const std::vector<float> mean0 = mean, sd0 = sd;
    eshost_update(P, K, H, optimizer, a.data(), u.data(), n_adm.data(), 0.1, 0.2, 0.99, 0.05, 1.0, 0.9, 0.999, 1e-8, 3, m1.data(),
                  m2.data(), mean.data(), sd.data(), mean.data(), sd.data(), g.data(), s.data());    // in place
    for (size_t i = 0; i < n; ++i) EXPECT(std::isfinite(mean[i]) && (sd[i] >= 0.05f || n_adm[(i / NU) % P] < 2));
    if (P > 1)
        for (int h = 0; h < H; ++h)
            for (int j = 0; j < NU; ++j) {
                const size_t o = ((size_t)h * P + P - 1) * NU + j;
                EXPECT(mean[o] == mean0[o] && sd[o] == sd0[o] && m1[o] == 0.0 && m2[o] == 0.0);
            }
}

}  // namespace

int main()
{
    EXPECT(eshost_sizeof(0) > 0 && eshost_sizeof(1) > 0 && eshost_sizeof(2) > 0);
    EXPECT(eshost_pow_t(0.5, 5) == 0.03125 && eshost_pow_t(0.9, 1) == 0.9 && eshost_pow_t(0.0, 7) == 0.0);
    drive(3, 70, 3, gles::ADAM);
    drive(2, 300, 2, gles::SGD);
    drive(1, 2, 1, gles::ADAM);
    drive(2, 258, 2, gles::ADAM);
    drive(1, 256, 1, gles::SGD);
    std::printf(failures ? "eshost FAILED (%d)\n" : "eshost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
