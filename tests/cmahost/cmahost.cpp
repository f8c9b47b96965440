// Host (g++) instantiation of the product's csrc/gl_cma.hpp -- tests only (tests/test_plan_cma_host.py).  A lane of
// plan_cma_sample_kernel is one call of sample_child; the block of plan_cma_update_kernel is a loop over the rows with the same tiles
// of 32 elites, the same owner per sum (component d for yw, entry (a, b <= a) for R), the lanes of its wavefront 0 as loops over the
// components, and the same order of the status checks; the new state is committed at the end or not at all.
// With -DCMAHOST_MAIN the file is a stand-alone program (the one the sanitizers run on): it drives both entries over small and
// awkward shapes with exactly sized heap buffers and prints "cmahost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "glgym.h"
#include "gl_cma.hpp"

using glplan::NU;

extern "C" {

int cmahost_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(glgym_plan_cma_sample_args);
        case 1: return (int)sizeof(glgym_plan_cma_update_args);
        case 2: return GLGYM_CMA_NMAX;
    }
    return -1;
}

// glgym_plan_cma_sample on the host; D = draw_index + *draw_base
void cmahost_sample(int P, int K, int N, const float* mean, const double* sigma, const double* chol, uint64_t seed, uint64_t D, float* theta)
{
    for (int p = 0; p < P; ++p)
        for (int k = 0; k < K; ++k)
            glcma::sample_child(p * K + k, p, P, K, N, D, seed, chol + (size_t)p * N * N, mean, sigma[p], theta);
}

// glgym_plan_cma_update on the host; hyper = mu_eff, c_sigma, d_sigma, c_c, c_1, c_mu, chi_n, min_sigma, max_sigma.
// yw_out / zw_out [P][N]: the intermediate vectors of the rows that got that far, or NULL
void cmahost_update(int P, int K, int N, int E, const float* theta, const int32_t* elite_k, const int32_t* n_elite, const double* w,
                    const double* hyper, uint64_t t, float* mean, double* sigma_io, double* cov, double* chol, double* p_sigma,
                    double* p_c, int32_t* status, double* yw_out, double* zw_out)
{
    constexpr int TE = glcma::TILE_E;
    const glcma::Hyper hp{hyper[0], hyper[1], hyper[2], hyper[3], hyper[4], hyper[5], hyper[6], hyper[7], hyper[8]};
    const size_t n_child = (size_t)P * K;
    const int NN = N * N;
    for (int p = 0; p < P; ++p) {
        const int32_t* elite = elite_k + (size_t)p * E;
        bool few = n_elite[p] < E;
        for (int e = 0; e < E; ++e) few = few || elite[e] < 0 || elite[e] >= K;
        if (t == 0 || few) { status[p] = t == 0 ? glcma::T_ZERO : glcma::FEW_ELITES; continue; }
        const double sigma = sigma_io[p];
        const double* L = chol + (size_t)p * NN;
        std::vector<float> m(N);
        for (int d = 0; d < N; ++d) m[d] = mean[((size_t)(d / NU) * P + p) * NU + d % NU];
        std::vector<double> yw(N, 0.0), R(NN, 0.0), y((size_t)TE * N), zw(N), acc(N);
        for (int e0 = 0; e0 < E; e0 += TE) {
            const int ne = E - e0 < TE ? E - e0 : TE;
            for (int e = 0; e < ne; ++e)
                for (int d = 0; d < N; ++d)
                    y[(size_t)e * N + d] = glcma::elite_y(theta[((size_t)(d / NU) * n_child + (size_t)p * K + elite[e0 + e]) * NU + d % NU], m[d], sigma);
            for (int d = 0; d < N; ++d)
                for (int e = 0; e < ne; ++e) yw[d] = glcma::add_yw(yw[d], w[e0 + e], y[(size_t)e * N + d]);
            for (int a = 0; a < N; ++a)
                for (int b = 0; b <= a; ++b)
                    for (int e = 0; e < ne; ++e) R[a * N + b] = glcma::add_r(R[a * N + b], w[e0 + e], y[(size_t)e * N + a], y[(size_t)e * N + b]);
        }
        for (int d = 0; d < N; ++d) acc[d] = yw[d];
        for (int j = 0; j < N; ++j) {
            zw[j] = acc[j] / L[j * N + j];
            for (int d = j + 1; d < N; ++d) acc[d] = glcma::fsub_take(acc[d], L[d * N + j], zw[j]);
        }
        if (yw_out) for (int d = 0; d < N; ++d) yw_out[(size_t)p * N + d] = yw[d];
        if (zw_out) for (int d = 0; d < N; ++d) zw_out[(size_t)p * N + d] = zw[d];
        const double qs = glcma::q_of(hp.c_sigma, hp.mu_eff), qc = glcma::q_of(hp.c_c, hp.mu_eff);
        std::vector<double> ps(N), pc(N), cv(NN), Ln(NN, 0.0);
        std::vector<float> mn(N);
        double n2 = 0.0;
        for (int d = 0; d < N; ++d) ps[d] = glcma::blend(hp.c_sigma, p_sigma[(size_t)p * N + d], glcma::times(qs, zw[d]));
        for (int d = 0; d < N; ++d) n2 = glcma::add_sq(n2, ps[d]);
        const double nrm = std::sqrt(n2);
        const bool hs = glcma::h_sigma(hp, N, t, nrm);
        bool bad = false;
        for (int d = 0; d < N; ++d) {
            pc[d] = glcma::blend(hp.c_c, p_c[(size_t)p * N + d], hs ? glcma::times(qc, yw[d]) : 0.0);
            mn[d] = glcma::new_mean(m[d], sigma, yw[d]);
            bad = bad || !std::isfinite(ps[d]) || !std::isfinite(pc[d]) || !std::isfinite(mn[d]);
        }
        const double sig = glcma::new_sigma(hp, sigma, nrm), a0 = glcma::a0_of(hp, hs);
        bad = bad || !std::isfinite(sig);
        for (int a = 0; a < N; ++a)
            for (int b = 0; b <= a; ++b) {
                const double v = glcma::cov_entry(hp, a0, cov[(size_t)p * NN + a * N + b], pc[a], pc[b], R[a * N + b]);
                cv[a * N + b] = cv[b * N + a] = v;
                bad = bad || !std::isfinite(v);
            }
        if (bad) { status[p] = glcma::NOT_FINITE; continue; }
        bool pivot_bad = false, inf = false;
        for (int j = 0; j < N; ++j) {
            const double s = glcma::chol_take(cv[j * N + j], &Ln[j * N], &Ln[j * N], j);
            pivot_bad = pivot_bad || !(s > 0.0);
            const double piv = std::sqrt(s);
            for (int i = j + 1; i < N; ++i) Ln[i * N + j] = glcma::chol_take(cv[i * N + j], &Ln[i * N], &Ln[j * N], j) / piv;
            Ln[j * N + j] = piv;
        }
        for (int i = 0; i < NN; ++i) inf = inf || !std::isfinite(Ln[i]);
        status[p] = pivot_bad ? glcma::NOT_POSITIVE : (inf ? glcma::NOT_FINITE : glcma::UPDATED);
        if (status[p] != glcma::UPDATED) continue;
        for (int i = 0; i < NN; ++i) { cov[(size_t)p * NN + i] = cv[i]; chol[(size_t)p * NN + i] = Ln[i]; }
        for (int d = 0; d < N; ++d) {
            p_sigma[(size_t)p * N + d] = ps[d];
            p_c[(size_t)p * N + d] = pc[d];
            mean[((size_t)(d / NU) * P + p) * NU + d % NU] = mn[d];
        }
        sigma_io[p] = sig;
    }
}

}  // extern "C"

#ifdef CMAHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// three generations at (P, K, N, E) on exactly sized buffers: sample, a made-up ranking, an update; the last row has too few elites
void drive(int P, int K, int N, int E)
{
    const int Ht = glcma::planes(N), NN = N * N;
    const size_t C = (size_t)P * K;
    std::vector<float> mean((size_t)Ht * P * NU, 0.f), theta((size_t)Ht * C * NU, 7.f);
    std::vector<double> sigma(P, 0.3), cov((size_t)P * NN, 0.0), chol((size_t)P * NN, 0.0), ps((size_t)P * N, 0.0), pc((size_t)P * N, 0.0), w(E);
    for (int p = 0; p < P; ++p)
        for (int d = 0; d < N; ++d) cov[(size_t)p * NN + d * N + d] = chol[(size_t)p * NN + d * N + d] = 1.0;
    for (size_t i = 0; i < mean.size(); ++i) mean[i] = (i % NU) + NU * ((i / NU) / P) < (size_t)N ? 0.1f * (float)((int)(i % 7) - 3) : 0.f;
    double sw = 0.0, sw2 = 0.0;
    for (int e = 0; e < E; ++e) { w[e] = (double)(E - e); sw += w[e]; }
    for (int e = 0; e < E; ++e) { w[e] /= sw; sw2 += w[e] * w[e]; }
    const double mu = 1.0 / sw2, n = (double)N;
    const double cs = (mu + 2.0) / (n + mu + 5.0), c1 = 2.0 / ((n + 1.3) * (n + 1.3) + mu);
    double cmu = 2.0 * (mu - 2.0 + 1.0 / mu) / ((n + 2.0) * (n + 2.0) + mu);
    if (cmu > 1.0 - c1) cmu = 1.0 - c1;
    const double hyper[9] = {mu, cs, 1.0 + cs, (4.0 + mu / n) / (n + 4.0 + 2.0 * mu / n), c1, cmu, std::sqrt(n) * (1.0 - 1.0 / (4.0 * n)), 1e-6, 1.0};
    std::vector<int32_t> elite((size_t)P * E), n_elite(P, E), status(P, 99);
    std::vector<double> yw((size_t)P * N), zw((size_t)P * N);
    for (uint64_t t = 1; t <= 3; ++t) {
        cmahost_sample(P, K, N, mean.data(), sigma.data(), chol.data(), 11u, t, theta.data());
        for (float v : theta) EXPECT(v >= -1.f && v <= 1.f);
        for (int h = 0; h < Ht; ++h)
            for (size_t c = 0; c < C; ++c)
                for (int j = 0; j < NU; ++j)
                    if (h * NU + j >= N) EXPECT(theta[((size_t)h * C + c) * NU + j] == 0.f);
        for (int p = 0; p < P; ++p)
            for (int e = 0; e < E; ++e) elite[(size_t)p * E + e] = (int32_t)((e * 7 + p + (int)t) % K);
        if (P > 1) n_elite[P - 1] = E - 1;
        cmahost_update(P, K, N, E, theta.data(), elite.data(), n_elite.data(), w.data(), hyper, t, mean.data(), sigma.data(), cov.data(),
                       chol.data(), ps.data(), pc.data(), status.data(), yw.data(), zw.data());
        for (int p = 0; p < P; ++p) {
            EXPECT(status[p] == (P > 1 && p == P - 1 ? glcma::FEW_ELITES : glcma::UPDATED));
            EXPECT(sigma[p] >= 1e-6 && sigma[p] <= 1.0);
            for (int i = 0; i < NN; ++i) EXPECT(std::isfinite(cov[(size_t)p * NN + i]) && std::isfinite(chol[(size_t)p * NN + i]));
            for (int a = 0; a < N; ++a)
                for (int b = a + 1; b < N; ++b) EXPECT(chol[(size_t)p * NN + a * N + b] == 0.0 && cov[(size_t)p * NN + a * N + b] == cov[(size_t)p * NN + b * N + a]);
        }
        if (P > 1) EXPECT(sigma[P - 1] == 0.3 && chol[(size_t)(P - 1) * NN] == 1.0 && ps[(size_t)(P - 1) * N] == 0.0);
    }
    // t = 0 and an elite index outside the row keep everything
    const std::vector<double> cov0 = cov, chol0 = chol;
    cmahost_update(P, K, N, E, theta.data(), elite.data(), n_elite.data(), w.data(), hyper, 0, mean.data(), sigma.data(), cov.data(),
                   chol.data(), ps.data(), pc.data(), status.data(), nullptr, nullptr);
    for (int p = 0; p < P; ++p) EXPECT(status[p] == glcma::T_ZERO);
    elite[0] = K;
    cmahost_update(P, K, N, E, theta.data(), elite.data(), n_elite.data(), w.data(), hyper, 4, mean.data(), sigma.data(), cov.data(),
                   chol.data(), ps.data(), pc.data(), status.data(), nullptr, nullptr);
    EXPECT(status[0] == glcma::FEW_ELITES);
    if (P == 1) EXPECT(cov == cov0 && chol == chol0);
}

}  // namespace

int main()
{
    EXPECT(cmahost_sizeof(0) > 0 && cmahost_sizeof(1) > 0 && cmahost_sizeof(2) == glcma::NMAX);
    drive(1, 2, 1, 1);
    drive(3, 6, 5, 3);
    drive(2, 66, 6, 33);
    drive(2, 66, 7, 66);
    drive(1, 258, 29, 129);
    drive(3, 70, 32, 35);
    std::printf(failures ? "cmahost FAILED (%d)\n" : "cmahost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
