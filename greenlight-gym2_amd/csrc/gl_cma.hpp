// gl_cma.hpp -- the scalar logic of the full-covariance CMA-ES stages between two rollouts (include/glgym.h glgym_plan_cma_sample,
// glgym_plan_cma_update), for host and device code alike:
//   sample_child    one child c = p*K + k: the CEM stream's normals z, plane after plane -> y = chol z, accumulated COLUMN by column
//                   (draw z_j, add its column into every y_i with i >= j), so that only y is live -> clip(mean + sigma * y)
//   elite_y, add_yw, add_r
//                   what ONE thread adds, elite after elite, to the component of yw or the entry of R that it owns
//   fsub_take, fsub_div
//                   forward substitution zw = chol^-1 yw with lanes on rows: lane i starts from yw[i], takes chol[i][j] * zw[j] away
//                   for j = 0, 1, .. i-1 and divides by chol[i][i]
//   q_of, blend, h_sigma, a0_of, cov_entry, new_mean, new_sigma
//                   the evolution paths, the covariance entry, the mean and the step size
//   chol_take, and the division by the pivot
//                   the row-oriented Cholesky factorisation with lanes on rows i, j sequential
// Everything is double with products and sums rounded separately, as in gl_cem.hpp and gl_es.hpp.  There is no RNG of its own: the
// normals are glcem::normals_of.
//
// Evaluation orders (N components; component i lives at plane h = i / 6, slot j = i % 6; Ht = ceil(N / 6)):
//   y_i       = sum_{j <= i} chol[i][j] * z_j, from 0.0, j ascending, each product rounded, then added
//   theta     = (float) clip1((double) mean + sigma * y_i); a slot i >= N stores 0.0f
//   y_e[d]    = ((double) x_e[d] - (double) mean[d]) / sigma
//   yw[d]     = sum_e w_e * y_e[d], from 0.0, e ascending
//   R[a][b]   = sum_e (w_e * y_e[a]) * y_e[b], from 0.0, e ascending (b <= a)
//   zw[i]     = (yw[i] - chol[i][0] * zw[0] - chol[i][1] * zw[1] - ..) / chol[i][i], each product subtracted in turn
//   q(c)      = sqrt((c * (2 - c)) * mu_eff)
//   p_sigma'  = (1 - c_sigma) * p_sigma + q(c_sigma) * zw
//   n2        = sum_d p_sigma'[d] * p_sigma'[d], from 0.0, d ascending; nrm = sqrt(n2)
//   h_sigma   = nrm / sqrt(1 - pow_t(1 - c_sigma, 2 t)) < (1.4 + 2 / (N + 1)) * chi_n
//   p_c'      = (1 - c_c) * p_c + (h_sigma ? q(c_c) * yw : 0.0)
//   a0        = ((1 - c_1) - c_mu) + (h_sigma ? 0.0 : (c_1 * c_c) * (2 - c_c))
//   cov'[a][b]= (a0 * cov[a][b] + c_1 * (p_c'[a] * p_c'[b])) + c_mu * R[a][b]
//   mean'     = (float) clip1((double) mean + sigma * yw)
//   sigma'    = min(max(sigma * exp((c_sigma / d_sigma) * (nrm / chi_n - 1)), min_sigma), max_sigma)
//   Cholesky  for j = 0 .. N-1: s = cov'[j][j] - chol'[j][0]^2 - .. - chol'[j][j-1]^2, chol'[j][j] = sqrt(s); for i > j:
//             chol'[i][j] = (cov'[i][j] - chol'[i][0] * chol'[j][0] - .. - chol'[i][j-1] * chol'[j][j-1]) / chol'[j][j]
#pragma once
#include "gl_cem.hpp"
#include "gl_es.hpp"

#if defined(__clang__)
#define GLCMA_UNROLL _Pragma("unroll")
#else
#define GLCMA_UNROLL
#endif

namespace glcma {

using glplan::NU;
using glplan::WAVE;

constexpr int NMAX = 32;                         // GLGYM_CMA_NMAX
constexpr int HTMAX = (NMAX + NU - 1) / NU;      // planes of theta at N = NMAX
constexpr int TILE_E = 32;                       // elites per round of the host instantiation (the kernel stages min(256, 1 024 / N); every
                                                 // sum over the elites runs in e ascending inside its owner, so the tile depth changes no bit)
enum { UPDATED = 0, FEW_ELITES = 1, NOT_FINITE = 2, NOT_POSITIVE = 3, T_ZERO = 4 };

struct Hyper {
    double mu_eff, c_sigma, d_sigma, c_c, c_1, c_mu, chi_n, min_sigma, max_sigma;
};

GLPLAN_HD int planes(int N) { return (N + NU - 1) / NU; }

// The Ht rows theta[h][c][0..5] of child c = p*K + k.  chol: the row's factor [N][N] (in the kernel: staged in LDS, every read a
// broadcast); mean: the whole [Ht][P][6] array.  y is indexed by unrolled loops only (registers, no scratch): the loop over the planes
// is a run-time loop for the draws -- the costly part -- and an unrolled one for the stores.
GLPLAN_HD void sample_child(int c, int p, int P, int K, int N, uint64_t D, uint64_t seed, const double* chol, const float* mean, double sigma,
                            float* theta)
{
#pragma clang fp contract(off)
    const int Ht = planes(N);
    const size_t n_child = (size_t)P * K;
    double y[NMAX];
    GLCMA_UNROLL
    for (int i = 0; i < NMAX; ++i) y[i] = 0.0;
    for (int h = 0; h < Ht; ++h) {
        double e[NU];
        glcem::normals_of(c, h, D, seed, e);
        GLCMA_UNROLL
        for (int j = 0; j < NU; ++j) {
            const int col = h * NU + j;
            if (col >= N) continue;
            const double z = e[j];
            GLCMA_UNROLL
            for (int i = 0; i < NMAX; ++i)
                if (i >= col && i < N) {
                    const double t = chol[i * N + col] * z;
                    y[i] = y[i] + t;
                }
        }
    }
    GLCMA_UNROLL
    for (int h = 0; h < HTMAX; ++h) {
        if (h >= Ht) continue;
        float* out = theta + ((size_t)h * n_child + c) * NU;
        const float* m = mean + ((size_t)h * P + p) * NU;
        GLCMA_UNROLL
        for (int j = 0; j < NU; ++j) {
            const int i = h * NU + j;
            float v = 0.f;
            if (i < NMAX && i < N) {
                const double t = sigma * y[i < NMAX ? i : 0];
                v = (float)glcem::clip1((double)m[j] + t);
            }
            out[j] = v;
        }
    }
}

// ---- update ------------------------------------------------------------------------------------------------------------------------
GLPLAN_HD double elite_y(float x, float mean, double sigma) { return ((double)x - (double)mean) / sigma; }

GLPLAN_HD double add_yw(double acc, double w, double y)
{
#pragma clang fp contract(off)
    const double t = w * y;
    return acc + t;
}

GLPLAN_HD double add_r(double acc, double w, double ya, double yb)
{
#pragma clang fp contract(off)
    const double t = w * ya;
    const double u = t * yb;
    return acc + u;
}

// acc - l * z, the product rounded first: one term of the forward substitution
GLPLAN_HD double fsub_take(double acc, double l, double z)
{
#pragma clang fp contract(off)
    const double t = l * z;
    return acc - t;
}

GLPLAN_HD double q_of(double c, double mu_eff)
{
#pragma clang fp contract(off)
    const double a = c * (2.0 - c);
    return std::sqrt(a * mu_eff);
}

// (1 - c) * p + t
GLPLAN_HD double blend(double c, double p, double t)
{
#pragma clang fp contract(off)
    const double a = (1.0 - c) * p;
    return a + t;
}

GLPLAN_HD double times(double a, double b)
{
#pragma clang fp contract(off)
    return a * b;
}

GLPLAN_HD double add_sq(double acc, double v)
{
#pragma clang fp contract(off)
    const double t = v * v;
    return acc + t;
}

GLPLAN_HD bool h_sigma(const Hyper& hp, int N, uint64_t t, double nrm)
{
#pragma clang fp contract(off)
    const double g = 1.0 - gles::pow_t(1.0 - hp.c_sigma, 2u * t);
    const double lhs = nrm / std::sqrt(g);
    const double rhs = (1.4 + 2.0 / (double)(N + 1)) * hp.chi_n;
    return lhs < rhs;
}

GLPLAN_HD double a0_of(const Hyper& hp, bool hs)
{
#pragma clang fp contract(off)
    const double a = (1.0 - hp.c_1) - hp.c_mu;
    const double b = hs ? 0.0 : (hp.c_1 * hp.c_c) * (2.0 - hp.c_c);
    return a + b;
}

GLPLAN_HD double cov_entry(const Hyper& hp, double a0, double cov, double pca, double pcb, double r)
{
#pragma clang fp contract(off)
    const double t0 = a0 * cov;
    const double pp = pca * pcb;
    const double t1 = hp.c_1 * pp;
    const double s = t0 + t1;
    const double t2 = hp.c_mu * r;
    return s + t2;
}

GLPLAN_HD float new_mean(float mean, double sigma, double yw)
{
#pragma clang fp contract(off)
    const double t = sigma * yw;
    return (float)glcem::clip1((double)mean + t);
}

// a NaN falls to min_sigma (the row is then kept anyway: nrm is not finite only if p_sigma' is not)
GLPLAN_HD double new_sigma(const Hyper& hp, double sigma, double nrm)
{
#pragma clang fp contract(off)
    const double x = (hp.c_sigma / hp.d_sigma) * (nrm / hp.chi_n - 1.0);
    const double v = sigma * std::exp(x);
    const double lo = v > hp.min_sigma ? v : hp.min_sigma;
    return lo < hp.max_sigma ? lo : hp.max_sigma;
}

// cov'[i][j] - sum_{k < j} chol'[i][k] * chol'[j][k], each product subtracted in turn: the pivot's radicand s for i = j, the
// numerator of chol'[i][j] for i > j.  row_i, row_j: rows i and j of the new factor, columns 0 .. j-1 complete.
GLPLAN_HD double chol_take(double cov_ij, const double* row_i, const double* row_j, int j)
{
#pragma clang fp contract(off)
    double v = cov_ij;
    for (int k = 0; k < j; ++k) {
        const double t = row_i[k] * row_j[k];
        v = v - t;
    }
    return v;
}

}  // namespace glcma
