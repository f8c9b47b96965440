// gl_es.hpp -- the scalar logic of the evolution strategy's stages between two rollouts (include/glgym.h glgym_plan_es_sample,
// glgym_plan_es_utilities, glgym_plan_es_update), for host and device code alike:
//   pair_rows       one mirrored pair q = p*M + m (children c+ = 2q, c- = 2q + 1) at one plane h: the CEM stream's normals e of the EVEN
//                   child, drawn once, -> clip(mean + std * e) and clip(mean - std * e): 12 consecutive floats
//   utility         the centred rank of one candidate from its rank by counting (gl_cem.hpp key / count_chunk) and the number of
//                   admissible candidates of its row
//   lane_terms      what ONE lane of the updating wavefront sums over its pairs m = lane, lane + 64, ... ascending: the search
//                   gradient's and the spread statistic's terms; the wavefront combines the 64 partial sums with gl_plan.hpp's
//                   butterfly (tests/eshost/eshost.cpp: a loop over an array of 64) and divides by M
//   pow_t, Hyper, adam_step, sgd_step, new_std, finite6
//                   what lane 0 then does with the six sums of its (row, plane)
// Everything is double with products and sums rounded separately, as in gl_cem.hpp.
//
// pow_t(b, t) = b^t by square-and-multiply from the LEAST significant bit of t: r = 1, q = b; while t != 0: if t is odd r = r * q;
// t = t >> 1; if t != 0 q = q * q.  (t = 5: r = b, q = b^2, q = b^4, r = b * b^4.)
#pragma once
#include "gl_cem.hpp"

namespace gles {

using glplan::NU;
using glplan::WAVE;

constexpr int SGD = 0, ADAM = 1;                 // GLGYM_ES_SGD, GLGYM_ES_ADAM

// rows[0..5] = theta[h][2q][.], rows[6..11] = theta[h][2q + 1][.]; mean / sd: the six values of (h, p)
GLPLAN_HD void pair_rows(int q, int h, uint64_t D, uint64_t seed, const float* mean, const float* sd, float rows[2 * NU])
{
    double e[NU];
    glcem::normals_of(2 * q, h, D, seed, e);
    for (int j = 0; j < NU; ++j) {
        rows[j] = glcem::action(mean[j], sd[j], e[j]);
        rows[NU + j] = glcem::action(mean[j], sd[j], -e[j]);
    }
}

// u of a candidate with `rank` admissible candidates before it, among n_adm admissible ones of its row
GLPLAN_HD double utility(bool adm, int rank, int n_adm)
{
    if (n_adm < 2) return 0.0;
    if (!adm) return -0.5;
    return 0.5 - (double)rank / (double)(n_adm - 1);
}

// One pair into a lane's sums.  rows: its 12 floats; up, um: u of c+ and c-; sigma: the current std of the six components.
//   d = (theta+ - theta-) / 2 (exact: both are float32);  g += (up - um) * d;  z = d / sigma;  s += (up + um) * (z * z - 1)
// A component whose sigma is not > 0 adds nothing to s.
GLPLAN_HD void pair_terms(const float rows[2 * NU], double up, double um, const double sigma[NU], double g[NU], double s[NU])
{
#pragma clang fp contract(off)
    const double du = up - um, su = up + um;
    for (int j = 0; j < NU; ++j) {
        const double d = ((double)rows[j] - (double)rows[NU + j]) * 0.5;
        const double tg = du * d;
        g[j] = g[j] + tg;
        if (sigma[j] > 0.0) {
            const double z = d / sigma[j];
            const double z2 = z * z;
            const double ts = su * (z2 - 1.0);
            s[j] = s[j] + ts;
        }
    }
}

// this lane's share of both sums; rows = the row's K rows of one plane, [K][6] f32; u = the row's K utilities
GLPLAN_HD void lane_terms(int lane, int M, const float* rows, const double* u, const double sigma[NU], double g[NU], double s[NU])
{
    for (int j = 0; j < NU; ++j) g[j] = s[j] = 0.0;
    for (int m = lane; m < M; m += WAVE) pair_terms(rows + (size_t)m * 2 * NU, u[2 * m], u[2 * m + 1], sigma, g, s);
}

GLPLAN_HD double pow_t(double b, uint64_t t)
{
#pragma clang fp contract(off)
    double r = 1.0, q = b;
    while (t) {
        if (t & 1u) r = r * q;
        t >>= 1;
        if (t) q = q * q;
    }
    return r;
}

struct Hyper {
    int optimizer;
    double lr, lr_std, std_decay, min_std, max_std, beta1, beta2, eps;
};

GLPLAN_HD bool finite6(const double v[NU])
{
    bool ok = true;
    for (int j = 0; j < NU; ++j) ok = ok && std::isfinite(v[j]);
    return ok;
}

GLPLAN_HD double sgd_step(const Hyper& hp, double g)
{
#pragma clang fp contract(off)
    return hp.lr * g;
}

// c1 = 1 - beta1^t, c2 = 1 - beta2^t.  m1 = beta1*m1 + (1 - beta1)*g; m2 = beta2*m2 + (1 - beta2)*(g*g);
// step = (lr * (m1 / c1)) / (sqrt(m2 / c2) + eps)
GLPLAN_HD double adam_step(const Hyper& hp, double c1, double c2, double g, double& m1, double& m2)
{
#pragma clang fp contract(off)
    const double a1 = hp.beta1 * m1, b1 = (1.0 - hp.beta1) * g;
    m1 = a1 + b1;
    const double g2 = g * g;
    const double a2 = hp.beta2 * m2, b2 = (1.0 - hp.beta2) * g2;
    m2 = a2 + b2;
    const double num = hp.lr * (m1 / c1), den = std::sqrt(m2 / c2) + hp.eps;
    return num / den;
}

// min(max((sigma * std_decay) * exp((0.5 * lr_std) * s), min_std), max_std); a NaN falls to min_std
GLPLAN_HD double new_std(const Hyper& hp, double sigma, double s)
{
#pragma clang fp contract(off)
    const double x = (0.5 * hp.lr_std) * s;
    const double v = (sigma * hp.std_decay) * std::exp(x);
    const double lo = v > hp.min_std ? v : hp.min_std;
    return lo < hp.max_std ? lo : hp.max_std;
}

// Lane 0 of (row p, plane h): the six components at offset o = (h*P + p)*6, given the wavefront's sums divided by M.
// keep: the row keeps mean, std and moments.  mean / sd are read before the (possibly aliased) stores.
GLPLAN_HD void update_row(const Hyper& hp, uint64_t t, bool keep, const double g[NU], const double s[NU], const float* mean,
                          const float* sd, double* m1, double* m2, float* mean_out, float* std_out)
{
#pragma clang fp contract(off)
    const bool adam = hp.optimizer == ADAM;
    const double c1 = adam ? 1.0 - pow_t(hp.beta1, t) : 1.0, c2 = adam ? 1.0 - pow_t(hp.beta2, t) : 1.0;
    for (int j = 0; j < NU; ++j) {
        const float mu = mean[j], sg = sd[j];
        if (keep) { mean_out[j] = mu; std_out[j] = sg; continue; }
        double step;
        if (adam) {
            double a = m1[j], b = m2[j];
            step = adam_step(hp, c1, c2, g[j], a, b);
            m1[j] = a; m2[j] = b;
        } else {
            step = sgd_step(hp, g[j]);
        }
        mean_out[j] = (float)((double)mu + step);
        std_out[j] = (float)new_std(hp, (double)sg, s[j]);
    }
}

}  // namespace gles
