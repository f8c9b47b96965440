// TESTS ONLY.  What tests/bdfwave/bdfwave.hip (one wavefront per problem, the product's team of gl_bdf_wave.hpp) and
// tests/bdfwave/bdfwave_host.cpp (a team of one lane) have in common: the synthetic right-hand sides and one problem of every entry
// point, written for a team like gl_bdf.hpp itself so that both run the same source around the same bdf_lu_factor, bdf_change_D,
// bdf_rms and bdf_step.  The product library never includes this file.
#pragma once
#include <cmath>
#include <cstdint>

#include "gl_bdf.hpp"

namespace bdfwave {

using glbdf::BdfScratch;
using glbdf::NX;

enum { RHS_LINEAR = 0, RHS_SQUARE = 1, RHS_VDP = 2, RHS_SQUARE_NAN = 3 };

// kind 0: A y + g (row-major A, fused multiply-adds in ascending column order on either side)
// kind 1: y_i' = y_i^2                      kind 3: the same, NaN wherever |y_i| > 1e6
// kind 2: Van der Pol (mu) in states 0, 1 and y_i' = -0.01 i y_i in the rest
struct SynthRhs {
    int kind;
    const double* A;
    const double* g;
    double mu;
    GL_HD void operator()(const double* xs, double* k) const
    {
        if (kind == RHS_LINEAR) {
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                double a = g[i];
#pragma unroll
                for (int j = 0; j < NX; ++j) a = ::fma(A[i * NX + j], xs[j], a);
                k[i] = a;
            }
        } else if (kind == RHS_VDP) {
#pragma unroll
            for (int i = 2; i < NX; ++i) k[i] = -0.01 * (double)i * xs[i];
            k[0] = xs[1];
            k[1] = ::fma(mu * (1.0 - xs[0] * xs[0]), xs[1], -xs[0]);
        } else {
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                const double v = xs[i] * xs[i];
                k[i] = (kind == RHS_SQUARE_NAN && ::fabs(xs[i]) > 1e6) ? __builtin_nan("") : v;
            }
        }
    }
};

struct NoRhs {
    GL_HD void operator()(const double*, double*) const {}
};

#define BDFWAVE_FOR(i, n) for (int i = tm.lane(); i < (n); i += Team::width)

// rms[l] = bdf_rms(v over scale) as lane l holds it (a team of one fills all 64 slots from its one lane)
template <class Team> GL_HD double rms_problem(const Team& tm, BdfScratch& sh, const double* v, const double* scale)
{
    BDFWAVE_FOR(i, NX) { sh.dy[i] = v[i]; sh.scale[i] = scale[i]; }
    tm.sync();
    return glbdf::bdf_rms(tm, [&](int i) { return sh.dy[i]; }, sh.scale);
}

// J, c, b -> ok = bdf_lu_factor, LU, piv, perm (entries the factorisation did not reach stay -1), x = lu_solve(b) when ok (else b)
template <class Team>
GL_HD void lu_problem(const Team& tm, BdfScratch& sh, const double* J, double c, const double* b, int* ok, double* LU, int* piv, int* perm,
                      double* x)
{
    BDFWAVE_FOR(e, NX * NX) sh.J[e] = J[e];
    BDFWAVE_FOR(i, NX) { sh.dy[i] = b[i]; sh.piv[i] = -1; sh.perm[i] = -1; }
    tm.sync();
    const bool good = glbdf::bdf_lu_factor(tm, sh, c);
    tm.sync();
    if (good) tm.lu_solve(sh, sh.dy);
    BDFWAVE_FOR(e, NX * NX) LU[e] = sh.LU[e];
    BDFWAVE_FOR(i, NX) { piv[i] = sh.piv[i]; perm[i] = sh.perm[i]; x[i] = sh.dy[i]; }
    if (tm.lane() == 0) *ok = good ? 1 : 0;
}

// D[8][28] -> bdf_change_D(order, factor) -> D
template <class Team> GL_HD void change_D_problem(const Team& tm, BdfScratch& sh, const double* D, int order, double factor, double* Dout)
{
    constexpr int ND = (glbdf::MAXORD + 3) * NX;
    BDFWAVE_FOR(e, ND) sh.D[e / NX][e % NX] = D[e];
    tm.sync();
    glbdf::bdf_change_D(tm, sh, order, factor);
    BDFWAVE_FOR(e, ND) Dout[e] = sh.D[e / NX][e % NX];
}

// y0 -> bdf_step -> y, stats[5], rc (the team's right-hand side is the problem's)
template <class Team>
GL_HD void step_problem(const Team& tm, BdfScratch& sh, const double* y0, double dt, double rtol, double atol, int max_steps, double* y,
                        int32_t* stats, int* rc)
{
    BDFWAVE_FOR(i, NX) sh.D[0][i] = y0[i];
    tm.sync();
    int32_t st[glbdf::NSTAT] = {0, 0, 0, 0, 0};
    const int r = glbdf::bdf_step(tm, sh, dt, rtol, atol, max_steps, st);
    tm.sync();
    BDFWAVE_FOR(i, NX) y[i] = sh.D[0][i];
    if (tm.lane() == 0) {
        for (int i = 0; i < glbdf::NSTAT; ++i) stats[i] = st[i];
        *rc = r;
    }
}

// x -> f = eval1(x); need_f0: f0 = the Jacobian call's own base point, else f0 is read; J = jac(x)
template <class Team>
GL_HD void jac_problem(const Team& tm, BdfScratch& sh, const double* x, int need_f0, double* f, double* f0, double* J)
{
    BDFWAVE_FOR(i, NX) { sh.ypred[i] = x[i]; sh.f[i] = need_f0 ? 0.0 : f0[i]; }
    tm.sync();
    tm.eval1(sh.ypred, sh.fy);
    tm.jac(sh.ypred, sh.f, need_f0 != 0, sh.J);
    tm.sync();
    BDFWAVE_FOR(i, NX) { f[i] = sh.fy[i]; f0[i] = sh.f[i]; }
    BDFWAVE_FOR(e, NX * NX) J[e] = sh.J[e];
}

#undef BDFWAVE_FOR

}  // namespace bdfwave
