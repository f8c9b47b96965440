// gl_bdf.hpp -- adaptive, error-controlled implicit step map for glgym_evalF (GLGYM_INTEGRATOR_BDF).
//
// Algorithm: variable-order (1-5), variable-step BDF / NDF in difference form with a fixed leading coefficient, modified Newton
// iterations and a finite-difference Jacobian that is reused until the iteration stops converging -- the formulation of
// L. F. Shampine and M. W. Reichelt, "The MATLAB ODE Suite", SIAM J. Sci. Comput. 18 (1997) 1-22 (NDF kappa coefficients,
// the difference array and its rescaling), as scipy.integrate.BDF documents it, with the initial step of Hairer, Norsett &
// Wanner, "Solving ODEs I", section II.4.  Every decision -- Newton limit and convergence test, Jacobian reuse, finite-difference
// increment, step and order selection, initial step, step-size underflow -- is that of the repository's CPU restatement, so the
// device result can be checked row by row.  The right-hand side is the product's own rhs<double, true, false> (gl_model.hpp),
// the full right-hand side at every evaluation.
//
// Written once for a "team" of lanes that integrates ONE row:
//   Team::width            lanes of the team (64 on the device: one wavefront per row; 1 on the host)
//   tm.lane()              this lane's index
//   tm.sum(v)              sum of v over the team, the same bits in every lane
//   tm.argmax(v, i)        (v, i) of the largest v over the team, the smallest i among equal v, in every lane
//   tm.sync()              orders the team's scratch writes before its reads
//   tm.eval1(x, f)         f = rhs(x) (one evaluation)
//   tm.jac(x, f0, need, J) J[i][j] = (rhs(x + dx_j e_j)_i - f0_i) / dx_j, with f0 = rhs(x) evaluated first when `need`
//   tm.lu_solve(s, b)      b <- (I - c J)^-1 b with the factors of bdf_lu_factor (team of one: bdf_lu_solve_serial)
// Vectors of 28 states and the matrices live in a BdfScratch the team shares (LDS on the device, a plain struct on the host);
// lane i of the team owns state i in every vector operation.  Scalars (step size, order, counters) are held by every lane
// alike, so every branch is uniform over the team.
#pragma once
#include <cmath>
#include <cstdint>

#include "gl_model.hpp"

namespace glbdf {

using glm::NX;
constexpr int MAXORD = 5;
constexpr int NEWTON_MAXITER = 4;
constexpr long MAX_RHS = 100000;    // hard cap on right-hand sides per row and env-step: beyond it the row has failed
enum { ST_STEPS = 0, ST_NFEV = 1, ST_NJEV = 2, ST_NLU = 3, ST_ORDER = 4, NSTAT = 5 };
enum { BDF_OK = 0, BDF_FAIL_STEPS = 1, BDF_FAIL_RHS = 2, BDF_FAIL_UNDERFLOW = 3, BDF_FAIL_NONFINITE = 4, BDF_FAIL_SINGULAR = 5 };

struct BdfScratch {
    double D[MAXORD + 3][NX];        // difference array
    double J[NX * NX];               // Jacobian, row-major
    double LU[NX * NX];              // P (I - c J) = L U, row-major, multipliers below the diagonal
    double f[NX], scale[NX], ypred[NX], psi[NX], ynew[NX], dd[NX], dy[NX], fy[NX], y1[NX];
    double R[MAXORD + 1][MAXORD + 1], RU[MAXORD + 1][MAXORD + 1];
    int perm[NX];                    // row i of P A is row perm[i] of A
    int piv[NX];
};

// NDF coefficients (Shampine & Reichelt 1997, table 1): kappa_k; gamma_k = sum_{j <= k} 1/j; alpha_k = (1 - kappa_k) gamma_k;
// error constant kappa_k gamma_k + 1/(k+1).  Functions of the order (wave-uniform), no indexed tables.
GL_HD double bdf_kappa(int k) { return k == 1 ? -0.1850 : k == 2 ? -1.0 / 9.0 : k == 3 ? -0.0823 : k == 4 ? -0.0415 : 0.0; }
GL_HD double bdf_gamma(int k)
{
    double g = 0.0;
#pragma unroll
    for (int j = 1; j <= MAXORD; ++j)
        if (j <= k) g = g + 1.0 / (double)j;
    return g;
}
GL_HD double bdf_alpha(int k) { return (1.0 - bdf_kappa(k)) * bdf_gamma(k); }
GL_HD double bdf_error_const(int k) { return bdf_kappa(k) * bdf_gamma(k) + 1.0 / (double)(k + 1); }

#define GL_BDF_FOR(i, n) for (int i = tm.lane(); i < (n); i += Team::width)

// weighted RMS norm of v_i = V(i) over scale
template <class Team, class V> GL_HD double bdf_rms(const Team& tm, V v, const double* scale)
{
    double e = 0.0;
    GL_BDF_FOR(i, NX) { const double r = v(i) / scale[i]; e += r * r; }
    e = tm.sum(e);
    return ::sqrt(e / NX);
}

// lane j: column j of R(order, factor), R[0][j] = 1, R[i][j] = R[i-1][j] (i - 1 - factor j) / i
GL_HD void bdf_R_column(int order, double factor, int j, double* r)
{
    r[0] = 1.0;
#pragma unroll
    for (int i = 1; i <= MAXORD; ++i)
        r[i] = (i <= order && j >= 1) ? r[i - 1] * ((double)(i - 1) - factor * (double)j) / (double)i : 0.0;
}

// D[0..order] <- (R(factor) U)^T D[0..order], U = R(1): rescales the differences to the step size h * factor
template <class Team> GL_HD void bdf_change_D(const Team& tm, BdfScratch& s, int order, double factor)
{
    GL_BDF_FOR(j, order + 1) {
        double r[MAXORD + 1];
        bdf_R_column(order, factor, j, r);
#pragma unroll
        for (int i = 0; i <= MAXORD; ++i)
            if (i <= order) s.R[i][j] = r[i];
    }
    tm.sync();
    GL_BDF_FOR(j, order + 1) {
        double u[MAXORD + 1];
        bdf_R_column(order, 1.0, j, u);
        for (int i = 0; i <= order; ++i) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k <= MAXORD; ++k)
                if (k <= order) a += s.R[i][k] * u[k];
            s.RU[i][j] = a;
        }
    }
    tm.sync();
    GL_BDF_FOR(c, NX) {
        double d[MAXORD + 1], t[MAXORD + 1];
#pragma unroll
        for (int k = 0; k <= MAXORD; ++k) d[k] = k <= order ? s.D[k][c] : 0.0;
#pragma unroll
        for (int i = 0; i <= MAXORD; ++i) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k <= MAXORD; ++k)
                if (k <= order && i <= order) a += s.RU[k][i] * d[k];
            t[i] = a;
        }
#pragma unroll
        for (int i = 0; i <= MAXORD; ++i)
            if (i <= order) s.D[i][c] = t[i];
    }
    tm.sync();
}

// s.LU <- P (I - c J) = L U with partial pivoting (row swaps of whole rows, the first largest |pivot|).  false: singular.
template <class Team> GL_HD bool bdf_lu_factor(const Team& tm, BdfScratch& s, double c)
{
    GL_BDF_FOR(e, NX * NX) {
        const int i = e / NX, j = e - i * NX;
        double v = -c * s.J[e];
        if (i == j) v += 1.0;
        s.LU[e] = v;
    }
    tm.sync();
    for (int k = 0; k < NX; ++k) {
        double best = -1.0;
        int m = NX;
        GL_BDF_FOR(i, NX) {
            const double a = i >= k ? ::fabs(s.LU[i * NX + k]) : -1.0;
            if (a > best) { best = a; m = i; }
        }
        tm.argmax(best, m);
        if (!(best > 0.0)) return false;               // zero (or non-finite) column: singular
        if (tm.lane() == 0) s.piv[k] = m;
        if (m != k) {
            GL_BDF_FOR(j, NX) { const double t = s.LU[k * NX + j]; s.LU[k * NX + j] = s.LU[m * NX + j]; s.LU[m * NX + j] = t; }
            tm.sync();
        }
        GL_BDF_FOR(i, NX)
            if (i > k) s.LU[i * NX + k] /= s.LU[k * NX + k];
        tm.sync();
        const int n = NX - 1 - k;
        GL_BDF_FOR(e, n * n) {
            const int i = k + 1 + e / n, j = k + 1 + e % n;
            s.LU[i * NX + j] -= s.LU[i * NX + k] * s.LU[k * NX + j];
        }
        tm.sync();
    }
    if (tm.lane() == 0) {
        for (int i = 0; i < NX; ++i) s.perm[i] = i;
        for (int k = 0; k < NX; ++k) { const int t = s.perm[k]; s.perm[k] = s.perm[s.piv[k]]; s.perm[s.piv[k]] = t; }
    }
    tm.sync();
    return true;
}

// b <- (I - c J)^-1 b on a team of one: permute, forward elimination (unit L), back substitution (U) row by row in ascending column
// order -- the serial algorithm's order of operations.  (The wavefront's solve, WaveTeam::lu_solve in gl_bdf_wave.hpp, keeps the
// forward sweep's order and runs the back substitution as a column sweep in registers.)
GL_HD void bdf_lu_solve_serial(BdfScratch& s, double* b)
{
    double* w = s.y1;
    for (int i = 0; i < NX; ++i) w[i] = b[s.perm[i]];
    for (int k = 0; k < NX - 1; ++k)
        for (int i = k + 1; i < NX; ++i) w[i] -= s.LU[i * NX + k] * w[k];
    for (int k = NX - 1; k >= 0; --k) {
        for (int j = k + 1; j < NX; ++j) w[k] -= s.LU[k * NX + j] * w[j];
        w[k] /= s.LU[k * NX + k];
    }
    for (int i = 0; i < NX; ++i) b[i] = w[i];
}

// One env-step x(0) = x0 -> x(dt) with rtol / atol.  x0 is read from s.D[0] (the caller stores it there); the result is s.D[0].
// stats[NSTAT] = steps, right-hand sides, Jacobians, LU factorisations, final order.  Returns BDF_OK or the reason of the failure.
template <class Team>
GL_HD int bdf_step(const Team& tm, BdfScratch& s, double dt, double rtol, double atol, int max_steps, int32_t* stats)
{
    const double newton_tol = ::fmax(10.0 * 2.220446049250313e-16 / rtol, ::fmin(0.03, ::sqrt(rtol)));
    long nfev = 0, nsteps = 0, njev = 0, nlu = 0;
    int order = 1, status = BDF_OK;
    double* y = s.D[0];
    tm.eval1(y, s.f); ++nfev;
    // initial step (Hairer, Norsett & Wanner II.4, order 1)
    double h_abs;
    {
        GL_BDF_FOR(i, NX) s.scale[i] = atol + rtol * ::fabs(y[i]);
        tm.sync();
        const double d0 = bdf_rms(tm, [&](int i) { return y[i]; }, s.scale), d1 = bdf_rms(tm, [&](int i) { return s.f[i]; }, s.scale);
        const double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
        GL_BDF_FOR(i, NX) s.y1[i] = y[i] + h0 * s.f[i];
        tm.sync();
        tm.eval1(s.y1, s.fy); ++nfev;
        const double d2 = bdf_rms(tm, [&](int i) { return s.fy[i] - s.f[i]; }, s.scale) / h0;
        const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? ::fmax(1e-6, h0 * 1e-3) : ::pow(0.01 / ::fmax(d1, d2), 0.5);
        h_abs = ::fmin(::fmin(100.0 * h0, h1), dt);
    }
    tm.jac(y, s.f, false, s.J); nfev += NX; ++njev;
    GL_BDF_FOR(i, NX) {
        s.D[1][i] = s.f[i] * h_abs;
#pragma unroll
        for (int k = 2; k < MAXORD + 3; ++k) s.D[k][i] = 0.0;
    }
    tm.sync();
    int n_equal_steps = 0, lu_valid = 0, current_jac = 1;
    double t = 0.0;
    while (t < dt * (1.0 - 1e-14)) {
        if (nsteps >= max_steps) { status = BDF_FAIL_STEPS; break; }
        if (h_abs > dt - t) {                                    // land exactly on dt
            bdf_change_D(tm, s, order, (dt - t) / h_abs);
            h_abs = dt - t; n_equal_steps = 0; lu_valid = 0;
        }
        int step_accepted = 0, n_iter = 0;
        double error_norm = 0.0, safety = 0.9;
        while (!step_accepted) {
            if (h_abs < 1e-12 * dt) { status = BDF_FAIL_UNDERFLOW; break; }
            if (nfev > MAX_RHS) { status = BDF_FAIL_RHS; break; }
            const double alpha = bdf_alpha(order);
            GL_BDF_FOR(i, NX) {
                double sm = 0.0, ps = 0.0;
#pragma unroll
                for (int k = 0; k <= MAXORD; ++k)
                    if (k <= order) sm += s.D[k][i];
#pragma unroll
                for (int k = 1; k <= MAXORD; ++k)
                    if (k <= order) ps += s.D[k][i] * bdf_gamma(k);
                s.ypred[i] = sm; s.psi[i] = ps / alpha;
                s.scale[i] = atol + rtol * ::fabs(sm);
            }
            tm.sync();
            const double c = h_abs / alpha;
            int converged = 0;
            while (!converged) {
                if (!lu_valid) {
                    if (!bdf_lu_factor(tm, s, c)) { status = BDF_FAIL_SINGULAR; break; }
                    ++nlu; lu_valid = 1;
                }
                // modified Newton on  y - c f(y) + psi - y_predict = 0  in the form  (I - cJ) dy = c f(y) - psi - d
                GL_BDF_FOR(i, NX) { s.ynew[i] = s.ypred[i]; s.dd[i] = 0.0; }
                tm.sync();
                double dy_norm_old = -1.0, rate = -1.0;
                converged = 0;
                for (n_iter = 0; n_iter < NEWTON_MAXITER; ++n_iter) {
                    tm.eval1(s.ynew, s.fy); ++nfev;
                    double bad = 0.0;
                    GL_BDF_FOR(i, NX) {
                        if (!__builtin_isfinite(s.fy[i])) bad = 1.0;
                        s.dy[i] = c * s.fy[i] - s.psi[i] - s.dd[i];
                    }
                    tm.sync();
                    if (tm.sum(bad) != 0.0) break;
                    tm.lu_solve(s, s.dy);
                    const double dy_norm = bdf_rms(tm, [&](int i) { return s.dy[i]; }, s.scale);
                    if (dy_norm_old >= 0.0) rate = dy_norm / dy_norm_old;
                    if (rate >= 0.0 && (rate >= 1.0 || ::pow(rate, (double)(NEWTON_MAXITER - n_iter)) / (1.0 - rate) * dy_norm > newton_tol)) break;
                    GL_BDF_FOR(i, NX) { s.ynew[i] += s.dy[i]; s.dd[i] += s.dy[i]; }
                    tm.sync();
                    if (dy_norm == 0.0 || (rate >= 0.0 && rate / (1.0 - rate) * dy_norm < newton_tol)) { converged = 1; ++n_iter; break; }
                    dy_norm_old = dy_norm;
                }
                if (!converged) {
                    if (current_jac) break;
                    tm.jac(s.ypred, s.f, true, s.J); nfev += NX + 1; ++njev;
                    lu_valid = 0; current_jac = 1;
                }
            }
            if (status != BDF_OK) break;
            if (!converged) {
                h_abs *= 0.5; bdf_change_D(tm, s, order, 0.5); n_equal_steps = 0; lu_valid = 0;
                continue;
            }
            safety = 0.9 * (2.0 * NEWTON_MAXITER + 1.0) / (2.0 * NEWTON_MAXITER + (double)n_iter);
            GL_BDF_FOR(i, NX) s.scale[i] = atol + rtol * ::fabs(s.ynew[i]);
            tm.sync();
            const double ec = bdf_error_const(order);
            error_norm = bdf_rms(tm, [&](int i) { return ec * s.dd[i]; }, s.scale);
            if (error_norm > 1.0) {
                const double factor = ::fmax(0.2, safety * ::pow(error_norm, -1.0 / (order + 1)));
                h_abs *= factor; bdf_change_D(tm, s, order, factor); n_equal_steps = 0; lu_valid = 0;
            } else {
                step_accepted = 1;
            }
        }
        if (status != BDF_OK) break;
        ++n_equal_steps; ++nsteps;
        t += h_abs;
        current_jac = 0;
        GL_BDF_FOR(i, NX) {
            double dk[MAXORD + 3];
#pragma unroll
            for (int k = 0; k < MAXORD + 3; ++k) dk[k] = s.D[k][i];
            const double ddi = s.dd[i];
#pragma unroll
            for (int k = 0; k <= MAXORD; ++k)
                if (k == order) { dk[k + 2] = ddi - dk[k + 1]; dk[k + 1] = ddi; }
#pragma unroll
            for (int k = MAXORD; k >= 0; --k)
                if (k <= order) dk[k] += dk[k + 1];
#pragma unroll
            for (int k = 0; k < MAXORD + 3; ++k) s.D[k][i] = dk[k];
        }
        tm.sync();
        if (n_equal_steps < order + 1) continue;
        double em = INFINITY, ep = INFINITY;
        if (order > 1) { const double e = bdf_error_const(order - 1); em = bdf_rms(tm, [&](int i) { return e * s.D[order][i]; }, s.scale); }
        if (order < MAXORD) { const double e = bdf_error_const(order + 1); ep = bdf_rms(tm, [&](int i) { return e * s.D[order + 2][i]; }, s.scale); }
        const double fm = (em > 0.0 && __builtin_isfinite(em)) ? ::pow(em, -1.0 / order) : (em == 0.0 ? INFINITY : 0.0);
        const double f0 = error_norm > 0.0 ? ::pow(error_norm, -1.0 / (order + 1)) : INFINITY;
        const double fp = (ep > 0.0 && __builtin_isfinite(ep)) ? ::pow(ep, -1.0 / (order + 2)) : (ep == 0.0 ? INFINITY : 0.0);
        int delta = 0; double best = f0;
        if (fm > best) { best = fm; delta = -1; }
        if (fp > best) { best = fp; delta = 1; }
        order += delta;
        const double factor = ::fmin(10.0, safety * best);
        h_abs *= factor; bdf_change_D(tm, s, order, factor); n_equal_steps = 0; lu_valid = 0;
    }
    if (status == BDF_OK) {
        double bad = 0.0;
        GL_BDF_FOR(i, NX) if (!__builtin_isfinite(y[i])) bad = 1.0;
        if (tm.sum(bad) != 0.0) status = BDF_FAIL_NONFINITE;
    }
    if (stats) {                                             // every lane (the scalars are the team's)
        stats[ST_STEPS] = (int32_t)nsteps; stats[ST_NFEV] = (int32_t)nfev; stats[ST_NJEV] = (int32_t)njev;
        stats[ST_NLU] = (int32_t)nlu; stats[ST_ORDER] = order;
    }
    return status;
}

#undef GL_BDF_FOR

}  // namespace glbdf
