// TESTS ONLY.  Host (g++) twin of tests/bdfwave/bdfwave.hip: the same entry points over host arrays, gl_bdf.hpp on a team of one lane
// with the serial solve (like tests/bdfhost/bdfhost.cpp), the same problem bodies (bdfwave_common.hpp).  The two reductions have no
// team of one to run on: they are restated here over 64 lane values in the order of the wavefront's xor butterfly.
// The product library (libglgym.so) never links or loads this file.
#include <cstring>

#include "bdfwave_common.hpp"

using namespace glm;

namespace {

template <class Rhs> struct HostTeam {
    static constexpr int width = 1;
    Rhs f;
    int lane() const { return 0; }
    double sum(double v) const { return v; }
    void argmax(double&, int&) const {}
    void sync() const {}
    void lu_solve(glbdf::BdfScratch& sh, double* b) const { glbdf::bdf_lu_solve_serial(sh, b); }
    void eval1(const double* x, double* fx) const { f(x, fx); }
    void jac(const double* x, double* f0, bool need_f0, double* J) const
    {
        if (need_f0) eval1(x, f0);
        double xp[NX], fp[NX];
        std::memcpy(xp, x, sizeof xp);
        for (int j = 0; j < NX; ++j) {
            const double dxj = 1.4901161193847656e-8 * ::fmax(::fabs(x[j]), 1.0);
            xp[j] = x[j] + dxj;
            eval1(xp, fp);
            for (int i = 0; i < NX; ++i) J[i * NX + j] = (fp[i] - f0[i]) / dxj;
            xp[j] = x[j];
        }
    }
};

struct HostModelRhs {
    const ModelConst<double>& m;
    const CropConst<double>& cr;
    const StepCoef<double>& s;
    void operator()(const double* xs, double* k) const { rhs<double, true, false>(xs, s, m, cr, k); }
};

constexpr int LANES = 64;

}  // namespace

extern "C" {

int bdfwave_reduce(const double* v, const int* idx, const double* rv, const double* rs, int n, double* sum_out, double* amax_v,
                   int* amax_i, double* rms_out)
{
    static thread_local glbdf::BdfScratch sh;
    const HostTeam<bdfwave::NoRhs> tm{{}};
    for (int b = 0; b < n; ++b) {
        double s[LANES], a[LANES], t[LANES];
        int ai[LANES], ti[LANES];
        for (int l = 0; l < LANES; ++l) { s[l] = a[l] = v[b * LANES + l]; ai[l] = idx[b * LANES + l]; }
        for (int o = 32; o > 0; o >>= 1) {
            for (int l = 0; l < LANES; ++l) t[l] = s[l] + s[l ^ o];
            std::memcpy(s, t, sizeof s);
            for (int l = 0; l < LANES; ++l) {
                const double ov = a[l ^ o];
                const int oi = ai[l ^ o];
                const bool take = ov > a[l] || (ov == a[l] && oi < ai[l]);
                t[l] = take ? ov : a[l]; ti[l] = take ? oi : ai[l];
            }
            std::memcpy(a, t, sizeof a); std::memcpy(ai, ti, sizeof ai);
        }
        const double r = bdfwave::rms_problem(tm, sh, rv + b * NX, rs + b * NX);
        for (int l = 0; l < LANES; ++l) {
            sum_out[b * LANES + l] = s[l]; amax_v[b * LANES + l] = a[l]; amax_i[b * LANES + l] = ai[l]; rms_out[b * LANES + l] = r;
        }
    }
    return 0;
}

int bdfwave_lu(const double* J, const double* c, const double* b, int n, int* ok, double* LU, int* piv, int* perm, double* x)
{
    static thread_local glbdf::BdfScratch sh;
    const HostTeam<bdfwave::NoRhs> tm{{}};
    for (int k = 0; k < n; ++k)
        bdfwave::lu_problem(tm, sh, J + k * NX * NX, c[k], b + k * NX, ok + k, LU + k * NX * NX, piv + k * NX, perm + k * NX, x + k * NX);
    return 0;
}

int bdfwave_change_D(const double* D, const int* order, const double* factor, int n, double* Dout)
{
    static thread_local glbdf::BdfScratch sh;
    const HostTeam<bdfwave::NoRhs> tm{{}};
    const int nd = (glbdf::MAXORD + 3) * NX;
    for (int k = 0; k < n; ++k) bdfwave::change_D_problem(tm, sh, D + k * nd, order[k], factor[k], Dout + k * nd);
    return 0;
}

int bdfwave_step(const int* kind, const double* y0, const double* A, const double* g, const double* mu, const double* dt,
                 const double* rtol, const double* atol, const int* max_steps, int n, double* y, int32_t* stats, int* rc)
{
    static thread_local glbdf::BdfScratch sh;
    for (int k = 0; k < n; ++k) {
        const HostTeam<bdfwave::SynthRhs> tm{{kind[k], A + k * NX * NX, g + k * NX, mu[k]}};
        bdfwave::step_problem(tm, sh, y0 + k * NX, dt[k], rtol[k], atol[k], max_steps[k], y + k * NX, stats + k * glbdf::NSTAT, rc + k);
    }
    return 0;
}

int bdfwave_model_jac(const double* x, const double* u, const double* d, const double* p, int need_f0, int n, double* f, double* f0,
                      double* J)
{
    static thread_local glbdf::BdfScratch sh;
    for (int k = 0; k < n; ++k) {
        ModelConst<double> m;
        std::memset(&m, 0, sizeof m);
        make_model_const<double>(p + k * NP, m);
        double uu[NU], dd[7];
        for (int i = 0; i < NU; ++i) uu[i] = u[k * NU + i];
        for (int i = 0; i < 7; ++i) dd[i] = d[k * 7 + i];
        StepCoef<double> s;
        precompute(uu, dd, m, m.crop, s);
        const HostTeam<HostModelRhs> tm{{m, m.crop, s}};
        bdfwave::jac_problem(tm, sh, x + k * NX, need_f0, f + k * NX, f0 + k * NX, J + k * NX * NX);
    }
    return 0;
}

}  // extern "C"
