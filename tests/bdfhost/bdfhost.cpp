// TESTS ONLY.  Host (g++) instantiation of greenlight-gym2_amd/csrc/gl_bdf.hpp with a team of width 1, over the host build of
// gl_model.hpp's right-hand side: the integrator's own arithmetic and decisions, checked on a machine without a GPU.  The product
// library (libglgym.so) never links or loads this file.
#include <cstring>

#include "gl_bdf.hpp"

using namespace glm;

namespace {

struct HostTeam {
    static constexpr int width = 1;
    const ModelConst<double>& m;
    const CropConst<double>& cr;
    const StepCoef<double>& s;
    int lane() const { return 0; }
    double sum(double v) const { return v; }
    void argmax(double&, int&) const {}
    void sync() const {}
    void lu_solve(glbdf::BdfScratch& sh, double* b) const { glbdf::bdf_lu_solve_serial(sh, b); }
    void eval1(const double* x, double* f) const { rhs<double, true, false>(x, s, m, cr, f); }
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

}  // namespace

// x0[28] u[6] d[>=7] p[208] (p[128..161] is the row's crop block, built per row like the device kernel) -> x1[28], stats[5].
// Returns 0 or the failure code of gl_bdf.hpp (x1 is then the state where the integration stopped).
extern "C" int bdfhost_step(const double* x0, const double* u, const double* d, const double* p, double dt, double rtol, double atol,
                            int max_steps, double* x1, int* stats)
{
    ModelConst<double> m;
    std::memset(&m, 0, sizeof m);
    make_model_const<double>(p, m);
    CropConst<double> cr;
    make_crop_const<double, double>(p + CROP0, p[39], p[162], cr);
    double uu[NU], dd[7];
    for (int i = 0; i < NU; ++i) uu[i] = u[i];
    for (int i = 0; i < 7; ++i) dd[i] = d[i];
    StepCoef<double> s;
    precompute(uu, dd, m, cr, s);
    static thread_local glbdf::BdfScratch sh;
    std::memcpy(sh.D[0], x0, NX * sizeof(double));
    HostTeam tm{m, cr, s};
    int32_t st[glbdf::NSTAT];
    const int rc = glbdf::bdf_step(tm, sh, dt, rtol, atol, max_steps, st);
    std::memcpy(x1, sh.D[0], NX * sizeof(double));
    for (int i = 0; i < glbdf::NSTAT; ++i) stats[i] = st[i];
    return rc;
}
