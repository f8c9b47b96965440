// Host (g++) instantiation of the product's csrc/gl_rule.hpp -- tests only (tests/test_plan_rule_host.py).  A lane of rule_rows_kernel
// is one call of row_cfg + controls on row b with the constants of theta row b / max(S, 1).
// With -DRULEHOST_MAIN the file is a stand-alone program (the one the sanitizers run on): it drives the entries below over small and
// awkward shapes with exactly sized heap buffers and prints "rulehost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "glgym.h"
#include "gl_rule.hpp"

extern "C" {

int rulehost_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(glgym_rule_space);
        case 1: return (int)sizeof(glgym_rule_rows_args);
        case 2: return (int)sizeof(glgym_plan_rollout_rule_args);
    }
    return -1;
}

// 0: the space is accepted; 1: refused, the reason copied to msg (at most n bytes)
int rulehost_space_error(const glgym_rule_space* sp, char* msg, int n)
{
    const char* why = glrule::space_error(sp);
    if (why && msg && n > 0) { std::strncpy(msg, why, (size_t)n - 1); msg[n - 1] = 0; }
    return why ? 1 : 0;
}

// the 29 constants of rows 0 .. B-1: cfg [B][29]
void rulehost_decode(const glgym_rule_space* sp, const float* theta, int J, int S, int B, double* cfg)
{
    const glrule::Space s = glrule::make_space(*sp);
    for (int b = 0; b < B; ++b) glrule::row_cfg(s, theta, J, glrule::theta_row(b, S), cfg + (size_t)b * glrule::NF);
}

// glgym_rule_rows on the host with explicit clocks: X [B][28], D [B][>= 10 columns, row stride nd], U [B][6] out
void rulehost_rows(const glgym_rule_space* sp, const float* theta, int J, int S, int B, const double* X, const double* D, int nd,
                   const double* hour, const double* doy, double* U)
{
    const glrule::Space s = glrule::make_space(*sp);
    for (int b = 0; b < B; ++b) {
        double c[glrule::NF];
        glrule::row_cfg(s, theta, J, glrule::theta_row(b, S), c);
        const double* x = X + (size_t)b * 28;
        const double* w = D + (size_t)b * nd;
        glrule::controls(c, w[0], w[1], w[7], w[8], w[9], x[0], x[2], x[15], hour[b], doy[b], U + (size_t)b * glrule::NU);
    }
}

}  // extern "C"

#ifdef RULEHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

glgym_rule_space space_of(int D)
{
    glgym_rule_space sp;
    std::memset(&sp, 0, sizeof sp);
    double* base = reinterpret_cast<double*>(&sp.base);
    for (int f = 0; f < glrule::NF; ++f) base[f] = 1.0 + f;
    sp.D = D;
    for (int i = 0; i < D; ++i) { sp.field[i] = (i * 7) % glrule::NF; sp.lo[i] = 2.0 + i; sp.hi[i] = 5.0 + 2 * i; }   // 7 and 29 coprime: distinct
    return sp;
}

void drive(int D, int J, int S)
{
    const int Ht = (D + 5) / 6, B = J * (S > 1 ? S : 1);
    glgym_rule_space sp = space_of(D);
    EXPECT(rulehost_space_error(&sp, nullptr, 0) == 0);
    std::vector<float> theta((size_t)Ht * J * 6);
    for (size_t i = 0; i < theta.size(); ++i) theta[i] = (float)((int)(i % 9) - 4) * 0.4f;
    theta[0] = std::numeric_limits<float>::quiet_NaN();
    std::vector<double> cfg((size_t)B * glrule::NF), X((size_t)B * 28), Dw((size_t)B * 10), hour(B), doy(B), U((size_t)B * 6);
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < 28; ++i) X[(size_t)b * 28 + i] = 10.0 + i + 0.1 * b;
        X[(size_t)b * 28] = 900.0; X[(size_t)b * 28 + 2] = 18.0 + 0.2 * b; X[(size_t)b * 28 + 15] = 1500.0;
        for (int i = 0; i < 10; ++i) Dw[(size_t)b * 10 + i] = 0.5 * i;
        hour[b] = std::fmod(0.75 * b, 24.0); doy[b] = 10.0 + b;
    }
    rulehost_decode(&sp, theta.data(), J, S, B, cfg.data());
    rulehost_rows(&sp, theta.data(), J, S, B, X.data(), Dw.data(), 10, hour.data(), doy.data(), U.data());
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < D; ++i) {
            const double v = cfg[(size_t)b * glrule::NF + sp.field[i]];
            EXPECT(v >= sp.lo[i] && v <= sp.hi[i]);
        }
        for (int j = 0; j < 6; ++j) EXPECT(std::isfinite(U[(size_t)b * 6 + j]));
    }
    EXPECT(cfg[sp.field[0]] == sp.lo[0]);                        // the NaN component reads as lo
}

}  // namespace

int main()
{
    EXPECT(rulehost_sizeof(0) > 0 && rulehost_sizeof(1) > 0 && rulehost_sizeof(2) > 0);
    drive(1, 1, 0);
    drive(6, 3, 1);
    drive(7, 5, 3);
    drive(29, 2, 0);
    glgym_rule_space bad = space_of(3);
    char msg[64];
    bad.field[2] = bad.field[0];
    EXPECT(rulehost_space_error(&bad, msg, (int)sizeof msg) == 1 && msg[0]);
    std::printf(failures ? "rulehost FAILED (%d)\n" : "rulehost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
