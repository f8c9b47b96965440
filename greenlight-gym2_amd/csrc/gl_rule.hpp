// gl_rule.hpp -- the rule-based controller for ONE row with that row's own constants (include/glgym.h glgym_rule_rows,
// glgym_plan_rollout_rule), for host and device code alike:
//   space_error     what is wrong with a glgym_rule_space (NULL: nothing), checked on the host before anything is launched
//   Space, make_space
//                   the search space by FIELD instead of by component: for each of the 29 constants its base value and, if it is
//                   tuned, which component of theta it is decoded from and between which bounds -- so that a lane indexes nothing
//                   by a run-time field number and its 29 constants stay in registers
//   decode_one, row_cfg
//                   theta -> constants of one row.  In double with products and sums rounded separately, as in gl_scen.hpp:
//                   t = fmin(fmax((double)theta, -1), 1); v = lo + (hi - lo) * (0.5 * (t + 1)).  fmax / fmin return their other
//                   operand when one is a NaN, so a NaN theta reads as -1, i.e. lo.  This is deliberate: the controls of a candidate
//                   go straight into the step kernel, and a NaN control must never reach it.
//   controls        the six controls from the row's constants, state, weather row and clocks: rule_based_kernel's body
//                   (glgym_env.hip; baseline.py:68-227) restated in fp64 with the constants in an array.  The comparisons
//                   lamps_on <= lamps_off, lamps_day_start <= lamps_day_stop and lamps_on == lamps_off are the ROW's: lanes of one
//                   wavefront may take different sides (selects, no branch).  rule_based_kernel itself is left as it is; the two
//                   are held together by tests/test_gpu_plan_rule.py.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "glgym.h"
#include "gl_plan.hpp"

namespace glrule {

constexpr int NF = 29;                           // constants of glgym_rule_cfg, read as double[29] in declaration order
constexpr int NU = 6;
// glgym_rule_cfg in declaration order
enum Field {
    LAMPS_ON, LAMPS_OFF, LAMPS_DAY_START, LAMPS_DAY_STOP, LAMPS_OFF_SUN, LAMP_RAD_SUM_LIMIT, TEMP_SETPOINT_DAY, TEMP_SETPOINT_NIGHT,
    HEAT_CORRECTION, HEAT_DEADZONE, CO2_DAY, VENT_HEAT_PBAND, RH_MAX, MECH_DEHUMID_PBAND, VENT_RH_PBAND, T_VENT_OFF, VENT_COLD_PBAND,
    TH_SCR_SP_DAY, TH_SCR_SP_NIGHT, TH_SCR_PBAND, TH_SCR_DEAD_ZONE, TH_SCR_RH, TH_SCR_RH_PBAND, LAMP_EXTRA_HEAT, BL_SCR_EXTRA_RH, RH_MAX2,
    T_HEAT_BAND, CO2_BAND, USE_BL_SCR
};
static_assert(USE_BL_SCR == NF - 1 && sizeof(glgym_rule_cfg) == NF * sizeof(double), "glgym_rule_cfg is 29 doubles");
constexpr int N_BAND = 7;                        // the proportional bands the rules divide by
constexpr int BAND[N_BAND] = {VENT_HEAT_PBAND, VENT_RH_PBAND, VENT_COLD_PBAND, TH_SCR_PBAND, TH_SCR_RH_PBAND, T_HEAT_BAND, CO2_BAND};

inline bool is_band(int f)
{
    for (int i = 0; i < N_BAND; ++i)
        if (BAND[i] == f) return true;
    return false;
}

// NULL, or the reason a search space is refused
inline const char* space_error(const glgym_rule_space* sp)
{
    if (!sp) return "null search space";
    if (sp->D < 1 || sp->D > NF) return "D outside 1..29";
    bool tuned[NF] = {};
    for (int i = 0; i < sp->D; ++i) {
        const int f = sp->field[i];
        if (f < 0 || f >= NF) return "a field index outside 0..28";
        if (tuned[f]) return "a field index given twice";
        tuned[f] = true;
        const double lo = sp->lo[i], hi = sp->hi[i];
        if (!std::isfinite(lo) || !std::isfinite(hi) || lo > hi) return "lo / hi not finite, or lo > hi";
        if (is_band(f) && lo <= 0.0 && 0.0 <= hi) return "the interval of a tuned proportional band contains 0";
    }
    const double* base = reinterpret_cast<const double*>(&sp->base);
    for (int i = 0; i < N_BAND; ++i)
        if (!tuned[BAND[i]] && base[BAND[i]] == 0) return "a zero proportional band in base";
    return nullptr;
}

// the search space by field.  slot[f] = the component of theta that field f is decoded from, or -1: base[f] it is
struct Space {
    double base[NF], lo[NF], hi[NF];
    int32_t slot[NF];
};

inline Space make_space(const glgym_rule_space& sp)
{
    Space s;
    const double* base = reinterpret_cast<const double*>(&sp.base);
    for (int f = 0; f < NF; ++f) { s.base[f] = base[f]; s.lo[f] = s.hi[f] = 0.0; s.slot[f] = -1; }
    for (int i = 0; i < sp.D; ++i) {
        const int f = sp.field[i];
        s.slot[f] = i; s.lo[f] = sp.lo[i]; s.hi[f] = sp.hi[i];
    }
    return s;
}

GLPLAN_HD double decode_one(float theta, double lo, double hi)
{
#pragma clang fp contract(off)
    const double t = fmin(fmax((double)theta, -1.0), 1.0);       // a NaN theta reads as -1: see the head of this file
    const double half = 0.5 * (t + 1.0);
    const double span = hi - lo;
    const double part = span * half;
    return lo + part;
}

// the 29 constants of row j of the block theta [Ht][J][6]: component i is theta[i / 6][j][i % 6]
GLPLAN_HD void row_cfg(const Space& s, const float* theta, int J, int j, double c[NF])
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int f = 0; f < NF; ++f) {
        const int i = s.slot[f];
        c[f] = i < 0 ? s.base[f] : decode_one(theta[((size_t)(i / NU) * (size_t)J + (size_t)j) * NU + (size_t)(i % NU)], s.lo[f], s.hi[f]);
    }
}

// proportional band: lo + (hi-lo) / (1 + exp(-2/pBand * ln(100) * (v - setPt - pBand/2)))   (baseline.py:226-227)
GLPLAN_HD double pband(double v, double sp, double band, double lo, double hi)
{
    return lo + (hi - lo) * (1.0 / (1.0 + exp(-2.0 / band * 4.605170185988092 * (v - sp - band * 0.5))));
}

GLPLAN_HD void controls(const double c[NF], double iGlob, double tOut, double dli, double isDay, double isDaySmooth, double co2Air,
                        double tAir, double vpAir, double hod, double doy, double u[NU])
{
    const double on = c[LAMPS_ON], off = c[LAMPS_OFF], d0 = c[LAMPS_DAY_START], d1 = c[LAMPS_DAY_STOP];
    const double tod = on <= off ? (double)(on < hod && hod < off) : (double)(on < hod || hod < off);              // :76-77
    const double doy_ok = d0 <= d1 ? (double)(d0 < doy && doy < d1) : (double)(d0 < doy || doy < d1);              // :85-86
    const double below_dli = (double)(dli < c[LAMP_RAD_SUM_LIMIT]);
    const double lamp_no_cons = (double)(iGlob < c[LAMPS_OFF_SUN]) * below_dli * tod * doy_ok;                      // :98
    const double sw_on = fmax(0.0, fmin(1.0, hod - on + 1.0));                                                     // :107
    const double sw_off = fmax(0.0, fmin(1.0, off - hod + 1.0));                                                   // :113
    const double both = on == off ? 0.0 : (on < off ? fmin(sw_on, sw_off) : fmax(sw_on, sw_off));                  // :119-120
    const double smooth_lamp = both * below_dli * doy_ok;                                                          // :128
    const double day_inside = fmax(smooth_lamp, isDay);                                                            // :133
    const double heat_sp = day_inside * c[TEMP_SETPOINT_DAY] + (1.0 - day_inside) * c[TEMP_SETPOINT_NIGHT] +
                           c[HEAT_CORRECTION] * lamp_no_cons;                                                      // :136
    const double heat_max = heat_sp + c[HEAT_DEADZONE];
    const double co2_sp = day_inside * c[CO2_DAY];
    const double co2_ppm = 1e6 * 8.3144598 * (tAir + 273.15) * (1e-6 * co2Air) / (101325.0 * 44.01e-3);            // :145
    const double rh_in = 100.0 * vpAir / (610.78 * exp(17.2694 * tAir / (tAir + 238.3)));                          // :151
    const double vent_heat = pband(tAir, heat_max, c[VENT_HEAT_PBAND], 0, 1);
    const double vent_rh = pband(rh_in, c[RH_MAX] + 0.0 * c[MECH_DEHUMID_PBAND], c[VENT_RH_PBAND], 0, 1);
    const double vent_cold = pband(tAir, heat_sp - c[T_VENT_OFF], c[VENT_COLD_PBAND], 1, 0);
    const double th_sp = isDay * c[TH_SCR_SP_DAY] + (1.0 - isDay) * c[TH_SCR_SP_NIGHT];
    const double th_cold = pband(tOut, th_sp, c[TH_SCR_PBAND], 0, 1);
    const double th_heat = pband(tAir, heat_sp + c[TH_SCR_DEAD_ZONE], -c[TH_SCR_PBAND], 1, 0);
    const double th_rh = fmax(pband(rh_in, c[RH_MAX2] + c[TH_SCR_RH], c[TH_SCR_RH_PBAND], 1, 0), 1.0 - vent_cold);
    const double lamp_on = lamp_no_cons * pband(tAir, heat_max + c[LAMP_EXTRA_HEAT], -0.5, 0, 1) *
                           (isDaySmooth + (1.0 - isDaySmooth)) *
                           fmax(pband(rh_in, c[RH_MAX2] + c[BL_SCR_EXTRA_RH], -0.5, 0, 1), 1.0 - vent_cold);       // :189-191
    u[0] = pband(tAir, heat_sp, c[T_HEAT_BAND], 0, 1);
    u[1] = pband(co2_ppm, co2_sp, c[CO2_BAND], 0, 1);
    u[2] = fmin(th_cold, fmax(th_heat, th_rh));
    u[3] = fmin(vent_cold, fmax(vent_heat, vent_rh));
    u[4] = lamp_on;
    u[5] = c[USE_BL_SCR] * (1.0 - isDaySmooth) * lamp_on;
}

// the row of theta that child / row b reads: b / max(S, 1)
GLPLAN_HD int theta_row(int b, int S) { return S > 1 ? b / S : b; }

}  // namespace glrule
