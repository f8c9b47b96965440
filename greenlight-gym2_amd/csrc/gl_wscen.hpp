// gl_wscen.hpp -- the scalar logic of weather-forecast scenarios (include/glgym.h glgym_plan_weather), for host and device code alike:
//   eps             the innovation of (greenhouse-scenario ps, horizon step h, weather column j): four Philox words, centred, summed
//                   and scaled to unit variance -- bounded, and made of correctly rounded double operations only
//   advance         the lag-1 error process e_h = phi * e_{h-1} + g * eps_h (e_0 = 0: the row being integrated is a measurement)
//   apply           the error on one source value: additive on the temperatures, multiplicative with a floor at 0 on the rest
//   source_row, child_offset
//                   the parent's row a plain child would read at step h, and the w_off that makes a child's unchanged timestep index
//                   its own window
//   column, copy_rest, window_lane
//                   what ONE lane of plan_weather_kernel does: lane (ps, j < 7) runs column j's recurrence over the horizon, lane
//                   (ps, 7) copies the columns the error model leaves alone
// Everything is double with products and sums rounded separately, as in gl_scen.hpp.
#pragma once
#include "gl_scen.hpp"

namespace glwscen {

constexpr int NCOL = 7;                          // iGlob, tOut, vpOut, co2Out, wind, tSky, tSoOut: the columns the right-hand side reads
constexpr int LANES = 8;                         // lanes per (greenhouse, scenario): NCOL recurrences and one copier
constexpr uint32_t KEY_TAG = 0x5753434eu;        // "WSCN": xor-ed into the key's high word, apart from the scenario, CEM and crop-noise streams
constexpr double SQRT3 = 1.7320508075688772;     // sqrt(3) rounded to double: four centred uniforms have variance 4/12
constexpr int MAX_H = 65536;

// the temperatures tOut, tSky, tSoOut take an additive error [K]; iGlob, vpOut, co2Out, wind a relative one and stay >= 0
GLPLAN_HD bool additive(int j) { return j == 1 || j == 5 || j == 6; }

// sqrt(1 - phi^2), the product and the difference rounded separately: computed once on the host, passed to the kernel by value
inline double innov_of(double phi)
{
#pragma clang fp contract(off)
    const double p2 = phi * phi;
    return std::sqrt(1.0 - p2);
}

// counter (ps, lo32(D), hi32(D), 8*h + j), key (lo32(seed), hi32(seed) ^ KEY_TAG); |eps| < 2 sqrt(3)
GLPLAN_HD double eps(uint32_t ps, int h, int j, uint64_t D, uint64_t seed)
{
#pragma clang fp contract(off)
    uint32_t r[4];
    glcem::philox4x32_10(ps, (uint32_t)D, (uint32_t)(D >> 32), 8u * (uint32_t)h + (uint32_t)j, (uint32_t)seed,
                         (uint32_t)(seed >> 32) ^ KEY_TAG, r);
    const double c0 = glscen::centred(r[0]), c1 = glscen::centred(r[1]), c2 = glscen::centred(r[2]), c3 = glscen::centred(r[3]);
    return (((c0 + c1) + c2) + c3) * SQRT3;
}

// e_h from e_{h-1}, h >= 1: two products and one sum
GLPLAN_HD double advance(double e, double phi, double g, double eps_h)
{
#pragma clang fp contract(off)
    const double t0 = phi * e, t1 = g * eps_h;
    return t0 + t1;
}

template <class T>
GLPLAN_HD T apply(int j, T w, double e)
{
#pragma clang fp contract(off)
    if (additive(j)) return (T)((double)w + e);
    const double t = e * (double)w;
    const double v0 = (double)w + t;
    return (T)(v0 < 0.0 ? 0.0 : v0);
}

// clamp(w_off + timestep + h, 0, rows - 1): the step kernels' row, with the sum taken in 64 bits
GLPLAN_HD int source_row(int32_t w_off, int32_t timestep, int h, int rows)
{
    const int64_t r = (int64_t)w_off + (int64_t)timestep + (int64_t)h;
    return r < 0 ? 0 : (r > (int64_t)rows - 1 ? rows - 1 : (int)r);
}

// w_off of the children of (greenhouse, scenario) ps: w_off + timestep + h = ps*H + h with the parent's timestep (may be negative)
GLPLAN_HD int32_t child_offset(uint32_t ps, int H, int32_t timestep) { return (int32_t)((int64_t)ps * H - (int64_t)timestep); }

// column j < NCOL of window rows ps*H .. ps*H + H-1.  g = innov * sigma_j.
template <class T>
GLPLAN_HD void column(uint32_t ps, int j, int H, int nd, const T* weather, int rows, int32_t w_off, int32_t timestep, double phi, double g,
                      uint64_t D, uint64_t seed, T* window)
{
    double e = 0.0;
    T* out = window + (size_t)ps * (size_t)H * (size_t)nd + j;
    for (int h = 0; h < H; ++h) {
        if (h > 0) e = advance(e, phi, g, eps(ps, h, j, D, seed));
        out[(size_t)h * nd] = apply<T>(j, weather[(size_t)source_row(w_off, timestep, h, rows) * nd + j], e);
    }
}

// columns NCOL .. nd-1 (dli, the day flags, the measured-pipe columns), unchanged
template <class T>
GLPLAN_HD void copy_rest(uint32_t ps, int H, int nd, const T* weather, int rows, int32_t w_off, int32_t timestep, T* window)
{
    T* out = window + (size_t)ps * (size_t)H * (size_t)nd;
    for (int h = 0; h < H; ++h) {
        const T* in = weather + (size_t)source_row(w_off, timestep, h, rows) * nd;
        for (int j = NCOL; j < nd; ++j) out[(size_t)h * nd + j] = in[j];
    }
}

// lane jj of (greenhouse, scenario) ps = p*S + s
template <class T>
GLPLAN_HD void window_lane(uint32_t ps, int jj, int S, int H, int nd, const T* weather, int rows, const int32_t* w_off_parent,
                           const int32_t* timestep_parent, const double* sigma, double phi, double innov, uint64_t D, uint64_t seed, T* window)
{
#pragma clang fp contract(off)
    const uint32_t p = ps / (uint32_t)S;
    const int32_t w_off = w_off_parent[p], ts = timestep_parent[p];
    if (jj < NCOL) {
        const double g = innov * sigma[jj];
        column<T>(ps, jj, H, nd, weather, rows, w_off, ts, phi, g, D, seed, window);
    } else {
        copy_rest<T>(ps, H, nd, weather, rows, w_off, ts, window);
    }
}

}  // namespace glwscen
