// Host (g++) instantiation of the product's csrc/gl_wscen.hpp -- tests only (tests/test_plan_wscen_host.py).  A lane of
// plan_weather_kernel is one call of window_lane, a lane of plan_weather_offsets_kernel one call of split_child + child_offset; the
// grids are loops over the lanes in index order.
// With -DWSCENHOST_MAIN the file is a stand-alone program (the one the sanitizers run on): it drives the entries below over small and
// awkward shapes with exactly sized heap buffers and prints "wscenhost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "glgym.h"
#include "gl_wscen.hpp"

namespace {

template <class T>
void window(int P, int K, int S, int H, int nd, const T* weather, int rows, const int32_t* w_off, const int32_t* ts, const double* sigma,
            double phi, uint64_t seed, uint64_t D, T* out, int32_t* w_off_child)
{
    const double innov = glwscen::innov_of(phi);
    const int64_t n_lanes = (int64_t)P * S * glwscen::LANES;
    for (int64_t t = 0; t < n_lanes; ++t) {
        const uint32_t ps = (uint32_t)(t / glwscen::LANES);
        glwscen::window_lane<T>(ps, (int)(t - (int64_t)ps * glwscen::LANES), S, H, nd, weather, rows, w_off, ts, sigma, phi, innov, D, seed, out);
    }
    if (!w_off_child) return;
    for (int c = 0; c < P * K * S; ++c) {
        uint32_t ps;
        int cand;
        glscen::split_child(c, K, S, &ps, &cand);
        w_off_child[c] = glwscen::child_offset(ps, H, ts[cand / K]);
    }
}

}  // namespace

extern "C" {

int wscenhost_sizeof(void) { return (int)sizeof(glgym_plan_weather_args); }

// glgym_plan_weather on the host; D = draw_index + *draw_base.  f64 != 0: the tables are double, else float.
void wscenhost_window(int f64, int P, int K, int S, int H, int nd, const void* weather, int rows, const int32_t* w_off, const int32_t* ts,
                      const double* sigma, double phi, uint64_t seed, uint64_t D, void* out, int32_t* w_off_child)
{
    if (f64) window<double>(P, K, S, H, nd, (const double*)weather, rows, w_off, ts, sigma, phi, seed, D, (double*)out, w_off_child);
    else window<float>(P, K, S, H, nd, (const float*)weather, rows, w_off, ts, sigma, phi, seed, D, (float*)out, w_off_child);
}

// the error process of stream (ps, j) with g = sqrt(1 - phi^2) * sigma: e[0 .. H-1]
void wscenhost_error(uint32_t ps, int j, int H, double sigma, double phi, uint64_t seed, uint64_t D, double* e)
{
    const double g = glwscen::innov_of(phi) * sigma;
    double v = 0.0;
    for (int h = 0; h < H; ++h) {
        if (h > 0) v = glwscen::advance(v, phi, g, glwscen::eps(ps, h, j, D, seed));
        e[h] = v;
    }
}

}  // extern "C"

#ifdef WSCENHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

template <class T>
void drive(int P, int K, int S, int H, int nd, int rows, double phi)
{
    std::vector<T> weather((size_t)rows * nd), out((size_t)P * S * H * nd, (T)-7);
    for (int r = 0; r < rows; ++r)
        for (int j = 0; j < nd; ++j) weather[(size_t)r * nd + j] = (T)(j == 0 ? (r % 3 ? 100.0 + r : 0.0) : 1.0 + j + 0.25 * r);
    std::vector<int32_t> w_off(P), ts(P), child((size_t)P * K * S, -7);
    for (int p = 0; p < P; ++p) { w_off[p] = 2 * p; ts[p] = p == P - 1 ? rows - 2 : p; }      // the last parent runs past the table's end
    const double sigma[7] = {0.2, 1.5, 0.1, 0.0, 0.3, 2.0, 0.5};
    wscenhost_window(sizeof(T) == 8, P, K, S, H, nd, weather.data(), rows, w_off.data(), ts.data(), sigma, phi, 0x1234567800000009ull,
                     (3ull << 32) | 5u, out.data(), child.data());
    for (int ps = 0; ps < P * S; ++ps) {
        const int p = ps / S;
        for (int h = 0; h < H; ++h) {
            const int row = glwscen::source_row(w_off[p], ts[p], h, rows);
            EXPECT(row >= 0 && row < rows);
            const T* got = out.data() + ((size_t)ps * H + h) * nd;
            const T* src = weather.data() + (size_t)row * nd;
            for (int j = 0; j < nd; ++j) {
                if (h == 0 || j == 3 || j >= 7) EXPECT(got[j] == src[j]);
                if (j < 7 && !glwscen::additive(j)) EXPECT(got[j] >= 0 && (src[j] != 0 || got[j] == 0));
                EXPECT(std::isfinite((double)got[j]));
            }
        }
    }
    for (int c = 0; c < P * K * S; ++c) {
        const int p = c / (K * S), s = c % S;
        EXPECT((int64_t)child[c] + ts[p] == (int64_t)(p * S + s) * H);
    }
    wscenhost_window(sizeof(T) == 8, P, K, S, H, nd, weather.data(), rows, w_off.data(), ts.data(), sigma, phi, 1, 0, out.data(), nullptr);
}

}  // namespace

int main()
{
    EXPECT(wscenhost_sizeof() > 0);
    drive<float>(2, 3, 5, 3, 10, 9, 0.7);
    drive<double>(3, 2, 4, 7, 14, 12, 0.0);
    drive<float>(1, 1, 1, 1, 10, 1, 0.7);
    drive<double>(1, 2, 256, 2, 10, 5, 0.9);
    std::vector<double> e(41);
    wscenhost_error(3, 6, 41, 1.0, 0.8, 2026, 0, e.data());
    EXPECT(e[0] == 0.0 && std::fabs(e[40]) < 3.47 * 5.0);
    std::printf(failures ? "wscenhost FAILED (%d)\n" : "wscenhost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
