// glgym_env.hip -- the env layer around the integrator: its kernels and their C entry points (include/glgym.h).
//   obs_kernel         row-major observation assembly incl. the weather-forecast gather (glgym_obs).      [HBM-write bound]
//   reset_kernel       masked init_state() with the episode start draw (glgym_reset).
//   crop_noise_kernel  Philox4x32-10 parameter noise (glgym_crop_noise).
//   rule_based_kernel  the rule-based controller (glgym_rule_based).
// Also glgym_set_obs_modules / glgym_obs_dim.  The device functions shared with the step kernels' epilogues (glgym.hip) are
// gl_envlayer.hpp's; glgym_step_obs / glgym_step_obs_reset (glgym.hip) reach glgym_obs and glgym_reset through the C ABI.
// Nothing in here instantiates an integrating kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>

#include "glgym_internal.h"
#include "gl_envlayer.hpp"

using namespace glm;
using namespace glenv;

namespace {

// ---------------------------------------------------------------------------------------------------
// observations: [B][23 + 5*Np] f32 row-major (observations.py:59-182).  One wavefront per env row so the
// 1 KB row is written with consecutive lanes on consecutive addresses.
// ---------------------------------------------------------------------------------------------------
template <class T> struct ObsArgsT {
    int B, ld;
    const T* x; const T* u; const T* weather; int weather_rows;
    const int* w_off; const int* timestep; const float* start_day;
    int Np; float* obs; double doy_inc, hod_inc;     // (dt/86400) mod 365 [days], dt/3600 [h] per env-step
    const unsigned char* mask; float* term_obs;
    int nd;                                          // weather row stride
    int moff[6], dim;                                // first column of each observation module (-1 = absent), row width
};

// OBS_ROWS (16) consecutive env rows = one contiguous, 32-byte aligned span of the row-major output.  The span is
// assembled in LDS and streamed out with 16-byte stores, lane t writing float4 t, t+256, ... (fully coalesced).
// The kernel is latency-, not bandwidth-bound (a block's chain is: scalar loads of the rows' clocks -> gathers -> LDS ->
// barrier -> stores), so everything is arranged to keep many independent loads in flight per lane: the 16 window bases
// are loaded up front, the 23 state / current-weather / clock features are straight-line code (pointer selects instead
// of a branch per feature: 3 loads in flight), and each lane gathers one forecast element for all 16 rows at once from
// the L2-resident weather table.  Measured at B = 65 536, Np = 48: 44 us (first LDS version) -> 33 (independent gathers)
// -> 26 (branch-free features) -> 24 us (16 rows per block) = 2.9 TB/s written; a plain fill of the buffer takes 11.6 us.
// Masked mode (auto-reset) copies only the finished rows, after saving their previous content as SB3's
// terminal_observation.
template <class T> __global__ __launch_bounds__(256) void obs_kernel(ObsArgsT<T> a)
{
    constexpr int ROWS = OBS_ROWS, NCORE = OBS_NCORE;
    extern __shared__ float4 span4[];               // ROWS * dim floats (dynamic: 8.4 KB at Np = 48), 16-byte aligned
    float* span = reinterpret_cast<float*>(span4);
    const int tid = threadIdx.x;
    const int dim = a.dim;
    for (int rb = blockIdx.x * ROWS; rb < a.B; rb += gridDim.x * ROWS) {
        const int nrows = min(ROWS, a.B - rb);
        if (a.mask) {                                 // masked mode: skip strips without a finished env
            int any = 0;
            for (int r = 0; r < nrows; ++r) any |= a.mask[rb + r];
            if (!any) continue;                       // block-uniform
        }
        // first weather row of each env's window (the row / "timestep" the reference shows is the pre-increment one):
        // block-uniform addresses -> scalar loads, all eight issued before anything depends on them
        int base_r[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int b = rb + (r < nrows ? r : 0);
            const int ts = a.timestep[b];
            base_r[r] = a.w_off[b] + (ts > 0 ? ts - 1 : 0);
        }
        for (int e = tid; e < ROWS * NCORE; e += 256) {
            // straight-line code for all 23 features: two pointer selects, three loads in flight, arithmetic selects --
            // a branch per feature would serialise one memory round trip per branch inside the wave
            const int r = e / NCORE, j = e - r * NCORE;
            const int b = rb + (r < nrows ? r : 0);
            const int ts = a.timestep[b];
            int base = 0;
#pragma unroll
            for (int rr = 0; rr < ROWS; ++rr) base = (rr == r) ? base_r[rr] : base;
            base = base >= a.weather_rows ? a.weather_rows - 1 : (base < 0 ? 0 : base);
            const T* wrow = a.weather + (size_t)base * a.nd;
            // (the features and their inputs: obs_core_feature)
            const int xi = j == 0 ? 0 : j == 1 ? 2 : j == 2 ? 15 : j == 3 ? 9 : j == 4 ? 21 : j == 5 ? 25 : 26;
            const T* p1 = j < 7 ? a.x + (size_t)xi * a.ld + b
                                : (j < 13 ? a.u + (size_t)(j - 7) * a.ld + b : wrow + (j < 18 ? j - 13 : 0));
            const T* p2 = j < 13 ? a.x + (size_t)2 * a.ld + b : wrow + 1;        // tAir or tOut
            const float prim = (float)*p1, aux = (float)*p2, sday = a.start_day[b];
            const float v = obs_core_feature(j, prim, aux, sday, ts, a.doy_inc, a.hod_inc);
            // column of feature j in the configured module order (TomatoEnv._get_obs concatenates the modules in
            // the order of the yml list, tomato_env.py:193-198)
            const int mo = j < 4 ? a.moff[0] : j < 7 ? a.moff[1] : j < 13 ? a.moff[2] : j < 18 ? a.moff[3] : a.moff[4];
            const int jl = j < 4 ? j : j < 7 ? j - 4 : j < 13 ? j - 7 : j < 18 ? j - 13 : j - 18;
            if (r < nrows && mo >= 0) span[r * dim + mo + jl] = v;
        }
        // raw forecast rows, no unit conversion (:175-182): element q of the block = weather[base+1 + q/5][q%5]
        const int nf = a.moff[5] >= 0 ? 5 * a.Np : 0;
        for (int q = tid; q < nf; q += 256) {
            const int i = q / 5, c = q - i * 5;              // division by a constant: mul + shift
            float v[ROWS];
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {                 // eight independent gathers in flight per lane
                int row = base_r[r] + 1 + i;
                row = row >= a.weather_rows ? a.weather_rows - 1 : (row < 0 ? 0 : row);
                v[r] = (float)a.weather[(size_t)row * a.nd + c];
            }
#pragma unroll
            for (int r = 0; r < ROWS; ++r)
                if (r < nrows) span[r * dim + a.moff[5] + q] = v[r];
        }
        __syncthreads();
        float* out = a.obs + (size_t)rb * dim;
        if (!a.mask && nrows == ROWS) {                      // full span: 16-byte stores (rb*dim*4 is a multiple of 32)
            const int n4 = (ROWS * dim) >> 2;                // ROWS multiple of 8 -> exact
            float4* out4 = reinterpret_cast<float4*>(out);
            typedef float v4f __attribute__((ext_vector_type(4)));
            const v4f* src4 = reinterpret_cast<const v4f*>(span4);
            v4f* dst4 = reinterpret_cast<v4f*>(out4);
            for (int e = tid; e < n4; e += 256) __builtin_nontemporal_store(src4[e], &dst4[e]);      // 69 MB per call, read by nobody on the device before the next step kernel has run
        } else {
            for (int r = 0; r < nrows; ++r) {
                if (a.mask && !a.mask[rb + r]) continue;
                for (int jj = tid; jj < dim; jj += 256) {
                    const size_t e = (size_t)r * dim + jj;
                    if (a.mask && a.term_obs) a.term_obs[(size_t)rb * dim + e] = out[e];     // SB3 terminal_observation
                    out[e] = span[e];
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------
// rule-based controller (baseline.py:68-227), one thread per env, fp64 throughout
// ---------------------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void rule_based_kernel(glgym_rule_cfg c, int B, int ld, const T* __restrict__ x,
                                                         const T* __restrict__ weather, int weather_rows,
                                                         const int* __restrict__ w_off, const int* __restrict__ timestep,
                                                         const float* __restrict__ start_day, const double* hour,
                                                         const double* doy_in, double doy_inc, double hod_inc,
                                                         T* __restrict__ control, int nd)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int ts = timestep[b];
    int row = w_off[b] + ts;
    row = row >= weather_rows ? weather_rows - 1 : (row < 0 ? 0 : row);
    const T* w = weather + (size_t)row * nd;
    const double iGlob = (double)w[0], tOut = (double)w[1], dli = (double)w[7], isDay = (double)w[8],
                 isDaySmooth = (double)w[9];
    const double co2Air = (double)x[b], tAir = (double)x[(size_t)2 * ld + b], vpAir = (double)x[(size_t)15 * ld + b];
    const double hod = hour ? hour[b] : fmod((double)ts * hod_inc, 24.0);
    const double doy = doy_in ? doy_in[b] : (double)start_day[b] + (double)ts * doy_inc;
    // proportional band: lo + (hi-lo) / (1 + exp(-2/pBand * ln(100) * (v - setPt - pBand/2)))   (:226-227)
    auto pband = [](double v, double sp, double band, double lo, double hi) {
        return lo + (hi - lo) * (1.0 / (1.0 + exp(-2.0 / band * 4.605170185988092 * (v - sp - band * 0.5))));
    };
    const double tod = c.lamps_on <= c.lamps_off ? (double)(c.lamps_on < hod && hod < c.lamps_off)
                                                 : (double)(c.lamps_on < hod || hod < c.lamps_off);              // :76-77
    const double doy_ok = c.lamps_day_start <= c.lamps_day_stop
                              ? (double)(c.lamps_day_start < doy && doy < c.lamps_day_stop)
                              : (double)(c.lamps_day_start < doy || doy < c.lamps_day_stop);                   // :85-86
    const double below_dli = (double)(dli < c.lamp_rad_sum_limit);
    const double lamp_no_cons = (double)(iGlob < c.lamps_off_sun) * below_dli * tod * doy_ok;                   // :98
    const double sw_on = fmax(0.0, fmin(1.0, hod - c.lamps_on + 1.0));                                          // :107
    const double sw_off = fmax(0.0, fmin(1.0, c.lamps_off - hod + 1.0));                                        // :113
    const double both = c.lamps_on == c.lamps_off ? 0.0
                        : (c.lamps_on < c.lamps_off ? fmin(sw_on, sw_off) : fmax(sw_on, sw_off));               // :119-120
    const double smooth_lamp = both * below_dli * doy_ok;                                                       // :128
    const double day_inside = fmax(smooth_lamp, isDay);                                                         // :133
    const double heat_sp = day_inside * c.temp_setpoint_day + (1.0 - day_inside) * c.temp_setpoint_night +
                           c.heat_correction * lamp_no_cons;                                                    // :136
    const double heat_max = heat_sp + c.heat_deadzone;
    const double co2_sp = day_inside * c.co2_day;
    const double co2_ppm = 1e6 * 8.3144598 * (tAir + 273.15) * (1e-6 * co2Air) / (101325.0 * 44.01e-3);         // :145
    const double rh_in = 100.0 * vpAir / (610.78 * exp(17.2694 * tAir / (tAir + 238.3)));                       // :151
    const double vent_heat = pband(tAir, heat_max, c.vent_heat_Pband, 0, 1);
    const double vent_rh = pband(rh_in, c.rh_max + 0.0 * c.mech_dehumid_Pband, c.vent_rh_Pband, 0, 1);
    const double vent_cold = pband(tAir, heat_sp - c.t_vent_off, c.vent_cold_Pband, 1, 0);
    const double th_sp = isDay * c.thScrSpDay + (1.0 - isDay) * c.thScrSpNight;
    const double th_cold = pband(tOut, th_sp, c.thScrPband, 0, 1);
    const double th_heat = pband(tAir, heat_sp + c.thScrDeadZone, -c.thScrPband, 1, 0);
    const double th_rh = fmax(pband(rh_in, c.rhMax + c.thScrRh, c.thScrRhPband, 1, 0), 1.0 - vent_cold);
    const double lamp_on = lamp_no_cons * pband(tAir, heat_max + c.lampExtraHeat, -0.5, 0, 1) *
                           (isDaySmooth + (1.0 - isDaySmooth)) *
                           fmax(pband(rh_in, c.rhMax + c.blScrExtraRh, -0.5, 0, 1), 1.0 - vent_cold);           // :189-191
    control[b] = (T)pband(tAir, heat_sp, c.tHeatBand, 0, 1);
    control[(size_t)1 * ld + b] = (T)pband(co2_ppm, co2_sp, c.co2Band, 0, 1);
    control[(size_t)2 * ld + b] = (T)fmin(th_cold, fmax(th_heat, th_rh));
    control[(size_t)3 * ld + b] = (T)fmin(vent_cold, fmax(vent_heat, vent_rh));
    control[(size_t)4 * ld + b] = (T)lamp_on;
    control[(size_t)5 * ld + b] = (T)(c.useBlScr * (1.0 - isDaySmooth) * lamp_on);
}

// ---------------------------------------------------------------------------------------------------
// masked reset: init_state (utils.py:13-46)
// ---------------------------------------------------------------------------------------------------
template <class T>
__global__ void reset_kernel(int B, int ld, const unsigned char* mask, T* x, T* u, int* timestep, const T* weather,
                             int weather_rows, int* w_off, const int* start_rows, const float* start_days, int n_starts,
                             float* start_day, int* episode, unsigned long long seed, int nd)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || (mask && !mask[b])) return;
    reset_env<T>(b, ld, x, u, timestep, weather, weather_rows, w_off, start_rows, start_days, n_starts, start_day, episode, seed, nd);
}

// ---------------------------------------------------------------------------------------------------
// crop-parameter noise (noise.py:3-23) with a counter-based generator: Philox4x32-10
// ---------------------------------------------------------------------------------------------------
template <class T>
__global__ void crop_noise_kernel(T* crop_p, int B, int ld, const float* p0, float scale, unsigned long long seed,
                                  unsigned long long draw)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float pn[NCROP + 2];
    for (int blk = 0; blk < 9; ++blk) {
        unsigned r[4];
        philox4x32_10((unsigned)b, (unsigned)draw, (unsigned)(draw >> 32), (unsigned)blk, (unsigned)seed,
                      (unsigned)(seed >> 32), r);
        for (int q = 0; q < 4; ++q) {
            const int i = blk * 4 + q;
            if (i < NCROP) {
                const float un = ((float)(r[q] >> 8) + 0.5f) * (1.0f / 16777216.0f);      // (0,1), 24 bits
                const float noise = (un - 0.5f) * scale;
                pn[i] = p0[i] + noise * p0[i];
            }
        }
    }
    pn[144 - CROP0] = pn[141 - CROP0] / pn[142 - CROP0];            // cLeafMax = laiMax / sla (noise.py:22)
    for (int i = 0; i < NCROP; ++i) crop_p[(size_t)i * ld + b] = T(pn[i]);
}

}  // namespace

template <class T> static int launch_obs(glgym_handle h, const glgym_obs_args* a, hipStream_t st)
{
    ObsArgsT<T> k;
    k.B = a->B; k.ld = a->ld; k.x = (const T*)a->x; k.u = (const T*)a->u; k.weather = (const T*)a->weather;
    k.weather_rows = a->weather_rows; k.w_off = a->w_off; k.timestep = a->timestep; k.start_day = a->start_day;
    k.Np = a->Np; k.obs = a->obs; k.mask = a->mask; k.term_obs = a->term_obs; k.nd = h->nd;
    obs_clock_increments(h, &k.doy_inc, &k.hod_inc);
    int blocks = (a->B + OBS_ROWS - 1) / OBS_ROWS;   // OBS_ROWS env rows per block-iteration
    static const int cap = [] { const char* e = std::getenv("GLGYM_OBS_BLOCKS"); return e ? std::atoi(e) : 4096; }();
    if (blocks > cap) blocks = cap;              // grid-stride beyond that
    obs_layout(h, a->Np, k.moff, &k.dim);
    const size_t lds = (size_t)OBS_ROWS * k.dim * sizeof(float);
    hipLaunchKernelGGL((obs_kernel<T>), dim3(blocks), dim3(256), lds, st, k);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

extern "C" {

int glgym_obs(glgym_handle h, const glgym_obs_args* a, void* stream)
{
    DeviceGuard dev_guard(h);
    if (!obs_args_ok(h, a)) {
        g_err = "glgym_obs: bad arguments (null pointer, ld < B, weather_rows < 1, or Np outside 0..128)";
        return GLGYM_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    return with_dtype(h->dtype, [&](auto t) { return launch_obs<decltype(t)>(h, a, st); });
}

int glgym_set_obs_modules(glgym_handle h, const int32_t* modules, int n)
{
    if (!h || !modules || n < 1 || n > 6) { g_err = "glgym_set_obs_modules: 1..6 module ids expected"; return GLGYM_EINVAL; }
    int seen = 0;
    for (int i = 0; i < n; ++i) {
        if (modules[i] < 0 || modules[i] > 5 || (seen >> modules[i] & 1)) {
            g_err = "glgym_set_obs_modules: ids must be distinct GLGYM_OBS_* values";
            return GLGYM_EINVAL;
        }
        seen |= 1 << modules[i];
    }
    for (int i = 0; i < n; ++i) h->obs_modules[i] = modules[i];
    h->n_obs_modules = n;
    return GLGYM_OK;
}

int glgym_obs_dim(glgym_handle h, int Np)
{
    if (!h || Np < 0 || Np > OBS_MAX_NP) return GLGYM_EINVAL;
    int moff[6], dim;
    obs_layout(h, Np, moff, &dim);
    return dim;
}

int glgym_reset(glgym_handle h, const glgym_reset_args* a, void* stream)
{
    DeviceGuard dev_guard(h);
    if (!h || !reset_args_ok(a)) {
        g_err = "glgym_reset: bad arguments (null handle or pointer, B < 1, ld < B, or weather_rows < 1)";
        return GLGYM_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((a->B + 255) / 256), block(256);
    with_dtype(h->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((reset_kernel<T>), grid, block, 0, st, a->B, a->ld, a->mask, (T*)a->x, (T*)a->u,
                           a->timestep, (const T*)a->weather, a->weather_rows, a->w_off, a->start_rows, a->start_days,
                           a->n_starts, a->start_day, a->episode, (unsigned long long)a->seed, h->nd);
    });
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_crop_noise(glgym_handle h, void* crop_p, int B, int ld, double scale, uint64_t seed, uint64_t draw_index,
                     void* stream)
{
    DeviceGuard dev_guard(h);
    if (!h || !crop_p || B < 1 || ld < B) return GLGYM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((B + 255) / 256), block(256);
    with_dtype(h->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((crop_noise_kernel<T>), grid, block, 0, st, (T*)crop_p, B, ld, h->p0_crop_dev,
                           (float)scale, (unsigned long long)seed, (unsigned long long)draw_index);
    });
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_rule_based(glgym_handle h, const glgym_rule_cfg* cfg, const glgym_rule_args* a, void* stream)
{
    DeviceGuard dev_guard(h);
    if (!h || !cfg || !a || a->B < 1 || a->ld < a->B || !a->x || !a->weather || !a->w_off || !a->timestep || !a->control ||
        a->weather_rows < 1 || (!a->start_day && !a->doy) || cfg->vent_heat_Pband == 0 || cfg->vent_rh_Pband == 0 ||
        cfg->vent_cold_Pband == 0 || cfg->thScrPband == 0 || cfg->thScrRhPband == 0 || cfg->tHeatBand == 0 ||
        cfg->co2Band == 0) {
        g_err = "glgym_rule_based: bad arguments (null pointer, ld < B, or a zero proportional band)";
        return GLGYM_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((a->B + 255) / 256), block(256);
    const double doy_inc = std::fmod(h->dt / 86400.0, 365.0), hod_inc = h->dt / 3600.0;
    with_dtype(h->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((rule_based_kernel<T>), grid, block, 0, st, *cfg, a->B, a->ld, (const T*)a->x,
                           (const T*)a->weather, a->weather_rows, a->w_off, a->timestep, a->start_day, a->hour, a->doy,
                           doy_inc, hod_inc, (T*)a->control, h->nd);
    });
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

}  // extern "C"
