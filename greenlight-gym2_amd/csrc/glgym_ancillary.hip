// glgym_ancillary.hip -- what runs beside the env-step, kernels and C entry points (include/glgym.h):
//   vecnorm_*_kernel (five)                                 VecNormalize on the device (glgym_vecnorm).          [HBM bound]
//   weather_convert / weather_scan / pchip_slopes / pchip_eval   the weather pipeline, raw samples -> rows (glgym_weather).
// Nothing in here instantiates an integrating kernel.
#include <hip/hip_runtime.h>

#include "glgym_internal.h"

using namespace glm;

namespace {

constexpr int WAVE = 64;

// ---------------------------------------------------------------------------------------------------
// VecNormalize on the device (HBM-bound: one read pass for the moments, one read + write pass to normalise)
// ---------------------------------------------------------------------------------------------------
// pass 1: per-feature sum and sum of squares over the batch.  Thread t owns columns t, t+256, ... (consecutive lanes ->
// consecutive addresses of a row), walks a strip of rows in registers (fp64), then one atomic pair per column.  Eight row
// loads are issued before the first is consumed: with two in flight the pass ran at 1.7 TB/s (41.6 us for 69 MB), the
// latency-bandwidth product of the chip wants ~60 KB in flight per CU.  The atomics go to one of VN_REP replicas of the
// accumulator block (merged by vecnorm_merge_kernel): 1 024 blocks x 526 fp64 atomics onto the 33 cache lines of a single
// block serialise in the L2 -- that, not the read, was most of the pass.
constexpr int VN_REP = 16;
// The sums are taken about a pivot, the column's value in row 0: sum(x - p) and sum((x - p)^2).  The merge forms the batch
// variance as E[d^2] - E[d]^2, which cancels (mean / spread)^2 of the fp64 mantissa when taken about zero: a column of mean
// 35 040 and spread 3e-3 came out 4e-3 off at B = 65 536, and on warm statistics that reached the normalised rows
// (profiles/vecnorm_moments_cost.txt).  About a value of the column itself the two terms are of the size of the spread; the
// difference of two float32 is exact in fp64.
__global__ __launch_bounds__(1024) void vecnorm_moments_kernel(const float* __restrict__ obs, int B, int dim,
                                                               double* __restrict__ acc_all)
{
    double* acc = acc_all + (size_t)(blockIdx.x % VN_REP) * 2 * dim;
    const int rows_per_block = (B + gridDim.x - 1) / gridDim.x;
    const int r0 = blockIdx.x * rows_per_block, r1 = min(B, r0 + rows_per_block);
    for (int c = threadIdx.x; c < dim; c += blockDim.x) {       // blockDim >= dim in practice: one column per thread
        const double p = (double)obs[c];
        double s0 = 0.0, q0 = 0.0, s1 = 0.0, q1 = 0.0;
        int r = r0;
        for (; r + 7 < r1; r += 8) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = obs[(size_t)(r + j) * dim + c];
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const double a = (double)v[j] - p, b = (double)v[j + 1] - p;
                s0 += a; q0 += a * a; s1 += b; q1 += b * b;
            }
        }
        for (; r < r1; ++r) { const double v = (double)obs[(size_t)r * dim + c] - p; s0 += v; q0 += v * v; }
        if (r1 > r0) { atomicAdd(acc + c, s0 + s1); atomicAdd(acc + dim + c, q0 + q1); }
    }
}

// discounted returns + their batch moments (wave reduction, one atomic pair per wave)
template <class T>
__global__ __launch_bounds__(256) void vecnorm_returns_kernel(const T* __restrict__ reward, double* __restrict__ returns,
                                                              int B, double gamma, double* __restrict__ acc2)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    double v = 0.0;
    if (b < B) { v = returns[b] * gamma + (double)reward[b]; returns[b] = v; }
    double s = v, q = v * v;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, WAVE); q += __shfl_xor(q, o, WAVE); }
    __shared__ double part[2][4];
    const int wv = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) { part[0][wv] = s; part[1][wv] = q; }
    __syncthreads();
    if (threadIdx.x == 0) {                                   // one atomic pair per 256-env block
        atomicAdd(acc2, part[0][0] + part[0][1] + part[0][2] + part[0][3]);
        atomicAdd(acc2 + 1, part[1][0] + part[1][1] + part[1][2] + part[1][3]);
    }
}

// RunningMeanStd.update_from_moments for every feature (and for the scalar return statistics), then the batch count, then
// per-column 1/sqrt(var + eps) (fp64, so that pass 2 is two fp64 ops per element) -- ONE block: the count every column
// reads is updated after a barrier, and scale[c] may overwrite acc[c], which only column c's own thread has read.
__global__ __launch_bounds__(1024) void vecnorm_merge_kernel(double* mean, double* var, double* count, const double* acc, int dim,
                                                            int B, const float* __restrict__ obs, double* ret_stats,
                                                            const double* acc2, int do_obs, int do_ret, double eps,
                                                            double* scale)
{
    const double n = (double)B;
    const double cnt = *count;
    for (int c = threadIdx.x; c < dim; c += blockDim.x) {
        if (do_obs) {
            double sum = 0.0, sq = 0.0;
            for (int r = 0; r < VN_REP; ++r) { sum += acc[(size_t)r * 2 * dim + c]; sq += acc[(size_t)r * 2 * dim + dim + c]; }
            const double dm = sum / n, bv = fmax(sq / n - dm * dm, 0.0);      // moments about the pivot obs[0][c]
            const double bm = (double)obs[c] + dm;
            const double tot = cnt + n, delta = bm - mean[c];
            const double m2 = var[c] * cnt + bv * n + delta * delta * cnt * n / tot;
            mean[c] += delta * n / tot;
            var[c] = m2 / tot;
        }
        if (scale) scale[c] = 1.0 / sqrt(var[c] + eps);
    }
    if (do_ret && threadIdx.x == 0) {
        const double bm = acc2[0] / n, bv = fmax(acc2[1] / n - bm * bm, 0.0);
        const double rc = ret_stats[2], tot = rc + n, delta = bm - ret_stats[0];
        const double m2 = ret_stats[1] * rc + bv * n + delta * delta * rc * n / tot;
        ret_stats[0] += delta * n / tot;
        ret_stats[1] = m2 / tot;
        ret_stats[2] = tot;
    }
    __syncthreads();
    if (do_obs && threadIdx.x == 0) *count = cnt + n;
}

// pass 2: clip((x - mean) * scale).  The subtraction stays in fp64 like SB3 (float32 obs - float64 mean): for
// near-constant features a ~1e-8 difference is divided by sqrt(eps).  Lane i handles element i (coalesced).
__global__ __launch_bounds__(1024) void vecnorm_apply_kernel(const float* __restrict__ obs, float* __restrict__ out,
                                                            int B, int dim, const double* __restrict__ mean,
                                                            const double* __restrict__ scale, float clip)
{
    const int rows_per_block = (B + gridDim.x - 1) / gridDim.x;
    const int r0 = blockIdx.x * rows_per_block, r1 = min(B, r0 + rows_per_block);
    for (int c = threadIdx.x; c < dim; c += blockDim.x) {
        const double mu = mean[c], sc = scale[c];
        for (int r = r0; r < r1; ++r) {
            const size_t i = (size_t)r * dim + c;
            const float v = (float)(((double)obs[i] - mu) * sc);
            out[i] = fminf(fmaxf(v, -clip), clip);
        }
    }
}

template <class T>
__global__ void vecnorm_reward_kernel(const T* __restrict__ reward, float* __restrict__ out, double* __restrict__ returns,
                                      const unsigned char* __restrict__ done, int B, const double* ret_stats, double eps,
                                      float clip, int norm_reward)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float r = (float)reward[b];
    if (norm_reward) r = fminf(fmaxf((float)((double)reward[b] / sqrt(ret_stats[1] + eps)), -clip), clip);
    out[b] = r;
    if (done && done[b]) returns[b] = 0.0;
}


// ---------------------------------------------------------------------------------------------------
// Weather pipeline on the device (gl_gym/environments/utils.py:48-125): raw 300-s samples -> unit
// conversions -> daily light sum / daylight flags -> PCHIP resample to the env's grid.  fp64 throughout (it runs once per
// season table, not per step); the result is written in the handle's dtype.  Mirrors gl_gym_amd/utils.py
// (weather_from_raw), itself checked bit for bit against the reference's loader.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double w_sat_vp(double t) { return 610.78 * exp(17.2694 * t / (t + 238.3)); }

// columns 0..6 of the raw-grid table W[10][n] (SoA)
__global__ void weather_convert_kernel(int n, const double* __restrict__ time, const double* __restrict__ i_glob,
                                       const double* __restrict__ t_out, const double* __restrict__ rh,
                                       const double* __restrict__ wind, const double* __restrict__ t_sky, double co2_ppm,
                                       double* __restrict__ W)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const double R = 8.3144598, C2K = 273.15, M_CO2 = 44.01e-3, M_H2O = 18.01528e-3, P_ATM = 101325.0;
    const double t = t_out[k];
    const double rho_v = (rh[k] / 100.0) * w_sat_vp(t) * M_H2O / (R * (t + C2K));              // rh2vaporDens
    const double rho_sat = (100.0 / 100.0) * w_sat_vp(t) * M_H2O / (R * (t + C2K));
    W[0 * (size_t)n + k] = i_glob[k];
    W[1 * (size_t)n + k] = t;
    W[2 * (size_t)n + k] = w_sat_vp(t) * (rho_v / rho_sat);                                    // vaporDens2pres
    W[3 * (size_t)n + k] = (P_ATM * 1e-6 * co2_ppm * M_CO2 / (R * (t + C2K))) * 1e6;           // co2ppm2dens * 1e6
    W[4 * (size_t)n + k] = wind[k];
    W[5 * (size_t)n + k] = t_sky[k];
    const double year = 3600.0 * 24.0 * 365.0;
    W[6 * (size_t)n + k] = 10.0 + 5.0 * sin(2.0 * 3.14159265358979323846 * (time[k] + 0.625 * year) / year);   // soilTempNl
}

// columns 7..9: the two sequential passes of the loader (dailLightSum: utils.py:216-250; computeisDay: :177-214, whose
// later tests see the ramps written by earlier ones).  One lane: O(n) work, n ~ 3e4.
__global__ void weather_scan_kernel(int n, const double* __restrict__ time, double* __restrict__ W)
{
    if (blockIdx.x != 0 || threadIdx.x != 0 || n < 2) return;
    const double* rad = W;
    double* dli = W + 7 * (size_t)n;
    double* is_day = W + 8 * (size_t)n;
    double* smooth = W + 9 * (size_t)n;
    const double c = 86400.0, interval = time[1] - time[0];
    auto next_jump = [&](int from) {
        for (int k = from < 0 ? 0 : from; k + 1 < n; ++k)
            if (floor(time[k + 1] / c) - floor(time[k] / c) == 1.0) return k;
        return -1;
    };
    int before = 0, j = next_jump(0), after = j >= 0 ? j + 1 : n, i = 0;
    while (i < n) {
        const int seg_end = after < n ? after : n;
        double sum = 0.0;
        for (int k = before; k <= after && k < n; ++k) sum += rad[k];
        for (int k = i; k < seg_end; ++k) dli[k] = sum * interval * 1e-6;
        i = seg_end;
        if (i >= n) break;
        before = after;
        j = next_jump(before + 2);
        after = j >= 0 ? j : n;
    }
    double dt_mean = (time[n - 1] - time[0]) / (double)(n - 1);
    for (int k = 0; k < n; ++k) { is_day[k] = rad[k] > 0.0 ? 1.0 : 0.0; smooth[k] = is_day[k]; }
    const int n_tr = (int)(3600.0 / dt_mean), half = n_tr / 2;
    if (n_tr < 2) return;
    const double step = 1.0 / (double)(n_tr - 1);
    bool in_sunset = false;
    for (int k = n_tr; k < n - n_tr; ++k) {
        const double cur = is_day[k], nxt = is_day[k + 1];
        if (cur == 0.0) {
            in_sunset = false;
            if (nxt == 1.0)
                for (int q = 0; q < 2 * half && q < n_tr; ++q) {
                    const double r = (q == n_tr - 1) ? 1.0 : (double)q * step;
                    is_day[k - half + q] = r;
                    smooth[k - half + q] = 1.0 / (1.0 + exp(-10.0 * (r - 0.5)));
                }
        } else if (cur == 1.0 && nxt == 0.0 && !in_sunset) {
            for (int q = 0; q < 2 * half && q < n_tr; ++q) {
                const double r = (q == n_tr - 1) ? 1.0 : (double)q * step;
                is_day[k - half + q] = 1.0 - r;
                smooth[k - half + q] = 1.0 - 1.0 / (1.0 + exp(-10.0 * (r - 0.5)));
            }
            in_sunset = true;
        }
    }
}

// PCHIP slopes (Fritsch-Carlson as scipy.interpolate.PchipInterpolator): D[c][k]
__device__ __forceinline__ double w_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }
__device__ __forceinline__ double pchip_edge(double h0, double h1, double m0, double m1)
{
    double d = ((2.0 * h0 + h1) * m0 - h0 * m1) / (h0 + h1);
    if (w_sign(d) != w_sign(m0)) d = 0.0;
    else if (w_sign(m0) != w_sign(m1) && fabs(d) > 3.0 * fabs(m0)) d = 3.0 * m0;
    return d;
}
__global__ void pchip_slopes_kernel(int n, int n_col, const double* __restrict__ x, const double* __restrict__ W,
                                    double* __restrict__ D)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x, col = blockIdx.y;
    if (k >= n || col >= n_col) return;
    const double* y = W + (size_t)col * n;
    auto h = [&](int i) { return x[i + 1] - x[i]; };
    auto m = [&](int i) { return (y[i + 1] - y[i]) / h(i); };
    double d;
    if (n == 2) d = m(0);
    else if (k == 0) d = pchip_edge(h(0), h(1), m(0), m(1));
    else if (k == n - 1) d = pchip_edge(h(n - 2), h(n - 3), m(n - 2), m(n - 3));
    else {
        const double m0 = m(k - 1), m1 = m(k), h0 = h(k - 1), h1 = h(k);
        if (w_sign(m0) != w_sign(m1) || m0 == 0.0 || m1 == 0.0) d = 0.0;
        else {
            const double w1 = 2.0 * h1 + h0, w2 = h1 + 2.0 * h0;
            d = 1.0 / ((w1 / m0 + w2 / m1) / (w1 + w2));
        }
    }
    D[(size_t)col * n + k] = d;
}

// evaluation on linspace(x[0], x[n-1], n_out) in the power-series order of scipy's PPoly; iGlob < 1e-10 -> 0
template <class T>
__global__ void pchip_eval_kernel(int n, int n_col, int n_out, int nd, const double* __restrict__ x,
                                  const double* __restrict__ W, const double* __restrict__ D, T* __restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, col = blockIdx.y;
    if (i >= n_out || col >= n_col) return;
    const double start = x[0], stop = x[n - 1];
    const double stepo = n_out > 1 ? (stop - start) / (double)(n_out - 1) : 0.0;
    double t = stop;
    if (i < n_out - 1 || n_out == 1) {
        // numpy's linspace rounds i * step before it adds start; fused into one FMA the point moves by an ulp of t (2e-9 s at
        // day 100), which a zig-zag column with knots 300 s apart turns into 6e-12 of its range
#pragma clang fp contract(off)
        t = (double)i * stepo + start;
    }
    int lo = 0, hi = n - 1;                         // last k with x[k] <= t, clipped to n - 2
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (x[mid] <= t) lo = mid; else hi = mid; }
    const int k = lo > n - 2 ? n - 2 : lo;
    const double* y = W + (size_t)col * n;
    const double* d = D + (size_t)col * n;
    const double dx = x[k + 1] - x[k], slope = (y[k + 1] - y[k]) / dx;
    const double tt = (d[k] + d[k + 1] - 2.0 * slope) / dx;
    const double c0 = tt / dx, c1 = (slope - d[k]) / dx - tt, c2 = d[k], c3 = y[k];
    const double sdx = t - x[k];
    double res = 0.0, z = 1.0;
    res += c3 * z; z *= sdx;
    res += c2 * z; z *= sdx;
    res += c1 * z; z *= sdx;
    res += c0 * z;
    if (col == 0 && res < 1e-10) res = 0.0;
    out[(size_t)i * nd + col] = T(res);
}

}  // namespace

extern "C" int glgym_weather(glgym_handle h, const glgym_weather_args* a, void* stream)
{
    DeviceGuard dev_guard(h);
    if (!h || !a || a->n_raw < 3 || a->n_out < 1 || a->nd < ND || !a->time || !a->i_glob || !a->t_out || !a->rh || !a->wind ||
        !a->t_sky || !a->out || !a->workspace) {
        g_err = "glgym_weather: bad arguments (>= 3 raw samples, nd >= 10, non-null device pointers)";
        return GLGYM_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int n = a->n_raw;
    double* W = a->workspace;                       // [10][n] converted columns on the raw grid
    double* D = a->workspace + (size_t)10 * n;      // [10][n] PCHIP slopes
    hipLaunchKernelGGL(weather_convert_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, a->time, a->i_glob, a->t_out,
                       a->rh, a->wind, a->t_sky, a->co2_ppm, W);
    hipLaunchKernelGGL(weather_scan_kernel, dim3(1), dim3(64), 0, st, n, a->time, W);
    hipLaunchKernelGGL(pchip_slopes_kernel, dim3((n + 255) / 256, 10), dim3(256), 0, st, n, 10, a->time, W, D);
    if (a->nd > ND) {                               // extra columns (ODE_pipe rows) are the caller's: start from zero
        HIPCHK(hipMemsetAsync(a->out, 0, (size_t)a->n_out * a->nd * (h->dtype == GLGYM_F32 ? 4 : 8), st));
    }
    const dim3 grid((a->n_out + 255) / 256, 10);
    with_dtype(h->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((pchip_eval_kernel<T>), grid, dim3(256), 0, st, n, 10, a->n_out, a->nd, a->time, W, D, (T*)a->out);
    });
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

extern "C" int glgym_vecnorm(glgym_handle h, const glgym_vecnorm_args* a, void* stream)
{
    DeviceGuard dev_guard(h);
    if (!h || !a || a->B < 1 || a->dim < 1 || !a->obs || !a->obs_out || !a->obs_mean || !a->obs_var || !a->obs_count ||
        !a->workspace || (a->reward && (!a->reward_out || !a->ret_stats || !a->returns))) {
        g_err = "glgym_vecnorm: bad arguments";
        return GLGYM_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    const int B = a->B, dim = a->dim;
    double* acc = a->workspace;
    double* acc2 = a->workspace + (size_t)VN_REP * 2 * dim;
    HIPCHK(hipMemsetAsync(a->workspace, 0, ((size_t)VN_REP * 2 * dim + 2) * sizeof(double), st));
    const int do_obs = a->training && a->norm_obs, do_ret = a->training && a->reward != nullptr;
    int col_threads = (dim + WAVE - 1) / WAVE * WAVE;       // one thread per observation column
    if (col_threads > 1024) col_threads = 1024;
    if (do_obs) {
        int blocks = (B + 63) / 64;                 // 64-row strips: <= 1024 blocks x 2*dim fp64 atomics
        if (blocks > 1024) blocks = 1024;
        hipLaunchKernelGGL(vecnorm_moments_kernel, dim3(blocks), dim3(col_threads), 0, st, a->obs, B, dim, acc);
    }
    if (do_ret) {
        with_dtype(h->dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((vecnorm_returns_kernel<T>), dim3((B + 255) / 256), dim3(256), 0, st,
                               (const T*)a->reward, a->returns, B, a->gamma, acc2);
        });
    }
    double* scale = acc;                           // the moment accumulators are dead once their column is merged
    if (do_obs || do_ret || a->norm_obs)
        hipLaunchKernelGGL(vecnorm_merge_kernel, dim3(1), dim3(1024), 0, st, a->obs_mean, a->obs_var, a->obs_count, acc, dim, B,
                           a->obs, a->ret_stats, acc2, do_obs, do_ret, a->epsilon, a->norm_obs ? scale : nullptr);
    const size_t total = (size_t)B * dim;
    if (a->norm_obs) {
        int blocks = (B + 15) / 16;
        if (blocks > 8192) blocks = 8192;
        hipLaunchKernelGGL(vecnorm_apply_kernel, dim3(blocks), dim3(col_threads), 0, st, a->obs, a->obs_out, B, dim,
                           a->obs_mean, scale, a->clip_obs);
    } else if (a->obs_out != a->obs) {
        HIPCHK(hipMemcpyAsync(a->obs_out, a->obs, total * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    if (a->reward) {
        with_dtype(h->dtype, [&](auto t) {
            using T = decltype(t);
            hipLaunchKernelGGL((vecnorm_reward_kernel<T>), dim3((B + 255) / 256), dim3(256), 0, st,
                               (const T*)a->reward, a->reward_out, a->returns, a->done, B, a->ret_stats, a->epsilon,
                               a->clip_reward, a->norm_reward);
        });
    }
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}
