// glgym.hip -- gfx950 kernels + the C ABI declared in include/glgym.h.
//
// Kernels (one lane = one environment; a 64-lane wavefront = one workgroup = 64 environments):
//   step_kernel   fused TomatoEnv.step(): action->control, weather-row gather, tier-2 precompute,
//                 n_sub x RK4 of the GreenLight ODE (gl_model.hpp), failure check, reward / violation /
//                 info epilogue, terminal test, wave-level metric reduction.   [VALU/transcendental bound]
//                 OBS builds (glgym_step_obs): the same, and each wavefront then also writes the observation rows of its 64 environments.
//   obs_kernel    row-major observation assembly incl. the weather-forecast gather.      [HBM-write bound]
//   reset_kernel  masked init_state().        crop_noise_kernel  Philox4x32-10 parameter noise.
//   evalf_kernel / rhs_kernel                 row-major double I/O for the reference-compatible evalF and tests.
// No MFMA anywhere: the path is elementwise + transcendental, not a contraction.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "glgym.h"
#include "gl_model.hpp"
#include "gl_model_quad.hpp"
#include "gl_reward.hpp"
#include "gl_step_select.hpp"
#include "glgym_bdf.h"
#include "glgym_rng.h"
#include "glgym_plan.h"

using namespace glm;

namespace {

thread_local std::string g_err;

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                                 \
            return GLGYM_EHIP;                                                                         \
        }                                                                                              \
    } while (0)

constexpr int WAVE = 64;

// ---------------------------------------------------------------------------------------------------
// constants of the DEFAULT parameter block, visible to the compiler (see gen_default_const.cpp)
// ---------------------------------------------------------------------------------------------------
#include "gl_default_const.inc"
static_assert(sizeof(ModelConst<float>) == sizeof(kDefaultConstF32_image), "regenerate gl_default_const.inc");
static_assert(sizeof(ModelConst<double>) == sizeof(kDefaultConstF64_image), "regenerate gl_default_const.inc");
template <class T> struct DefaultConst;
template <> struct DefaultConst<float> {
    static constexpr ModelConst<float> value = __builtin_bit_cast(ModelConst<float>, kDefaultConstF32_bits);
};
template <> struct DefaultConst<double> {
    static constexpr ModelConst<double> value = __builtin_bit_cast(ModelConst<double>, kDefaultConstF64_bits);
};
// Device-side objects with the same constant initialisers: the kernels bind references to THESE (a host constexpr has
// no device address; only its folded values exist there).  Being const with a constant initialiser, every load from
// them that the optimiser can see still folds to a literal.
__constant__ const ModelConst<float> g_default_f32 = __builtin_bit_cast(ModelConst<float>, kDefaultConstF32_bits);
__constant__ const ModelConst<double> g_default_f64 = __builtin_bit_cast(ModelConst<double>, kDefaultConstF64_bits);
template <class T> __device__ __forceinline__ const ModelConst<T>& device_default();
template <> __device__ __forceinline__ const ModelConst<float>& device_default<float>() { return g_default_f32; }
template <> __device__ __forceinline__ const ModelConst<double>& device_default<double>() { return g_default_f64; }

// ---------------------------------------------------------------------------------------------------
// reward constants (gl_reward.hpp, shared with the BDF env-step of glgym_bdf.hip)
// ---------------------------------------------------------------------------------------------------
template <class T> struct RewardConst : RewardConstBase<T> {};

template <class T> struct StepArgsT {
    int B, ld;
    T* x; T* u;
    const float* action; const T* control;
    const T* weather; int weather_rows;
    const int* w_off; int* timestep;
    const T* crop_p;
    int N;
    T* reward; T* info; unsigned char* done; float* metrics; int* step_flags;
    T dt; int n_sub;
    T gasR, tCanMin;
    int nd;                     // weather row stride (10, or 14 with the measured-pipe columns of ODE_pipe)
    float du, u_min[NU], u_max[NU];      // action_to_control: clip(u + action * delta_u_max, u_min, u_max)
    int verify;                 // 1: step-doubling verified integration (rk4_delta_guarded), see glgym_set_verify
    int pipe;                   // 1: the handle's ODE variant is GLGYM_ODE_PIPE (kernels that select the variant at run time)
    int window;                 // > 0: nominal sub-steps per tier-2b window, overriding the scheme's own (glgym_set_window)
};

template <class T> __device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// ---------------------------------------------------------------------------------------------------
// the 23 core observation features (observations.py:70-161), shared by obs_kernel and the observation epilogue of step_kernel
// ---------------------------------------------------------------------------------------------------
// j: 0 co2_ppm(x0,x2) 1 x2 2 RH(x15,x2) 3 x9 | 4 x21 5 x25 6 x26 | 7..12 u | 13 d0 14 d1 15 RH(d2,d1)
//    16 co2_ppm(d3,d1) 17 d4 | 18 timestep 19..22 sin/cos clocks
// prim: the feature's own input (x, u or weather column; unused from j = 18), aux: tAir (j < 13) or tOut.  ts: the env's timestep AFTER
// the step's increment; the row / "timestep" the reference shows is the pre-increment one, k = ts - 1 (0 for a freshly reset env).
// Straight-line selects: with a run-time j (obs_kernel) no branch per feature, with a compile-time j (step_kernel) everything but the
// feature's own arithmetic folds away.  ONE definition, so that both kernels produce the same bits.
constexpr int OBS_NCORE = 23;
__device__ __forceinline__ float obs_core_feature(int j, float prim, float aux, float sday, int ts, double doy_inc, double hod_inc)
{
    // No implicit contraction in here: which products the compiler fuses into a following add depends on the caller -- with a
    // compile-time j it turned rev - floor(rev) into fma(t, c, -floor(t * c)), which is not 0 where rev is a whole number (step 96 of
    // an episode), with a run-time j it did not.  The one fused operation obs_kernel has always had is written out.
#pragma clang fp contract(off)
    const float kPpm = (float)(8.3144598 / (101325.0 * 44.01e-3));
    const int k = ts > 0 ? ts - 1 : 0;
    // fp32 hardware transcendentals: the observation block is float32 (observation_space dtype)
    const float sat = 610.78f * __builtin_amdgcn_exp2f(1.44269504f * 17.2694f * aux * __builtin_amdgcn_rcpf(aux + 238.3f));
    const float rh = fminf(fmaxf(100.0f * prim * __builtin_amdgcn_rcpf(sat), 0.0f), 100.0f);
    const float ppm = kPpm * (aux + 273.15f) * prim;
    // v_sin_f32 / v_cos_f32 take revolutions: sin(2*pi*x)   (tomato_env.py:126-128)
    const int c = j - 18;
    const double rev = (c <= 2) ? __builtin_fma((double)ts, doy_inc, (double)sday) * (1.0 / 365.0)
                                : (double)ts * hod_inc * (1.0 / 24.0);
    const float fr = (float)(rev - floor(rev));
    const float clk = (c == 1 || c == 3) ? __builtin_amdgcn_sinf(fr) : __builtin_amdgcn_cosf(fr);
    float v = prim;
    v = (j == 0 || j == 16) ? ppm : v;
    v = (j == 2 || j == 15) ? rh : v;
    v = (j == 18) ? (float)k : v;
    v = (j > 18) ? clk : v;
    return v;
}
// module (GLGYM_OBS_*) and column inside it of core feature j
__device__ __forceinline__ constexpr int obs_core_module(int j) { return j < 4 ? 0 : j < 7 ? 1 : j < 13 ? 2 : j < 18 ? 3 : 4; }
__device__ __forceinline__ constexpr int obs_core_col(int j) { return j < 4 ? j : j < 7 ? j - 4 : j < 13 ? j - 7 : j < 18 ? j - 13 : j - 18; }

// counter-based generator shared by the reset (episode start draw) and crop-noise kernels
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned* out)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ---------------------------------------------------------------------------------------------------
// one environment's reset: the episode start draw and init_state (utils.py:13-46) -- reset_kernel's body, shared with the auto-reset
// epilogue of step_kernel.  ONE definition, so that both produce the same bits.
// ---------------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void reset_env(int b, int ld, T* x, T* u, int* timestep, const T* weather, int weather_rows, int* w_off,
                                          const int* start_rows, const float* start_days, int n_starts, float* start_day, int* episode,
                                          unsigned long long seed, int nd)
{
    // No implicit contraction in here (obs_core_feature): the two fused operations reset_kernel has always had are written out.
#pragma clang fp contract(off)
    if (start_rows && n_starts > 0) {            // draw this episode's start (tomato_env.py:236-244)
        const int ep = episode ? episode[b] : 0;
        unsigned rnd[4];
        philox4x32_10((unsigned)b, (unsigned)ep, 0x5eedu, 0u, (unsigned)seed, (unsigned)(seed >> 32), rnd);
        const int j = (int)(rnd[0] % (unsigned)n_starts);
        w_off[b] = start_rows[j];
        if (start_day && start_days) start_day[b] = start_days[j];
        if (episode) episode[b] = ep + 1;
    }
    int r = w_off[b];
    r = r < 0 ? 0 : (r >= weather_rows ? weather_rows - 1 : r);
    const double co2Out = (double)weather[(size_t)r * nd + 3], tSoOut = (double)weather[(size_t)r * nd + 6];
    const double tAir = 16.5;
    double xi[NX];
    xi[0] = xi[1] = co2Out;
    for (int i = 2; i <= 10; ++i) xi[i] = tAir;
    xi[4] = tAir + 4;
    xi[11] = 0.25 * (3.0 * tAir + tSoOut);
    xi[12] = 0.25 * __builtin_fma(2.0, tSoOut, 2.0 * tAir);
    xi[13] = 0.25 * __builtin_fma(3.0, tSoOut, tAir);
    xi[14] = tSoOut;
    xi[15] = xi[16] = 90.0 / 100.0 * (610.78 * exp(17.2694 * tAir / (tAir + 238.3)));
    xi[17] = xi[18] = xi[19] = xi[20] = tAir;
    xi[21] = xi[4];
    xi[22] = 0.0; xi[23] = 9.5283e4; xi[24] = 2.5107e5; xi[25] = 5.5338e4; xi[26] = 3.0978e3; xi[27] = 0.0;
    for (int i = 0; i < NX; ++i) x[(size_t)i * ld + b] = T(xi[i]);
    for (int j = 0; j < NU; ++j) u[(size_t)j * ld + b] = T(0);
    timestep[b] = 0;
}

#ifndef GL_OBS_ROWS
#define GL_OBS_ROWS 16
#endif
constexpr int OBS_ROWS = GL_OBS_ROWS, OBS_MAX_NP = 128;     // obs_kernel's LDS span = rows * (23 + 5 Np) floats <= 42 KB
// what step_kernel's OBS build needs beyond StepArgsT to write the observation rows of its 64 environments (obs_kernel's arguments
// that the step does not have already)
struct StepObsArgs {
    float* obs; const float* start_day;
    double doy_inc, hod_inc;
    int Np, dim, moff[6];
};
// widest row the epilogue can stage.  Two-waves build: what its window buffer (64 x 73 floats) holds of OBS_ROWS rows, 292 columns.
// One-wave build: a static area of its own, 512 columns = 32 KB, 37 - 38 KB per workgroup with everything else: the four workgroups of
// a CU (one wavefront per SIMD) fit its 160 KB.  NOT less: the compiler keeps the integrator's small per-window arrays in LDS only
// while that does not lower the occupancy tier which the kernel's LDS use already implies; with a 18.7 KB or a 24 KB area (tiers of
// eight and six workgroups per CU) it sent them to scratch instead, inside the window loop (profiles/step_obs_fusion.txt).
constexpr int STEP_OBS_MAX_DIM_OCC2 = WAVE * ((2 * NX + GL_N_SLOW) | 1) / OBS_ROWS, STEP_OBS_MAX_DIM_OCC1 = 512;
struct StepNoObs {};
// ... and what the auto-reset epilogue needs on top (glgym_step_obs_reset): the terminal-observation block and reset_kernel's arguments that
// the step does not have already (w_off / start_day are the step's and the observation's own buffers, writable here)
struct StepObsResetArgs : StepObsArgs {
    float* term_obs;
    int* w_off_rw; float* start_day_rw; int* episode;
    const int* start_rows; const float* start_days; int n_starts;
    unsigned long long seed;
};
constexpr int GL_SCH_OBS = 8;          // step_kernel's scheme argument: | GL_SCH_OBS = the build with the observation epilogue
constexpr int GL_SCH_RESET = 16;       // | GL_SCH_RESET (with GL_SCH_OBS): the auto-reset epilogue behind it
template <int EPI> struct StepObsSel { using type = StepNoObs; };
template <> struct StepObsSel<GL_SCH_OBS> { using type = StepObsArgs; };
template <> struct StepObsSel<GL_SCH_OBS | GL_SCH_RESET> { using type = StepObsResetArgs; };

// ---------------------------------------------------------------------------------------------------
// fused env-step
// ---------------------------------------------------------------------------------------------------
// DEFAULT_P = true: the handle's parameter block is bit-identical to the default one, so every tier-1 constant is a
// compile-time literal (no SGPRs, constant products folded, zero-coefficient exchange terms removed).
#ifndef GL_STEP_WAVES_PER_SIMD
#define GL_STEP_WAVES_PER_SIMD 1
#endif
// Tier-2b / harvest window of the RK4 scheme: FOUR sub-steps (15 s at the default n_sub 240) in both precisions (round 4; two in
// round 3, three mid-round).  The per-window work -- tier 2b, the rate-bound stage, estimate, limiter: 820 instructions -- is then
// shared by 16 stages.  Measured on the GPU, window 2 / 3 / 4 at n_sub 240: 6.82e7 / 7.7e7 / 8.15e7 env-steps/s; 10-day fixture
// fp32 2.41e-5 / 2.43e-5 / 2.93e-5, fp64 8.3e-6 / 8.5e-6 / 1.5e-5; storm fixture 4e-6 -> 8e-6, jump fixture 2.5e-5 -> 4.5e-5 (0 of
// 576 above 1e-4, 0 failed); tight one-step tuples 2.4e-5 / 3.5e-5 / 6.2e-5 in fp64 -- all of the growth one artificial tuple that
// starts with an EMPTY carbohydrate buffer (every other tuple 2.4e-5 at any window; the CPU studies); 0 flagged
// first attempts in 1.3e8 env-steps of the bench workload.  Window 5 would put that tuple at 9.6e-5: not taken.
// (Midpoint scheme: 4 sub-steps, three-stage scheme: 3.)
#ifndef GL_RK4_WIN_F32
#define GL_RK4_WIN_F32 4
#endif
#ifndef GL_RK4_WIN_F64
#define GL_RK4_WIN_F64 4
#endif
template <class T> struct RK4_WINDOW { static constexpr int value = sizeof(T) == 4 ? GL_RK4_WIN_F32 : GL_RK4_WIN_F64; };
// SCH (template argument of the integrating kernels) = GLGYM_SCHEME_*: 0 RK4, 1 the midpoint member (four sub-steps per tier-2b
// window), 2 the three-stage member (three) of the exponential family (gl_model.hpp rk_delta)
// 3 (GLGYM_SCHEME_LS5): the five-stage fourth-order 2N scheme, two sub-steps per window (gl_model.hpp rk_delta ORDER 5)
constexpr int gl_order(int sch) { return sch == 0 ? 4 : sch == 1 ? 2 : sch == 2 ? 3 : 5; }
template <class T, int SCH> struct SchemeWin { static constexpr int value = SCH == 0 ? RK4_WINDOW<T>::value : SCH == 1 ? 4 : SCH == 2 ? 3 : 2; };

// PIPE = true: the reference's ODE_pipe variant (ode.hpp:126-263; weather rows carry tPipe / pipeSwitchOff in columns 10 / 12).
// SCH = GLGYM_SCHEME_RK2 / _RK3: midpoint / three-stage sub-steps, tier 2b and the harvest flow shared by four / three of them,
// instead of RK4 sub-steps (GLGYM_SCHEME_RK4) -- rk_delta<T, PIPE, ORDER, WIN> in gl_model.hpp.  One lane per environment: fp32 only.
// OCC = waves per SIMD the kernel is compiled for.  1: up to 512 registers per lane, no scratch -- the right choice
// when the batch gives every SIMD one wave (B <= 65 536).  2: 256 registers per lane so that two waves share a SIMD -- a lone
// wave issues a vector instruction only every ~5 cycles, two co-resident waves one every ~2.7 (tools/microbench.hip with
// verified placement, profiles/r02_microbench_issue_rates.txt).  Rounds 2-4 measured 0.70x for that build: its 120 spilled
// registers were re-read from scratch at every window, 2 x 63 MB of scratch per launch did not fit the L2 (1.4 GB of HBM reads per
// launch, 41 % of the wave cycles waiting: tools/pmc_occ2.sh).  Round 5: what the windows read once each (z0, del, the slow
// slots' differences; x0 is re-read after the integrator) lives in LDS, 73 floats per lane = eight wavefronts per CU
// (rk_delta<WBUF>); 208 B of scratch are left and stay in the L2: 1.06x at B = 131 072, 1.08x at 262 144, 1.11x from 524 288 --
// the build batches of two or more wavefronts per SIMD take (launch_step).
// OBS = true (glgym_step_obs): after its stores, each wavefront also writes the observation rows of its own 64 environments -- what
// obs_kernel in full mode would write after the launch -- from the values its lanes hold, so that the rows of all but the slowest
// wavefront are written while the launch waits for that one anyway.  A template argument, not a run-time branch: the build that runs
// when no observation is asked for is the kernel it was (registers, scratch, the sub-step loop).
// It rides on the scheme argument -- SCHX = GLGYM_SCHEME_* | GL_SCH_OBS -- so that the plain builds keep the names they have always had
// (step_kernel<float, false, true, false, 3, 1> in every profile on record; tests/test_capi_surface.py finds its kernels by that prefix).
template <class T, bool PER_ENV_CROP, bool DEFAULT_P, bool PIPE = false, int SCHX = 0, int OCC = GL_STEP_WAVES_PER_SIMD>
__global__ __launch_bounds__(WAVE, OCC) void step_kernel(StepArgsT<T> a, ModelConst<T> m_arg, RewardConst<T> rw,
                                                         typename StepObsSel<(SCHX & (GL_SCH_OBS | GL_SCH_RESET))>::type o)
{
    constexpr bool OBS = (SCHX & GL_SCH_OBS) != 0, RST = (SCHX & GL_SCH_RESET) != 0;
    constexpr int SCH = SCHX & (GL_SCH_OBS - 1);
    static_assert(!OBS || (sizeof(T) == 4 && !PIPE), "observation epilogue: fp32, default ODE");
    static_assert(!RST || (OBS && !PER_ENV_CROP), "auto-reset epilogue: behind the observation epilogue, shared crop parameters");
    const ModelConst<T>& m = DEFAULT_P ? device_default<T>() : m_arg;
    // OCC = 2 (round 5): what the windows read once each -- z0, the increments del, the slow slots' window differences -- lives in LDS,
    // WSTRIDE floats per lane (odd: conflict-free), 19.2 KB per wavefront = eight wavefronts per CU; the action tile of the prologue
    // shares the storage (it is consumed before the integrator starts).  gl_model.hpp rk_delta<WBUF>.
    constexpr bool WBUF = OCC == 2;
    constexpr int WSTRIDE = (2 * NX + GL_N_SLOW) | 1;
    alignas(16) __shared__ float sh_w[WBUF ? WAVE * WSTRIDE : WAVE * NU];      // (the alignment the compiler gives it anyway; OBS reads it back with 16-byte loads)
    float* sh_act = sh_w;
    const int lane = threadIdx.x;
    const int b0 = blockIdx.x * WAVE;
    const int b = b0 + lane;
    const bool live = b < a.B;
    const int bb = live ? b : a.B - 1;        // out-of-range lanes shadow the last env, stores are masked

    // ---- controls: coalesced tile load of the row-major action block through LDS
    T u[NU];
    if (a.action) {
        const int n_tile = min(WAVE, a.B - b0) * NU;
        for (int i = lane; i < n_tile; i += WAVE) sh_act[i] = a.action[(size_t)b0 * NU + i];
        __syncthreads();
        const int l = live ? lane : (a.B - 1 - b0);
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const float inc = sh_act[l * NU + j] * a.du;                     // f32 product, as tomato_env.py:113
            const T v = a.u[(size_t)j * a.ld + bb] + T(inc);
            u[j] = Math<T>::min(Math<T>::max(v, T(a.u_min[j])), T(a.u_max[j]));
        }
    } else {
#pragma unroll
        for (int j = 0; j < NU; ++j) u[j] = a.control[(size_t)j * a.ld + bb];
    }

    // ---- state + the weather row of this step (zero-order hold, tomato_env.py:120)
    T x0[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x0[i] = a.x[(size_t)i * a.ld + bb];
    const int ts = a.timestep[bb];
    int row = a.w_off[bb] + ts;
    row = row < 0 ? 0 : (row >= a.weather_rows ? a.weather_rows - 1 : row);
    T d[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) d[j] = a.weather[(size_t)row * a.nd + j];

    // ---- tier 2, then the sub-stepped RK4
    CropConst<T> crLocal;
    if (PER_ENV_CROP) {
        T pc[NCROP];
#pragma unroll
        for (int i = 0; i < NCROP; ++i) pc[i] = a.crop_p[(size_t)i * a.ld + bb];
        make_crop_const<T, T>(pc, a.gasR, a.tCanMin, crLocal);
    }
    const CropConst<T>& cr = PER_ENV_CROP ? crLocal : m.crop;
    // (fp64: keeping this block in LDS instead -- 79 doubles x 64 lanes = 40 KB per wave -- was built and measured: the
    // generic kernel still needs 494 registers + 2 512 B of scratch, against 512 + 3 016 B, because the six 28-entry stage
    // arrays alone are 336 registers in fp64; not kept)
    StepCoef<T> s_reg;
    precompute(u, d, m, cr, s_reg);
    if (PIPE) {                                                           // ode.hpp:184-189
        const T tPipe = a.weather[(size_t)row * a.nd + 10], swOff = a.weather[(size_t)row * a.nd + 12];
        s_reg.pipeTrack = ((tPipe < T(1)) || (swOff > T(0))) ? T(0) : T(1);
        s_reg.tPipeSet = tPipe;
    }
    const StepCoef<T>& s = s_reg;
    // the applied control is final here (self.u is set before evalF and survives a failed integration, tomato_env.py:117-123):
    // store it now and re-read the three entries the reward needs afterwards, so that no u[] stays live across the integrator
    if (live) {
#pragma unroll
        for (int j = 0; j < NU; ++j) a.u[(size_t)j * a.ld + b] = u[j];
    }
    T del_reg[WBUF ? 1 : NX];
    T* wb = reinterpret_cast<T*>(sh_w) + (size_t)lane * WSTRIDE;
    T* del = WBUF ? wb + NX + GL_N_SLOW : del_reg;
    if (WBUF) {
        __syncthreads();                                   // every lane has taken its actions out of the shared storage
#pragma unroll
        for (int i = 0; i < NX; ++i) wb[i] = x0[i];
        wb[5] = x0[3] - x0[5]; wb[7] = x0[2] - x0[7]; wb[20] = x0[2] - x0[20]; wb[6] = x0[5] - x0[6];      // rk_delta's coordinates
    }
    bool bad;
    int extra_steps, first_flags = 0;
    const int retries = rk4_delta_guarded<T, PIPE, gl_order(SCH), SchemeWin<T, SCH>::value, WBUF>(x0, s, m, cr, a.dt, a.n_sub, del, &bad, &extra_steps, a.verify != 0, &first_flags, a.window, wb);
    const T uBoil = a.u[(size_t)0 * a.ld + bb], uCo2 = a.u[(size_t)1 * a.ld + bb], uLamp = a.u[(size_t)4 * a.ld + bb];
    if (WBUF) {                                            // the state again (not kept across the integrator in this build)
#pragma unroll
        for (int i = 0; i < NX; ++i) x0[i] = a.x[(size_t)i * a.ld + bb];
    }

    // ---- failure (tomato_env.py:119-123: on an integrator error the state is left unchanged and the env terminates)
    T x1[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x1[i] = bad ? x0[i] : x0[i] + del[i];
    {   // x27 = time [days since reset]: exact from the step counter when the episode started at 0 (it always does in
        // the reference), so that fp32 storage does not random-walk over a 5 761-step season
        const double per_step = (double)a.dt / 86400.0;
        double t_start = (double)x0[NX - 1] - (double)ts * per_step;
        if (fabs(t_start) < 5e-4) t_start = 0.0;
        if (!bad) x1[NX - 1] = T(t_start + ((double)ts + 1.0) * per_step);
    }

    // ---- reward epilogue (rewards.py:156-231); indoor obs conversions (observations.py:70-77)
    const T co2ppm = rw.kPpm * (x1[2] + T(273.15)) * x1[0];
    const T rh = Math<T>::min(Math<T>::max(T(100) * x1[15] / sat_vp_exact(x1[2]), T(0)), T(100));
    const T o3[3] = {co2ppm, x1[2], rh};
    T viol[3], pen = T(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        viol[i] = Math<T>::max(rw.lo[i] - o3[i], T(0)) + Math<T>::max(o3[i] - rw.hi[i], T(0));
        pen += viol[i] * rw.invMaxViol[i];
    }
    const T heat = uBoil * rw.heatK, elec = uLamp * rw.elecK, co2c = uCo2 * rw.co2K;
    const T varc = heat + co2c + elec;
    const T gains = (bad ? T(0) : del[25]) * rw.gainK;
    const T profit = gains - varc;
    const T reward = (profit - rw.minProfit) * rw.invRange - pen;        // lamp penalty is identically 0 (:203-212)
    const bool term = bad || (ts >= a.N);

    if (live) {
#pragma unroll
        for (int i = 0; i < NX; ++i) a.x[(size_t)i * a.ld + b] = x1[i];
        a.timestep[b] = ts + 1;
        a.reward[b] = reward;
        a.done[b] = term ? 1 : 0;
        if (a.step_flags) a.step_flags[b] = first_flags | (retries << 8) | (bad ? GLGYM_SF_FAILED : 0) | (min(extra_steps, 32767) << 16);
        if (a.info) {
            const T inf[GLGYM_NINFO] = {profit, gains, varc, rw.fixedCosts, co2c, heat, elec, viol[1], viol[0], viol[2], T(0)};
#pragma unroll
            for (int i = 0; i < GLGYM_NINFO; ++i) a.info[(size_t)i * a.ld + b] = inf[i];
        }
    }
    if (a.metrics) {     // wave-level reductions, one atomic per wave per metric
        const float w = live ? 1.f : 0.f;
        float mv[GLGYM_NMETRIC] = {w * (float)reward, w * (float)profit, (live && term) ? 1.f : 0.f,
                                   (live && bad) ? 1.f : 0.f, w * (float)viol[0], w * (float)viol[1],
                                   w * (float)viol[2], w, w * (float)retries, w * (float)extra_steps,
                                   (live && (first_flags & SC_FLAG_ERR)) ? 1.f : 0.f, (live && (first_flags & SC_FLAG_BRANCH)) ? 1.f : 0.f,
                                   (live && (first_flags & (SC_FLAG_CAP | SC_FLAG_NONFINITE))) ? 1.f : 0.f,
                                   (live && (first_flags & 16)) ? 1.f : 0.f};
        // one atomic per wave per metric, onto the wave's replica of the accumulator block (its own 128-byte line): 1 024 waves
        // finishing together onto ONE line serialised in the L2 for 52 us per launch
        float* mrep = a.metrics + (size_t)(blockIdx.x % GLGYM_METRIC_REPLICAS) * GLGYM_METRIC_STRIDE;
#pragma unroll
        for (int i = 0; i < GLGYM_NMETRIC; ++i) {
            const float sum = wave_sum(mv[i]);
            if (lane == 0) atomicAdd(mrep + i, sum);
        }
    }
    if constexpr (OBS) {
        // ---- observation epilogue: rows b0 .. b0 + 63 of the row-major block, obs_kernel's full mode for this wavefront's environments.
        // Every lane computes the 23 core features of its own row from the registers it has just stored (x1; the control and the
        // weather row, which did not stay live across the integrator, are re-read by the lane that wrote / gathered them); the rows are
        // assembled OBS_ROWS at a time in LDS with obs_kernel's span layout -- the two-waves build in its window buffer, which is dead
        // here -- the forecast elements gathered from the L2-resident table, one element of all 16 rows per lane and pass, and the span
        // streamed out with 16-byte non-temporal stores ((b0 + 16 s) * dim * 4 bytes is a multiple of 64).
        typedef float v4f __attribute__((ext_vector_type(4)));
        float* span;
        if constexpr (WBUF) {
            span = sh_w;
        } else {
            __shared__ float4 sh_obs4[OBS_ROWS * STEP_OBS_MAX_DIM_OCC1 / 4];      // static, and this size: see STEP_OBS_MAX_DIM_OCC1
            span = reinterpret_cast<float*>(sh_obs4);
        }
        const int dim = o.dim;
        const int ts1 = ts + 1;                             // what the step has stored: obs_kernel's `ts`
        const int base = a.w_off[bb] + (ts1 > 0 ? ts1 - 1 : 0);
        const int basec = base >= a.weather_rows ? a.weather_rows - 1 : (base < 0 ? 0 : base);
        const T* wrow = a.weather + (size_t)basec * a.nd;
        float wv[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) wv[j] = wrow[j];
        const float sday = o.start_day[bb];
        const float uo[NU] = {uBoil, uCo2, a.u[(size_t)2 * a.ld + bb], a.u[(size_t)3 * a.ld + bb], uLamp, a.u[(size_t)5 * a.ld + bb]};
        float f[OBS_NCORE];
#pragma unroll
        for (int j = 0; j < OBS_NCORE; ++j) {
            const int xi = j == 0 ? 0 : j == 1 ? 2 : j == 2 ? 15 : j == 3 ? 9 : j == 4 ? 21 : j == 5 ? 25 : 26;
            const float prim = j < 7 ? x1[xi] : (j < 13 ? uo[(j >= 7 && j < 13) ? j - 7 : 0] : wv[j < 18 ? j - 13 : 0]);
            const float aux = j < 13 ? x1[2] : wv[1];
            f[j] = obs_core_feature(j, prim, aux, sday, ts1, o.doy_inc, o.hod_inc);
        }
        const int n_live = min(WAVE, a.B - b0);
        const int nf = o.moff[5] >= 0 ? 5 * o.Np : 0;
        __syncthreads();                                    // the window buffer's last reader (del) is done
        for (int s0 = 0; s0 < n_live; s0 += OBS_ROWS) {     // wave-uniform
            const int nrows = min(OBS_ROWS, n_live - s0);
            const int r_me = lane - s0;
            if (r_me >= 0 && r_me < nrows) {
#pragma unroll
                for (int j = 0; j < OBS_NCORE; ++j) {
                    const int mo = o.moff[obs_core_module(j)];
                    if (mo >= 0) span[r_me * dim + mo + obs_core_col(j)] = f[j];
                }
            }
            // first weather row of each of the strip's windows, unclamped as in obs_kernel (rows past the last live one repeat it:
            // dead lanes shadow environment B - 1)
            int base_r[OBS_ROWS];
#pragma unroll
            for (int r = 0; r < OBS_ROWS; ++r) base_r[r] = __builtin_amdgcn_readlane(base, s0 + r);
            for (int q = lane; q < nf; q += WAVE) {
                const int i = q / 5, c = q - i * 5;
                float v[OBS_ROWS];
#pragma unroll
                for (int r = 0; r < OBS_ROWS; ++r) {
                    int row = base_r[r] + 1 + i;
                    row = row >= a.weather_rows ? a.weather_rows - 1 : (row < 0 ? 0 : row);
                    v[r] = (float)a.weather[(size_t)row * a.nd + c];
                }
#pragma unroll
                for (int r = 0; r < OBS_ROWS; ++r)
                    if (r < nrows) span[r * dim + o.moff[5] + q] = v[r];
            }
            __syncthreads();
            float* out = o.obs + (size_t)(b0 + s0) * dim;
            if (nrows == OBS_ROWS) {
                const int n4 = (OBS_ROWS * dim) >> 2;
                const v4f* src4 = reinterpret_cast<const v4f*>(span);
                v4f* dst4 = reinterpret_cast<v4f*>(out);
                for (int e = lane; e < n4; e += WAVE) __builtin_nontemporal_store(src4[e], &dst4[e]);
            } else {                                        // ragged tail of the batch: row-wise, as obs_kernel
                for (int r = 0; r < nrows; ++r)
                    for (int jj = lane; jj < dim; jj += WAVE) out[(size_t)r * dim + jj] = span[(size_t)r * dim + jj];
            }
            __syncthreads();
        }
        if constexpr (RST) {
            // ---- auto-reset epilogue (glgym_step_obs_reset): what reset_kernel over the mask `done` and obs_kernel in masked mode would do
            // behind this launch, for this wavefront's own finished environments.  One wave-uniform test; a wavefront without a finished
            // environment -- almost every wavefront of almost every step -- executes nothing else.  done, reward, info, step_flags and the
            // metrics stay as the step wrote them.
            const bool fin = live && term;
            const unsigned long long fin_mask = __builtin_amdgcn_ballot_w64(fin);
            if (fin_mask != 0) {
                const size_t row0 = (size_t)b0 * dim;
                __syncthreads();                            // (the strips' stores to obs, made by other lanes, are read back below)
                // (a) the finished rows as they stand, the terminal observations, to the same rows of term_obs; a row per pass
                if (o.term_obs) {
                    for (unsigned long long mk = fin_mask; mk != 0; mk &= mk - 1) {
                        const size_t e0 = row0 + (size_t)__builtin_ctzll(mk) * dim;
                        for (int jj = lane; jj < dim; jj += WAVE) o.term_obs[e0 + jj] = o.obs[e0 + jj];
                    }
                }
                __syncthreads();                            // all of them read before the first is overwritten
                // (b) the new episode: start draw, initial state, zero controls, timestep 0 (reset_env, reset_kernel's body)
                // (c) the row of the reset state: its 23 core features by the lane that owns the environment ...
                int base_new = 0;
                if (fin) {
                    reset_env<T>(b, a.ld, a.x, a.u, a.timestep, a.weather, a.weather_rows, o.w_off_rw, o.start_rows, o.start_days, o.n_starts,
                                 o.start_day_rw, o.episode, o.seed, a.nd);
                    base_new = o.w_off_rw[b];               // timestep 0: the window starts at the episode's first row
                    const int basen = base_new >= a.weather_rows ? a.weather_rows - 1 : (base_new < 0 ? 0 : base_new);
                    const T* wrown = a.weather + (size_t)basen * a.nd;
                    float wn[5];
#pragma unroll
                    for (int j = 0; j < 5; ++j) wn[j] = wrown[j];
                    const float sdayn = o.start_day_rw[b];
                    const float tAirn = a.x[(size_t)2 * a.ld + b];
                    float* orow = o.obs + row0 + (size_t)lane * dim;
#pragma unroll
                    for (int j = 0; j < OBS_NCORE; ++j) {
                        const int xi = j == 0 ? 0 : j == 1 ? 2 : j == 2 ? 15 : j == 3 ? 9 : j == 4 ? 21 : j == 5 ? 25 : 26;
                        const float prim = j < 7 ? a.x[(size_t)xi * a.ld + b] : (j < 13 ? 0.0f : wn[j < 18 ? j - 13 : 0]);
                        const float aux = j < 13 ? tAirn : wn[1];
                        const int mo = o.moff[obs_core_module(j)];
                        if (mo >= 0) orow[mo + obs_core_col(j)] = obs_core_feature(j, prim, aux, sdayn, 0, o.doy_inc, o.hod_inc);
                    }
                }
                // ... and its forecast block by the whole wavefront, a row per pass
                for (unsigned long long mk = fin_mask; mk != 0; mk &= mk - 1) {
                    const int r = __builtin_ctzll(mk);
                    const int base_r1 = __builtin_amdgcn_readlane(base_new, r);
                    float* orow = o.obs + row0 + (size_t)r * dim + o.moff[5];
                    for (int q = lane; q < nf; q += WAVE) {
                        const int i = q / 5, c = q - i * 5;
                        int row = base_r1 + 1 + i;
                        row = row >= a.weather_rows ? a.weather_rows - 1 : (row < 0 ? 0 : row);
                        orow[q] = (float)a.weather[(size_t)row * a.nd + c];
                    }
                }
            }
        }
    }
}


// ---------------------------------------------------------------------------------------------------
// fused env-step, FOUR LANES PER ENVIRONMENT (gl_model_quad.hpp): 16 environments per wavefront; for batches that leave SIMDs
// idle (B <= 16 384: profiles/r03_lanes_stage_proto.txt).  Same prologue / epilogue as step_kernel; lane 0 of a quad writes the
// per-env outputs, every lane the states it owns.
// ---------------------------------------------------------------------------------------------------
// SCH / CROP as in step_kernel: every scheme of the family, per-env crop blocks (config 5).  PIPE: ODE_pipe compiled in, selected at run
// time by a.pipe (gq_stage) -- in fp64 this kernel is the only step kernel (round 4: the one-lane fp64 kernels with their LDS mailbox
// and 2-3 KB of scratch are gone) and is always built with it.
// PAIR (round 6): TWO quads per environment run the verified ladder two rungs at a time (gl_model_quad.hpp rk4_delta_guarded_quad_pair, what
// glgym_evalF has done since round 5): for glgym_step(control = ...) -- step_raw_control, the rule-based controller: config 1 -- on batches
// that leave lanes free; the quad that holds the accepted attempt writes.  Bit-identical to the sequential ladder incl. step_flags.
template <class T, bool DEFAULT_P, int SCH = 0, bool PIPE = false, bool CROP = false, bool PAIR = false>
__global__ __launch_bounds__(WAVE) void step_kernel_quad(StepArgsT<T> a, ModelConst<T> m_arg, RewardConst<T> rw)
{
    static_assert(!(PAIR && CROP), "the two-rungs ladder is instantiated for shared crop constants only");
    // fp64: the handle's parameter block is staged in LDS as well (one uniform record per wavefront, broadcast reads behind the stage
    // fence): as a kernel argument its ~180 doubles live in SGPRs, of which there are 100 -- the compiler parks the rest in VGPR
    // lanes and pays two v_readlane per use (2 000 of the kernel's 20 000 static instructions)
    constexpr bool LDSM = sizeof(T) == 8 && !DEFAULT_P;
    __shared__ ModelConst<T> sh_m[1];
    if (LDSM) {
        static_assert(sizeof(ModelConst<T>) % 4 == 0, "word copy");
        const unsigned* src = reinterpret_cast<const unsigned*>(&m_arg);
        unsigned* dst = reinterpret_cast<unsigned*>(&sh_m[0]);
        for (int i = threadIdx.x; i < (int)(sizeof(ModelConst<T>) / 4); i += WAVE) dst[i] = src[i];
        __syncthreads();                       // one wavefront per block
    }
    const ModelConst<T>& m = LDSM ? sh_m[0] : DEFAULT_P ? device_default<T>() : m_arg;
    const int gl = blockIdx.x * WAVE + threadIdx.x, role = gl & 3;
    const int b = PAIR ? gl >> 3 : gl >> 2, half = PAIR ? (gl >> 2) & 1 : 0;
    const bool live = b < a.B;
    const int bb = live ? b : a.B - 1;        // out-of-range quads shadow the last env, stores are masked
    T u[NU];
    if (a.action) {
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            const float inc = a.action[(size_t)bb * NU + j] * a.du;               // f32 product, as tomato_env.py:113
            const T v = a.u[(size_t)j * a.ld + bb] + T(inc);
            u[j] = Math<T>::min(Math<T>::max(v, T(a.u_min[j])), T(a.u_max[j]));
        }
    } else {
#pragma unroll
        for (int j = 0; j < NU; ++j) u[j] = a.control[(size_t)j * a.ld + bb];
    }
    const int ts = a.timestep[bb];
    int row = a.w_off[bb] + ts;
    row = row < 0 ? 0 : (row >= a.weather_rows ? a.weather_rows - 1 : row);
    T d[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) d[j] = a.weather[(size_t)row * a.nd + j];
    // fp64: the coefficient blocks live in LDS (rk_delta_quad<LDSQ>): StepCoef (and the env's crop constants) once per quad, LaneK per
    // lane, records padded to an odd number of 8-byte words (conflict-free ds_read_b64 across the lanes)
    constexpr bool LDSQ = sizeof(T) == 8;
    struct SRec { StepCoef<T> s; T pad[(sizeof(StepCoef<T>) / sizeof(T)) % 2 == 0 ? 1 : 2]; };
    struct KRec { LaneK<T> k; T pad[(sizeof(LaneK<T>) / sizeof(T)) % 2 == 0 ? 1 : 2]; };
    struct CRec { CropConst<T> c; T pad[(sizeof(CropConst<T>) / sizeof(T)) % 2 == 0 ? 1 : 2]; };
    __shared__ SRec sh_s[LDSQ ? WAVE / 4 : 1];
    __shared__ KRec sh_k[LDSQ ? WAVE : 1];
    __shared__ CRec sh_c[(LDSQ && CROP) ? WAVE / 4 : 1];
    StepCoef<T> s_reg;
    LaneK<T> k_reg;
    CropConst<T> cr_reg;
    if (CROP && (!LDSQ || role == 0)) {
        T pc[NCROP];
#pragma unroll
        for (int i = 0; i < NCROP; ++i) pc[i] = a.crop_p[(size_t)i * a.ld + bb];
        make_crop_const<T, T>(pc, a.gasR, a.tCanMin, cr_reg);
    }
    if (!LDSQ || role == 0) {
        precompute(u, d, m, CROP ? cr_reg : m.crop, s_reg);
        if (PIPE && a.pipe) {                                                 // ode.hpp:184-189
            const T tPipe = a.weather[(size_t)row * a.nd + 10], swOff = a.weather[(size_t)row * a.nd + 12];
            s_reg.pipeTrack = ((tPipe < T(1)) || (swOff > T(0))) ? T(0) : T(1);
            s_reg.tPipeSet = tPipe;
            s_reg.pipeOde = T(1);
        }
    }
    if (LDSQ) {
        if (role == 0) { sh_s[threadIdx.x >> 2].s = s_reg; if (CROP) sh_c[threadIdx.x >> 2].c = cr_reg; }
        __syncthreads();                       // one wavefront per block: orders the LDS writes before the quad's reads
    }
    const CropConst<T>& cr = !CROP ? m.crop : LDSQ ? sh_c[threadIdx.x >> 2].c : cr_reg;
    const StepCoef<T>& s = LDSQ ? sh_s[threadIdx.x >> 2].s : s_reg;
    LaneK<T>& K = LDSQ ? sh_k[threadIdx.x].k : k_reg;
    // the lane's states, in the integrator's coordinates (screens / inner cover face as differences to their air node)
    auto X = [&](int i) { return a.x[(size_t)i * a.ld + bb]; };
    QVec<T> x0, z0, del;
#pragma unroll
    for (int i = 0; i < 6; ++i) x0.sh[i] = X(role == 0 ? gq_sh_ix(i) : role == 1 ? gq_sh_ix(i) : role == 2 ? gq_sh_ix(i) : gq_sh_ix(i));
    x0.p = gq_mk<T>(X(role == 0 ? 4 : role == 1 ? 8 : role == 2 ? 7 : 5), X(role == 0 ? 9 : role == 1 ? 17 : role == 2 ? 20 : 6));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ix = role == 0 ? gq_other_ix(0, j) : role == 1 ? gq_other_ix(1, j) : role == 2 ? gq_other_ix(2, j) : gq_other_ix(3, j < 2 ? j : 1);
        x0.o[j] = X(ix);
    }
    z0 = x0;
    z0.p = gq_mk<T>(role == 2 ? x0.sh[2] - x0.p.x : role == 3 ? x0.sh[3] - x0.p.x : x0.p.x,
                    role == 2 ? x0.sh[2] - x0.p.y : role == 3 ? x0.p.x - x0.p.y : x0.p.y);      // cover lane: w = tCovIn - tCovE
    if (live && role == 0 && half == 0) {
#pragma unroll
        for (int j = 0; j < NU; ++j) a.u[(size_t)j * a.ld + b] = u[j];
    }
    bool bad;
    int extra_steps = 0, first_flags = 0, retries = 0, mine = 1;
    constexpr bool HVU = sizeof(T) == 8 || DEFAULT_P;         // harvest_flow's wave-uniform exits: not where the parameters live in SGPRs (fp32, handle parameters)
    if (PAIR) {
        int bad_i;
        rk4_delta_guarded_quad_pair<T, gl_order(SCH), SchemeWin<T, SCH>::value, LDSQ, PIPE, false, true, HVU>(role, half, z0, s, K, m, cr, a.dt, a.n_sub, del, &bad_i, &mine,
                                                                                                         a.window, &retries, &extra_steps, &first_flags);
        asm volatile("" : "+v"(bad_i), "+v"(mine));
        bad = bad_i != 0;
    } else {
        retries = rk4_delta_guarded_quad<T, gl_order(SCH), SchemeWin<T, SCH>::value, LDSQ, PIPE, LDSQ && CROP, HVU>(role, z0, s, K, m, cr, a.dt, a.n_sub, del, &bad,
                                                                                                    &extra_steps, a.verify != 0, &first_flags, a.window);
    }
    // ---- new state: physical increments of what the lane owns.  Nothing but the integrator's own state is kept live across the
    // integrator (the fp64 build is at its register limit there): the old state and the applied control are read again
    P2<T> dP;
    gq_phys_pair<T>(role, del, dP);
    asm volatile("" ::: "memory");
    // (opaque copies of the env indices: the address arithmetic of the epilogue is redone here instead of being carried -- as spilled
    // 64-bit pointers -- across the integrator)
    int gl2 = blockIdx.x * WAVE + threadIdx.x;
    asm volatile("" : "+v"(gl2));
    const int role2 = gl2 & 3, b2 = PAIR ? gl2 >> 3 : gl2 >> 2;
    const bool live2 = b2 < a.B && mine != 0;             // (PAIR: the quad that holds the accepted attempt writes)
    const int bb2 = (b2 < a.B) ? b2 : a.B - 1;
    const int ts2 = a.timestep[bb2];
    auto X2 = [&](int i) { return a.x[(size_t)i * a.ld + bb2]; };
#pragma unroll
    for (int i = 0; i < 6; ++i) x0.sh[i] = X2(gq_sh_ix(i));
    x0.p = gq_mk<T>(X2(role2 == 0 ? 4 : role2 == 1 ? 8 : role2 == 2 ? 7 : 5), X2(role2 == 0 ? 9 : role2 == 1 ? 17 : role2 == 2 ? 20 : 6));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ix = role2 == 0 ? gq_other_ix(0, j) : role2 == 1 ? gq_other_ix(1, j) : role2 == 2 ? gq_other_ix(2, j) : gq_other_ix(3, j < 2 ? j : 1);
        x0.o[j] = X2(ix);
    }
#pragma unroll
    for (int j = 0; j < NU; ++j) u[j] = a.u[(size_t)j * a.ld + bb2];       // (written above by lane 0 of the quad)
    QVec<T> x1;
    x1.p = gq_mk<T>(bad ? x0.p.x : x0.p.x + dP.x, bad ? x0.p.y : x0.p.y + dP.y);
#pragma unroll
    for (int i = 0; i < 6; ++i) x1.sh[i] = bad ? x0.sh[i] : x0.sh[i] + del.sh[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) x1.o[j] = bad ? x0.o[j] : x0.o[j] + del.o[j];
    if (role2 == 3) {    // x27 = time [days since reset]: exact from the step counter (step_kernel)
        const double per_step = (double)a.dt / 86400.0;
        double t_start = (double)x0.o[1] - (double)ts2 * per_step;
        if (fabs(t_start) < 5e-4) t_start = 0.0;
        if (!bad) x1.o[1] = T(t_start + ((double)ts2 + 1.0) * per_step);
    }
    const T dFruit = gq_bcast<2>(del.o[3]);                 // cFruit lives on lane 2
    // ---- reward epilogue (step_kernel): every lane has what it needs, lane 0 writes
    const T co2ppm = rw.kPpm * (x1.sh[2] + T(273.15)) * x1.sh[0];
    const T rh = Math<T>::min(Math<T>::max(T(100) * x1.sh[4] / sat_vp_exact(x1.sh[2]), T(0)), T(100));
    const T o3[3] = {co2ppm, x1.sh[2], rh};
    T viol[3], pen = T(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        viol[i] = Math<T>::max(rw.lo[i] - o3[i], T(0)) + Math<T>::max(o3[i] - rw.hi[i], T(0));
        pen += viol[i] * rw.invMaxViol[i];
    }
    const T heat = u[0] * rw.heatK, elec = u[4] * rw.elecK, co2c = u[1] * rw.co2K;
    const T varc = heat + co2c + elec;
    const T gains = (bad ? T(0) : dFruit) * rw.gainK;
    const T profit = gains - varc;
    const T reward = (profit - rw.minProfit) * rw.invRange - pen;
    const bool term = bad || (ts2 >= a.N);
    if (live2) {
        auto W = [&](int i, T v) { a.x[(size_t)i * a.ld + b2] = v; };
        W(role2 == 0 ? 4 : role2 == 1 ? 8 : role2 == 2 ? 7 : 5, x1.p.x);
        W(role2 == 0 ? 9 : role2 == 1 ? 17 : role2 == 2 ? 20 : 6, x1.p.y);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (role2 != 3 || j < 2) W(role2 == 0 ? gq_other_ix(0, j) : role2 == 1 ? gq_other_ix(1, j) : role2 == 2 ? gq_other_ix(2, j) : gq_other_ix(3, j < 2 ? j : 1), x1.o[j]);
        if (role2 == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) W(gq_sh_ix(i), x1.sh[i]);
            a.timestep[b2] = ts2 + 1;
            a.reward[b2] = reward;
            a.done[b2] = term ? 1 : 0;
            if (a.step_flags) a.step_flags[b2] = first_flags | (retries << 8) | (bad ? GLGYM_SF_FAILED : 0) | (min(extra_steps, 32767) << 16);
            if (a.info) {
                const T inf[GLGYM_NINFO] = {profit, gains, varc, rw.fixedCosts, co2c, heat, elec, viol[1], viol[0], viol[2], T(0)};
#pragma unroll
                for (int i = 0; i < GLGYM_NINFO; ++i) a.info[(size_t)i * a.ld + b2] = inf[i];
            }
        }
    }
    if (a.metrics) {
        const bool cnt = live2 && role2 == 0;
        const float w = cnt ? 1.f : 0.f;
        float mv[GLGYM_NMETRIC] = {w * (float)reward, w * (float)profit, (cnt && term) ? 1.f : 0.f,
                                   (cnt && bad) ? 1.f : 0.f, w * (float)viol[0], w * (float)viol[1],
                                   w * (float)viol[2], w, w * (float)retries, w * (float)extra_steps,
                                   (cnt && (first_flags & SC_FLAG_ERR)) ? 1.f : 0.f, (cnt && (first_flags & SC_FLAG_BRANCH)) ? 1.f : 0.f,
                                   (cnt && (first_flags & (SC_FLAG_CAP | SC_FLAG_NONFINITE))) ? 1.f : 0.f,
                                   (cnt && (first_flags & 16)) ? 1.f : 0.f};
        float* mrep = a.metrics + (size_t)(blockIdx.x % GLGYM_METRIC_REPLICAS) * GLGYM_METRIC_STRIDE;
#pragma unroll
        for (int i = 0; i < GLGYM_NMETRIC; ++i) {
            const float sum = wave_sum(mv[i]);
            if (threadIdx.x == 0) atomicAdd(mrep + i, sum);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// reference-compatible step map, four lanes per row (what fp64 handles run: row-major double I/O, per-row crop blocks)
// ---------------------------------------------------------------------------------------------------
// PAIR (round 5): two quads per row, the verified ladder two rungs at a time (gl_model_quad.hpp rk4_delta_guarded_quad_pair) -- what
// glgym_evalF launches in verified mode while the batch leaves lanes free; bit-identical results, two thirds of the latency
template <class T, int SCH, bool PIPE, bool CROP, bool PAIR = false>
__global__ __launch_bounds__(WAVE) void evalf_kernel_quad(const double* x, const double* u, const double* d, const double* crop, int B, T dt,
                                                          int n_sub, T gasR, T tCanMin, ModelConst<T> m_arg, double* x_next, int nd,
                                                          int* n_failed, int verify, int pipe, int window)
{
    constexpr bool LDSM = sizeof(T) == 8;      // the parameter block in LDS (step_kernel_quad)
    __shared__ ModelConst<T> sh_m[1];
    if (LDSM) {
        const unsigned* src = reinterpret_cast<const unsigned*>(&m_arg);
        unsigned* dst = reinterpret_cast<unsigned*>(&sh_m[0]);
        for (int i = threadIdx.x; i < (int)(sizeof(ModelConst<T>) / 4); i += WAVE) dst[i] = src[i];
        __syncthreads();
    }
    const ModelConst<T>& m = LDSM ? sh_m[0] : m_arg;
    const int gl = blockIdx.x * WAVE + threadIdx.x, role = gl & 3, b = PAIR ? gl >> 3 : gl >> 2, half = PAIR ? (gl >> 2) & 1 : 0;
    const bool live = b < B;
    const int bb = live ? b : B - 1;
    T uu[NU], dd[7];
#pragma unroll
    for (int i = 0; i < NU; ++i) uu[i] = T(u[(size_t)bb * NU + i]);
#pragma unroll
    for (int i = 0; i < 7; ++i) dd[i] = T(d[(size_t)bb * nd + i]);
    constexpr bool LDSQ = sizeof(T) == 8;
    struct SRec { StepCoef<T> s; T pad[(sizeof(StepCoef<T>) / sizeof(T)) % 2 == 0 ? 1 : 2]; };
    struct KRec { LaneK<T> k; T pad[(sizeof(LaneK<T>) / sizeof(T)) % 2 == 0 ? 1 : 2]; };
    struct CRec { CropConst<T> c; T pad[(sizeof(CropConst<T>) / sizeof(T)) % 2 == 0 ? 1 : 2]; };
    __shared__ SRec sh_s[LDSQ ? WAVE / 4 : 1];
    __shared__ KRec sh_k[LDSQ ? WAVE : 1];
    __shared__ CRec sh_c[(LDSQ && CROP) ? WAVE / 4 : 1];
    StepCoef<T> s_reg;
    LaneK<T> k_reg;
    CropConst<T> cr_reg;
    if (CROP && (!LDSQ || role == 0)) {
        T pc[NCROP];
#pragma unroll
        for (int i = 0; i < NCROP; ++i) pc[i] = T(crop[(size_t)bb * NCROP + i]);
        make_crop_const<T, T>(pc, gasR, tCanMin, cr_reg);
    }
    if (!LDSQ || role == 0) {
        precompute(uu, dd, m, CROP ? cr_reg : m.crop, s_reg);
        if (PIPE && pipe) {
            const T tPipe = T(d[(size_t)bb * nd + 10]), swOff = T(d[(size_t)bb * nd + 12]);
            s_reg.pipeTrack = ((tPipe < T(1)) || (swOff > T(0))) ? T(0) : T(1);
            s_reg.tPipeSet = tPipe;
            s_reg.pipeOde = T(1);
        }
    }
    if (LDSQ) {
        if (role == 0) { sh_s[threadIdx.x >> 2].s = s_reg; if (CROP) sh_c[threadIdx.x >> 2].c = cr_reg; }
        __syncthreads();
    }
    const CropConst<T>& cr = !CROP ? m.crop : LDSQ ? sh_c[threadIdx.x >> 2].c : cr_reg;
    const StepCoef<T>& s = LDSQ ? sh_s[threadIdx.x >> 2].s : s_reg;
    LaneK<T>& K = LDSQ ? sh_k[threadIdx.x].k : k_reg;
    auto X = [&](int i) { return T(x[(size_t)bb * NX + i]); };
    QVec<T> x0, z0, del;
#pragma unroll
    for (int i = 0; i < 6; ++i) x0.sh[i] = X(gq_sh_ix(i));
    x0.p = gq_mk<T>(X(role == 0 ? 4 : role == 1 ? 8 : role == 2 ? 7 : 5), X(role == 0 ? 9 : role == 1 ? 17 : role == 2 ? 20 : 6));
#pragma unroll
    for (int j = 0; j < 4; ++j)
        x0.o[j] = X(role == 0 ? gq_other_ix(0, j) : role == 1 ? gq_other_ix(1, j) : role == 2 ? gq_other_ix(2, j) : gq_other_ix(3, j < 2 ? j : 1));
    z0 = x0;
    z0.p = gq_mk<T>(role == 2 ? x0.sh[2] - x0.p.x : role == 3 ? x0.sh[3] - x0.p.x : x0.p.x,
                    role == 2 ? x0.sh[2] - x0.p.y : role == 3 ? x0.p.x - x0.p.y : x0.p.y);
    bool bad;
    constexpr bool HVU = sizeof(T) == 8;       // fp32 rows carry their parameters in SGPRs: harvest_flow per lane (gl_model.hpp)
    int mine = 1;                        // (an integer on purpose: rk4_delta_guarded_quad_pair)
    if (PAIR) {
        int bad_i;
        rk4_delta_guarded_quad_pair<T, gl_order(SCH), SchemeWin<T, SCH>::value, LDSQ, PIPE, LDSQ && CROP, false, HVU>(role, half, z0, s, K, m, cr, dt, n_sub, del, &bad_i, &mine, window);
        asm volatile("" : "+v"(bad_i), "+v"(mine));
        bad = bad_i != 0;
    } else {
        int extra_steps, first_flags = 0;
        rk4_delta_guarded_quad<T, gl_order(SCH), SchemeWin<T, SCH>::value, LDSQ, PIPE, LDSQ && CROP, HVU>(role, z0, s, K, m, cr, dt, n_sub, del, &bad, &extra_steps, verify != 0,
                                                                                      &first_flags, window);
    }
    // a failed integration (the reference's evalF raises): the row is NaN and the call returns GLGYM_EODE
    P2<T> dP;
    gq_phys_pair<T>(role, del, dP);
    asm volatile("" ::: "memory");
    int gl2 = blockIdx.x * WAVE + threadIdx.x;
    asm volatile("" : "+v"(gl2));
    const int role2 = gl2 & 3, b2 = PAIR ? gl2 >> 3 : gl2 >> 2;
    if (b2 < B && mine != 0) {
        const double nan = __builtin_nan("");
        auto X2 = [&](int i) { return x[(size_t)b2 * NX + i]; };
        auto W = [&](int i, T dv) { x_next[(size_t)b2 * NX + i] = bad ? nan : X2(i) + (double)dv; };
        W(role2 == 0 ? 4 : role2 == 1 ? 8 : role2 == 2 ? 7 : 5, dP.x);
        W(role2 == 0 ? 9 : role2 == 1 ? 17 : role2 == 2 ? 20 : 6, dP.y);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (role2 != 3 || j < 2)
                W(role2 == 0 ? gq_other_ix(0, j) : role2 == 1 ? gq_other_ix(1, j) : role2 == 2 ? gq_other_ix(2, j) : gq_other_ix(3, j < 2 ? j : 1), del.o[j]);
        if (role2 == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) W(gq_sh_ix(i), del.sh[i]);
            if (bad) atomicAdd(n_failed, 1);
        }
    }
}

// the reference's right-hand side at one state per row (test hook behind glgym_rhs)
template <class T, bool PER_ENV_CROP, bool PIPE>
__global__ __launch_bounds__(WAVE) void rhs_kernel(const double* x, const double* u, const double* d, const double* crop, int B, T gasR,
                                                   T tCanMin, ModelConst<T> m, double* dx, int nd)
{
    const int b = blockIdx.x * WAVE + threadIdx.x;
    if (b >= B) return;
    T x0[NX], uu[NU], dd[7];
    for (int i = 0; i < NX; ++i) x0[i] = T(x[(size_t)b * NX + i]);
    for (int i = 0; i < NU; ++i) uu[i] = T(u[(size_t)b * NU + i]);
    for (int i = 0; i < 7; ++i) dd[i] = T(d[(size_t)b * nd + i]);
    CropConst<T> crLocal;
    if (PER_ENV_CROP) {
        T pc[NCROP];
        for (int i = 0; i < NCROP; ++i) pc[i] = T(crop[(size_t)b * NCROP + i]);
        make_crop_const<T, T>(pc, gasR, tCanMin, crLocal);
    }
    const CropConst<T>& cr = PER_ENV_CROP ? crLocal : m.crop;
    StepCoef<T> s;
    precompute(uu, dd, m, cr, s);
    if (PIPE) {
        const T tPipe = T(d[(size_t)b * nd + 10]), swOff = T(d[(size_t)b * nd + 12]);
        s.pipeTrack = ((tPipe < T(1)) || (swOff > T(0))) ? T(0) : T(1);
        s.tPipeSet = tPipe;
    }
    T k[NX];
    rhs<T, true, PIPE>(x0, s, m, cr, k);
    for (int i = 0; i < NX; ++i) dx[(size_t)b * NX + i] = (double)k[i];
}

// ---------------------------------------------------------------------------------------------------
// reference-compatible step map / RHS with row-major double I/O (B small; B = 1 for the drop-in evalF)
// ---------------------------------------------------------------------------------------------------
template <class T, bool PER_ENV_CROP, bool PIPE = false, int SCH = 0>
__global__ __launch_bounds__(WAVE) void evalf_kernel(const double* x, const double* u, const double* d,
                                                     const double* crop, int B, T dt, int n_sub, T gasR, T tCanMin,
                                                     ModelConst<T> m, double* x_next, int rhs_only, int nd,
                                                     int* n_failed, int verify, int window)
{
    const int b = blockIdx.x * WAVE + threadIdx.x;
    if (b >= B) return;
    T x0[NX], uu[NU], dd[7];
    for (int i = 0; i < NX; ++i) x0[i] = T(x[(size_t)b * NX + i]);
    for (int i = 0; i < NU; ++i) uu[i] = T(u[(size_t)b * NU + i]);
    for (int i = 0; i < 7; ++i) dd[i] = T(d[(size_t)b * nd + i]);
    CropConst<T> crLocal;
    if (PER_ENV_CROP) {
        T pc[NCROP];
        for (int i = 0; i < NCROP; ++i) pc[i] = T(crop[(size_t)b * NCROP + i]);
        make_crop_const<T, T>(pc, gasR, tCanMin, crLocal);
    }
    const CropConst<T>& cr = PER_ENV_CROP ? crLocal : m.crop;
    StepCoef<T> s;
    precompute(uu, dd, m, cr, s);
    if (PIPE) {
        const T tPipe = T(d[(size_t)b * nd + 10]), swOff = T(d[(size_t)b * nd + 12]);
        s.pipeTrack = ((tPipe < T(1)) || (swOff > T(0))) ? T(0) : T(1);
        s.tPipeSet = tPipe;
    }
    if (rhs_only) {
        T k[NX];
        rhs<T, true, PIPE>(x0, s, m, cr, k);
        for (int i = 0; i < NX; ++i) x_next[(size_t)b * NX + i] = (double)k[i];
        return;
    }
    T del[NX];
    bool failed;
    rk4_delta_guarded<T, PIPE, gl_order(SCH), SchemeWin<T, SCH>::value>(x0, s, m, cr, dt, n_sub, del, &failed, nullptr, verify != 0, nullptr, window);
    // a failed integration (the reference's evalF raises): the row is NaN and the call returns GLGYM_EODE
    for (int i = 0; i < NX; ++i)
        x_next[(size_t)b * NX + i] = failed ? __builtin_nan("") : (double)x0[i] + (double)del[i];
    if (failed) atomicAdd(n_failed, 1);
}

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

// ---------------------------------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------------------------------
struct glgym_handle_s {
    int device = 0;
    int dtype = GLGYM_F32;
    int n_sub = 256;
    double dt = 900.0;
    double p[NP];
    ModelConst<float> mf;
    ModelConst<double> md;
    glgym_reward_cfg rcfg;
    RewardConst<float> rf;
    RewardConst<double> rd;
    double max_profit = 0, min_profit = 0, fixed_costs = 0;
    float* p0_crop_dev = nullptr;       // shared p[128..161] as f32 (noise kernel input)
    int* fail_dev = nullptr;            // glgym_evalF: number of rows whose integration failed
    int nd = ND;                        // weather / disturbance row stride: 10, or up to 16 (ODE_pipe reads columns 10, 12)
    int variant = GLGYM_ODE;            // GLGYM_ODE | GLGYM_ODE_PIPE
    int scheme = GLGYM_SCHEME_RK4;      // GLGYM_SCHEME_RK4 | GLGYM_SCHEME_RK2 | GLGYM_SCHEME_RK3
    int verify_mode = GLGYM_VERIFY_AUTO;   // glgym_set_verify
    int use_specialised = 1;            // GLGYM_GENERIC=1 in the environment forces the generic kernels (A/B tests)
    int window = 0;                     // glgym_set_window: 0 = the scheme's own
    int layout = GLGYM_LAYOUT_AUTO;     // glgym_set_layout (fp32); initial value from GLGYM_LAYOUT at glgym_create
    int occupancy = 0;                  // glgym_set_occupancy (one-lane fp32 kernel): 0 = by batch size; initial value from GLGYM_OCC at glgym_create
    int ladder_parallel = 1;            // glgym_set_ladder_parallel: verified glgym_evalF calls may run two rungs of the ladder side by side
    int n_simd = 1024;                  // SIMDs of the device (4 per CU)
    float du = 0.1f, u_min[NU] = {0, 0, 0, 0, 0, 0}, u_max[NU] = {1, 1, 1, 1, 1, 1};   // glgym_set_control_limits
    int obs_modules[6] = {0, 1, 2, 3, 4, 5};   // observation modules in output order (glgym_set_obs_modules)
    int n_obs_modules = 6;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // glgym_evalF's integrator (glgym_set_integrator / glgym_set_tolerances) and the per-row statistics of its last BDF call
    int integrator = GLGYM_INTEGRATOR_EXPLICIT;
    int step_integrator = GLGYM_INTEGRATOR_EXPLICIT;     // glgym_step's (glgym_set_step_integrator); the tolerances are shared
    double rtol = 1e-6, atol = 1e-6;
    int max_steps = 10000;
    int32_t* stats_dev = nullptr;
    int stats_cap = 0;
    std::vector<int32_t> stats;         // [stats_rows][GLGYM_NSOLVER_STAT]
    int stats_rows = 0;
    // scratch for the host-pointer entry points
    double* scratch = nullptr;
    size_t scratch_elems = 0;
};

static void default_reward(glgym_reward_cfg& c)
{
    c.elec_price = 0.3; c.heating_price = 0.09; c.co2_price = 0.3; c.fruit_price = 1.6; c.dmfm = 0.065;
    c.fixed_greenhouse_cost = 15.0; c.fixed_co2_cost = 0.015; c.fixed_lamp_cost = 0.07; c.fixed_screen_cost = 2.0;
    c.pen_lamp = 0.1;
    c.co2_min = 300; c.co2_max = 1600; c.temp_min = 15; c.temp_max = 34; c.rh_min = 50; c.rh_max = 85;
}

static int refresh(glgym_handle h)
{
    std::memset(&h->mf, 0, sizeof h->mf);
    std::memset(&h->md, 0, sizeof h->md);
    make_model_const<float>(h->p, h->mf);
    make_model_const<double>(h->p, h->md);
    make_reward_const<float>(h->p, h->dt, h->rcfg, h->rf, &h->max_profit, &h->min_profit, &h->fixed_costs);
    make_reward_const<double>(h->p, h->dt, h->rcfg, h->rd, nullptr, nullptr, nullptr);
    float pc[NCROP];
    for (int i = 0; i < NCROP; ++i) pc[i] = (float)h->p[CROP0 + i];
    HIPCHK(hipMemcpy(h->p0_crop_dev, pc, sizeof pc, hipMemcpyHostToDevice));
    return GLGYM_OK;
}

// The device-pointer entry points launch on the CALLER's stream; HIP wants the calling thread's current device to be the stream's.
// One process per GPU (the layout this library is built for) never notices; a process that holds handles on several devices does:
// bind the handle's device for the duration of the call and put the caller's back (a no-op when it already is current).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    // a null handle binds nothing (the entry point then returns GLGYM_EINVAL without having created a context on any device)
    explicit DeviceGuard(const glgym_handle_s* h)
    {
        if (h && hipGetDevice(&prev) == hipSuccess && prev != h->device) switched = hipSetDevice(h->device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

extern "C" {

#define GLGYM_STR_(v) #v
#define GLGYM_STR(v) GLGYM_STR_(v)
const char* glgym_version(void)
{
    return "glgym 0.7 (gfx950; ABI " GLGYM_STR(GLGYM_ABI_VERSION) "; stability-controlled, step-doubling-verified sub-steppers in delta form: "
           "five-stage fourth-order 2N scheme / RK4 / RK3 / midpoint; adaptive variable-order BDF for glgym_evalF)";
}
int glgym_abi_version(void) { return GLGYM_ABI_VERSION; }
const char* glgym_last_error(void) { return g_err.c_str(); }

int glgym_destroy(glgym_handle h);

int glgym_create(int nx, int nu, int nd, int np, double dt, const double* p, int dtype, int n_sub, int device,
                 glgym_handle* out)
{
    if (!out || !p || nx != NX || nu != NU || nd < ND || nd > 16 || np != NP || !(dt > 0) || n_sub < 1 ||
        (dtype != GLGYM_F32 && dtype != GLGYM_F64)) {
        g_err = "glgym_create: expected nx=28 nu=6 nd=10..16 np=208, dt>0, n_sub>=1, dtype in {F32,F64}";
        return GLGYM_EINVAL;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0 || device < 0 || device >= n_dev) {
        g_err = "glgym_create: no usable HIP device (this library has no CPU fallback)";
        return GLGYM_ENODEV;
    }
    HIPCHK(hipSetDevice(device));
    glgym_handle h = new (std::nothrow) glgym_handle_s();
    if (!h) return GLGYM_ENOMEM;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            h->n_simd = 4 * prop.multiProcessorCount;
    }
    h->device = device; h->dtype = dtype; h->n_sub = n_sub; h->dt = dt; h->nd = nd;
    std::memcpy(h->p, p, sizeof h->p);
    default_reward(h->rcfg);
    if (const char* e = std::getenv("GLGYM_GENERIC")) h->use_specialised = (e[0] == '1') ? 0 : 1;
    if (const char* e = std::getenv("GLGYM_VERIFY"))          // default of glgym_set_verify: auto | always | never (A/B tests)
        h->verify_mode = (e[0] == 'n') ? GLGYM_VERIFY_NEVER : (e[0] == 'a' && e[1] == 'l') ? GLGYM_VERIFY_ALWAYS : GLGYM_VERIFY_AUTO;
    // initial values of glgym_set_layout / glgym_set_occupancy, read ONCE here (A/B tools set them before creating their handle); the
    // launch path reads handle state only
    if (const char* e = std::getenv("GLGYM_LAYOUT")) h->layout = (e[0] == 'q') ? GLGYM_LAYOUT_QUAD : (e[0] == 'o') ? GLGYM_LAYOUT_ONE : GLGYM_LAYOUT_AUTO;
    if (const char* e = std::getenv("GLGYM_OCC")) h->occupancy = (std::atoi(e) == 2) ? 2 : (std::atoi(e) == 1) ? 1 : 0;
    // from here on a failure must release what was acquired: run the steps through one exit point
    int rc = [&]() -> int {
        HIPCHK(hipMalloc(&h->p0_crop_dev, NCROP * sizeof(float)));
        HIPCHK(hipMalloc(&h->fail_dev, sizeof(int)));
        HIPCHK(hipEventCreate(&h->ev0));
        HIPCHK(hipEventCreate(&h->ev1));
        return refresh(h);
    }();
    if (rc != GLGYM_OK) {
        const std::string keep = g_err;
        (void)glgym_destroy(h);
        g_err = keep;
        return rc;
    }
    *out = h;
    return GLGYM_OK;
}

int glgym_destroy(glgym_handle h)
{
    if (!h) return GLGYM_EINVAL;
    (void)hipSetDevice(h->device);
    if (h->p0_crop_dev) (void)hipFree(h->p0_crop_dev);
    if (h->fail_dev) (void)hipFree(h->fail_dev);
    if (h->scratch) (void)hipFree(h->scratch);
    if (h->stats_dev) (void)hipFree(h->stats_dev);
    if (h->ev0) (void)hipEventDestroy(h->ev0);
    if (h->ev1) (void)hipEventDestroy(h->ev1);
    delete h;
    return GLGYM_OK;
}

int glgym_set_params(glgym_handle h, const double* p)
{
    if (!h || !p) return GLGYM_EINVAL;
    std::memcpy(h->p, p, sizeof h->p);
    return refresh(h);
}

int glgym_set_params_keep_reward_scale(glgym_handle h, const double* p)
{
    if (!h || !p) return GLGYM_EINVAL;
    const float minf = h->rf.minProfit, invf = h->rf.invRange;
    const double mind = h->rd.minProfit, invd = h->rd.invRange, maxp = h->max_profit, minp = h->min_profit;
    std::memcpy(h->p, p, sizeof h->p);
    const int rc = refresh(h);
    h->rf.minProfit = minf; h->rf.invRange = invf;
    h->rd.minProfit = mind; h->rd.invRange = invd;
    h->max_profit = maxp; h->min_profit = minp;
    return rc;
}

int glgym_set_model_variant(glgym_handle h, int variant)
{
    if (!h || (variant != GLGYM_ODE && variant != GLGYM_ODE_PIPE) || (variant == GLGYM_ODE_PIPE && h->nd < 14)) {
        g_err = "glgym_set_model_variant: GLGYM_ODE or GLGYM_ODE_PIPE (the latter needs a handle created with nd >= 14)";
        return GLGYM_EINVAL;
    }
    h->variant = variant;
    return GLGYM_OK;
}

int glgym_set_scheme(glgym_handle h, int scheme)
{
    if (!h || (scheme != GLGYM_SCHEME_RK4 && scheme != GLGYM_SCHEME_RK2 && scheme != GLGYM_SCHEME_RK3 && scheme != GLGYM_SCHEME_LS5)) {
        g_err = "glgym_set_scheme: GLGYM_SCHEME_RK4, GLGYM_SCHEME_RK2, GLGYM_SCHEME_RK3 or GLGYM_SCHEME_LS5";
        return GLGYM_EINVAL;
    }
    h->scheme = scheme;
    return GLGYM_OK;
}

int glgym_set_window(glgym_handle h, int window)
{
    if (!h || window < 0 || window > 8) { g_err = "glgym_set_window: 0 (the scheme's own) or 1..8 nominal sub-steps per window"; return GLGYM_EINVAL; }
    h->window = window;
    return GLGYM_OK;
}

int glgym_set_layout(glgym_handle h, int layout)
{
    if (!h || (layout != GLGYM_LAYOUT_AUTO && layout != GLGYM_LAYOUT_ONE && layout != GLGYM_LAYOUT_QUAD)) {
        g_err = "glgym_set_layout: GLGYM_LAYOUT_AUTO, GLGYM_LAYOUT_ONE or GLGYM_LAYOUT_QUAD";
        return GLGYM_EINVAL;
    }
    h->layout = layout;
    return GLGYM_OK;
}

int glgym_set_occupancy(glgym_handle h, int waves_per_simd)
{
    if (!h || waves_per_simd < 0 || waves_per_simd > 2) { g_err = "glgym_set_occupancy: 0 (by batch size), 1 or 2 waves per SIMD"; return GLGYM_EINVAL; }
    h->occupancy = waves_per_simd;
    return GLGYM_OK;
}

int glgym_set_ladder_parallel(glgym_handle h, int on)
{
    if (!h || (on != 0 && on != 1)) { g_err = "glgym_set_ladder_parallel: 0 or 1"; return GLGYM_EINVAL; }
    h->ladder_parallel = on;
    return GLGYM_OK;
}

int glgym_set_control_limits(glgym_handle h, const double* u_min, const double* u_max, double delta_u_max)
{
    if (!h || !u_min || !u_max || !(delta_u_max >= 0)) { g_err = "glgym_set_control_limits: bad arguments"; return GLGYM_EINVAL; }
    for (int j = 0; j < NU; ++j)
        if (!(u_min[j] <= u_max[j])) { g_err = "glgym_set_control_limits: u_min > u_max"; return GLGYM_EINVAL; }
    for (int j = 0; j < NU; ++j) { h->u_min[j] = (float)u_min[j]; h->u_max[j] = (float)u_max[j]; }    // float32 arrays,
    h->du = (float)delta_u_max;                                                                       // base_env.py:72-74
    return GLGYM_OK;
}

int glgym_set_integrator(glgym_handle h, int integrator)
{
    if (!h || (integrator != GLGYM_INTEGRATOR_EXPLICIT && integrator != GLGYM_INTEGRATOR_BDF)) {
        g_err = "glgym_set_integrator: GLGYM_INTEGRATOR_EXPLICIT or GLGYM_INTEGRATOR_BDF";
        return GLGYM_EINVAL;
    }
    h->integrator = integrator;
    return GLGYM_OK;
}

int glgym_set_step_integrator(glgym_handle h, int integrator)
{
    if (!h || (integrator != GLGYM_INTEGRATOR_EXPLICIT && integrator != GLGYM_INTEGRATOR_BDF)) {
        g_err = "glgym_set_step_integrator: GLGYM_INTEGRATOR_EXPLICIT or GLGYM_INTEGRATOR_BDF";
        return GLGYM_EINVAL;
    }
    h->step_integrator = integrator;
    return GLGYM_OK;
}

int glgym_set_tolerances(glgym_handle h, double rtol, double atol, int max_steps)
{
    if (!h || !(rtol > 0.0) || !(atol > 0.0) || !std::isfinite(rtol) || !std::isfinite(atol) || max_steps < 1) {
        g_err = "glgym_set_tolerances: rtol > 0, atol > 0 (finite), max_steps >= 1";
        return GLGYM_EINVAL;
    }
    h->rtol = rtol; h->atol = atol; h->max_steps = max_steps;
    return GLGYM_OK;
}

int glgym_get_solver_stats(glgym_handle h, int B, int32_t* stats)
{
    if (!h || !stats || B < 1 || B != h->stats_rows) {
        g_err = "glgym_get_solver_stats: B must be the batch size of the last glgym_evalF with GLGYM_INTEGRATOR_BDF";
        return GLGYM_EINVAL;
    }
    std::memcpy(stats, h->stats.data(), (size_t)B * GLGYM_NSOLVER_STAT * sizeof(int32_t));
    return GLGYM_OK;
}

int glgym_set_verify(glgym_handle h, int mode)
{
    if (!h || (mode != GLGYM_VERIFY_AUTO && mode != GLGYM_VERIFY_ALWAYS && mode != GLGYM_VERIFY_NEVER)) {
        g_err = "glgym_set_verify: GLGYM_VERIFY_AUTO, GLGYM_VERIFY_ALWAYS or GLGYM_VERIFY_NEVER";
        return GLGYM_EINVAL;
    }
    h->verify_mode = mode;
    return GLGYM_OK;
}

int glgym_set_n_sub(glgym_handle h, int n_sub)
{
    if (!h || n_sub < 1) return GLGYM_EINVAL;
    h->n_sub = n_sub;
    return GLGYM_OK;
}

int glgym_set_reward(glgym_handle h, const glgym_reward_cfg* cfg)
{
    if (!h || !cfg) return GLGYM_EINVAL;
    h->rcfg = *cfg;
    return refresh(h);
}

int glgym_get_reward_scale(glgym_handle h, double* max_profit, double* min_profit, double* fixed_costs)
{
    if (!h) return GLGYM_EINVAL;
    if (max_profit) *max_profit = h->max_profit;
    if (min_profit) *min_profit = h->min_profit;
    if (fixed_costs) *fixed_costs = h->fixed_costs;
    return GLGYM_OK;
}

}  // extern "C"

// ---- host-pointer entry points --------------------------------------------------------------------
static int ensure_scratch(glgym_handle h, size_t elems)
{
    if (h->scratch_elems >= elems) return GLGYM_OK;
    if (h->scratch) (void)hipFree(h->scratch);
    h->scratch = nullptr; h->scratch_elems = 0;
    HIPCHK(hipMalloc(&h->scratch, elems * sizeof(double)));
    h->scratch_elems = elems;
    return GLGYM_OK;
}

// the run-time scheme as a compile-time constant: f(std::integral_constant<int, GLGYM_SCHEME_*>)
template <class F> static void with_scheme(int scheme, F&& f)
{
    if (scheme == GLGYM_SCHEME_RK2) f(std::integral_constant<int, GLGYM_SCHEME_RK2>{});
    else if (scheme == GLGYM_SCHEME_RK3) f(std::integral_constant<int, GLGYM_SCHEME_RK3>{});
    else if (scheme == GLGYM_SCHEME_LS5) f(std::integral_constant<int, GLGYM_SCHEME_LS5>{});
    else f(std::integral_constant<int, GLGYM_SCHEME_RK4>{});
}

template <class T, int SCH>
static void launch_evalf_sch(glgym_handle h, const ModelConst<T>& m, const double* p_used, const double* dx, const double* du,
                             const double* dd, const double* dcrop, int B, double* dout)
{
    const int verify = h->verify_mode != GLGYM_VERIFY_NEVER;
    const int pipe = h->variant == GLGYM_ODE_PIPE ? 1 : 0;
    const dim3 grid((B + WAVE - 1) / WAVE), qgrid((4 * B + WAVE - 1) / WAVE), pgrid((8 * B + WAVE - 1) / WAVE), block(WAVE);
    const auto go = [&](auto kernel, dim3 g, auto... tail) {
        hipLaunchKernelGGL(kernel, g, block, 0, (hipStream_t)0, dx, du, dd, dcrop, B, T(h->dt), h->n_sub, T(p_used[39]), T(p_used[162]), m,
                           dout, tail...);
    };
    const auto one = [&](auto kernel) { go(kernel, grid, 0, h->nd, h->fail_dev, verify, h->window); };
    const auto quad = [&](auto kernel, dim3 g) { go(kernel, g, h->nd, h->fail_dev, verify, pipe, h->window); };
    // verified calls on batches that leave lanes free run the ladder two rungs at a time, two quads per row (evalf_kernel_quad<PAIR>):
    // up to one wavefront per SIMD of the device (8 lanes per row); beyond that the sequential ladder does the same work on fewer lanes
    const bool pair = verify && h->ladder_parallel && !dcrop && (size_t)8 * B <= (size_t)WAVE * h->n_simd &&
                      (sizeof(T) == 8 || h->layout != GLGYM_LAYOUT_ONE);
    if constexpr (sizeof(T) == 8) {      // fp64: four lanes per row (no one-lane fp64 integrator exists any more), the variant selected at run time
        if (pair) quad(evalf_kernel_quad<T, SCH, true, false, true>, pgrid);
        else if (dcrop) quad(evalf_kernel_quad<T, SCH, true, true>, qgrid);
        else quad(evalf_kernel_quad<T, SCH, true, false>, qgrid);
    } else {
        if (pipe) one(evalf_kernel<T, false, true>);        // the single generic RK4 build (run_evalf)
        else if (pair) quad(evalf_kernel_quad<T, SCH, false, false, true>, pgrid);
        // fp32 rows without their own parameter block take the four-lanes-per-row kernel where glgym_step does (up to one round of
        // quad wavefronts: 16 384 rows on MI355X; glgym_set_layout overrides)
        else if (!dcrop && (h->layout == GLGYM_LAYOUT_QUAD || (h->layout == GLGYM_LAYOUT_AUTO && B <= 4 * h->n_simd * 4)))
            quad(evalf_kernel_quad<T, SCH, false, false, false>, qgrid);
        else if (dcrop) one(evalf_kernel<T, true, false, SCH>);
        else one(evalf_kernel<T, false, false, SCH>);
    }
}

template <class T>
static int run_evalf(glgym_handle h, const ModelConst<T>& m, const double* p_used, const double* dx, const double* du,
                     const double* dd, const double* dcrop, int B, double* dout, int rhs_only)
{
    const bool pipe = h->variant == GLGYM_ODE_PIPE;
    if (rhs_only) {                      // the right-hand side at one state per row (test hook): one lane per row in either dtype
        const dim3 grid((B + WAVE - 1) / WAVE), block(WAVE);
        if (pipe) hipLaunchKernelGGL((rhs_kernel<T, false, true>), grid, block, 0, (hipStream_t)0, dx, du, dd, dcrop, B, T(p_used[39]), T(p_used[162]), m, dout, h->nd);
        else if (dcrop) hipLaunchKernelGGL((rhs_kernel<T, true, false>), grid, block, 0, (hipStream_t)0, dx, du, dd, dcrop, B, T(p_used[39]), T(p_used[162]), m, dout, h->nd);
        else hipLaunchKernelGGL((rhs_kernel<T, false, false>), grid, block, 0, (hipStream_t)0, dx, du, dd, dcrop, B, T(p_used[39]), T(p_used[162]), m, dout, h->nd);
        HIPCHK(hipGetLastError());
        return GLGYM_OK;
    }
    if (pipe && (dcrop || h->scheme != GLGYM_SCHEME_RK4)) {
        g_err = "glgym_evalF: GLGYM_ODE_PIPE supports neither per-row parameter blocks nor schemes other than GLGYM_SCHEME_RK4";
        return GLGYM_EINVAL;
    }
    with_scheme(h->scheme, [&](auto sch) { launch_evalf_sch<T, decltype(sch)::value>(h, m, p_used, dx, du, dd, dcrop, B, dout); });
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

static int evalf_impl(glgym_handle h, const double* x, const double* u, const double* d, const double* p, int p_rows,
                      int B, double* out, int rhs_only)
{
    if (!h || !x || !u || !d || !out || B < 1 || (p && p_rows != 1 && p_rows != B)) {
        g_err = "glgym_evalF: bad arguments";
        return GLGYM_EINVAL;
    }
    HIPCHK(hipSetDevice(h->device));
    const bool bdf = !rhs_only && h->integrator == GLGYM_INTEGRATOR_BDF;
    if (bdf && h->variant == GLGYM_ODE_PIPE) {
        g_err = "glgym_evalF: GLGYM_INTEGRATOR_BDF does not support GLGYM_ODE_PIPE";
        return GLGYM_EINVAL;
    }
    const double* p_used = p ? p : h->p;
    // per-row parameter blocks may differ only inside the crop block p[128..161] (what noise.py perturbs);
    // anything else is handled one row at a time.
    bool per_row = p && p_rows == B && B > 1;
    if (per_row) {
        for (int b = 1; b < B && per_row; ++b)
            for (int i = 0; i < NP; ++i)
                if ((i < CROP0 || i >= CROP0 + NCROP) && p[(size_t)b * NP + i] != p[i]) {
                    std::vector<int32_t> st(bdf ? (size_t)B * GLGYM_NSOLVER_STAT : 0);
                    for (int r = 0; r < B; ++r) {
                        const int rc = evalf_impl(h, x + (size_t)r * NX, u + (size_t)r * NU, d + (size_t)r * h->nd,
                                                  p + (size_t)r * NP, 1, 1, out + (size_t)r * NX, rhs_only);
                        if (bdf && h->stats_rows == 1)
                            std::memcpy(&st[(size_t)r * GLGYM_NSOLVER_STAT], h->stats.data(), sizeof(int32_t) * GLGYM_NSOLVER_STAT);
                        if (rc != GLGYM_OK) return rc;
                    }
                    if (bdf) { h->stats = st; h->stats_rows = B; }
                    return GLGYM_OK;
                }
    }
    const size_t n_in = (size_t)B * (NX + NU + h->nd + (per_row ? NCROP : 0));
    int rc = ensure_scratch(h, n_in + (size_t)B * NX);
    if (rc != GLGYM_OK) return rc;
    double* dx = h->scratch; double* du = dx + (size_t)B * NX; double* dd = du + (size_t)B * NU;
    double* dcrop = per_row ? dd + (size_t)B * h->nd : nullptr;
    double* dout = h->scratch + n_in;
    HIPCHK(hipMemcpy(dx, x, (size_t)B * NX * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(du, u, (size_t)B * NU * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dd, d, (size_t)B * h->nd * sizeof(double), hipMemcpyHostToDevice));
    if (per_row) {
        std::vector<double> crop((size_t)B * NCROP);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < NCROP; ++i) crop[(size_t)b * NCROP + i] = p[(size_t)b * NP + CROP0 + i];
        HIPCHK(hipMemcpy(dcrop, crop.data(), crop.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(h->fail_dev, 0, sizeof(int)));
    HIPCHK(hipMemset(dout, 0xFF, (size_t)B * NX * sizeof(double)));      // a row no lane writes reads back as NaN, not as the previous call's
    if (bdf) {
        // fp64 for either handle dtype (every handle carries the fp64 constants)
        if (h->stats_cap < B) {
            if (h->stats_dev) (void)hipFree(h->stats_dev);
            h->stats_dev = nullptr; h->stats_cap = 0;
            HIPCHK(hipMalloc(&h->stats_dev, (size_t)B * GLGYM_NSOLVER_STAT * sizeof(int32_t)));
            h->stats_cap = B;
        }
        h->stats_rows = 0;
        ModelConst<double> m = h->md;
        if (p) make_model_const<double>(p_used, m);
        HIPCHK(bdf_launch(dx, du, dd, dcrop, B, h->nd, h->dt, h->rtol, h->atol, h->max_steps, m, p_used[39], p_used[162], dout,
                          h->stats_dev, h->fail_dev));
        h->stats.resize((size_t)B * GLGYM_NSOLVER_STAT);
        HIPCHK(hipMemcpy(h->stats.data(), h->stats_dev, h->stats.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        h->stats_rows = B;
    } else if (h->dtype == GLGYM_F32) {
        ModelConst<float> m = h->mf;
        if (p) make_model_const<float>(p_used, m);
        rc = run_evalf<float>(h, m, p_used, dx, du, dd, dcrop, B, dout, rhs_only);
    } else {
        ModelConst<double> m = h->md;
        if (p) make_model_const<double>(p_used, m);
        rc = run_evalf<double>(h, m, p_used, dx, du, dd, dcrop, B, dout, rhs_only);
    }
    if (rc != GLGYM_OK) return rc;
    HIPCHK(hipMemcpy(out, dout, (size_t)B * NX * sizeof(double), hipMemcpyDeviceToHost));
    int n_failed = 0;
    HIPCHK(hipMemcpy(&n_failed, h->fail_dev, sizeof(int), hipMemcpyDeviceToHost));
    if (n_failed > 0) {
        g_err = "glgym_evalF: the integration failed for " + std::to_string(n_failed) + " of " + std::to_string(B) +
                (bdf ? " rows (BDF: step limit, right-hand-side limit, step-size underflow or a non-finite value)"
                     : " rows (no two consecutive attempts of the n_sub, 2x, 4x, 8x ladder agreed)") + "; their rows of x_next are NaN";
        return GLGYM_EODE;
    }
    // Every row of a call that reports no failure has been written by exactly one lane group; the buffer was NaN-filled before the
    // launch, so a row that still reads NaN here was written by NO lane -- the signature of the lane-mask miscompile of round 5
    // (tools/README.md "pair ladder"; designed around, not root-caused).  Never hand such a row back with GLGYM_OK.
    if (!rhs_only) {
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < NX; ++i)
                if (std::isnan(out[(size_t)b * NX + i])) {
                    g_err = "glgym_evalF: row " + std::to_string(b) + " of " + std::to_string(B) + " came back unwritten (state " + std::to_string(i) +
                            " is NaN although no integration was reported as failed): internal error of the kernel's row-writing lane selection";
                    return GLGYM_EHIP;
                }
    }
    return GLGYM_OK;
}

extern "C" {

int glgym_evalF(glgym_handle h, const double* x, const double* u, const double* d, const double* p, int p_rows, int B,
                double* x_next)
{
    return evalf_impl(h, x, u, d, p, p_rows, B, x_next, 0);
}

int glgym_rhs(glgym_handle h, const double* x, const double* u, const double* d, int B, double* dx)
{
    return evalf_impl(h, x, u, d, nullptr, 1, B, dx, 1);
}

}  // extern "C"

// ---- device-pointer hot path ----------------------------------------------------------------------
static const int OBS_MODULE_SIZE[6] = {4, 3, 6, 5, 5, 0};      // observations.py:64,84,102,123,143; forecast = 5 * Np (:168)
// first column of each observation module in the handle's module order (-1 = absent) and the row width
static void obs_layout(glgym_handle h, int Np, int moff[6], int* dim)
{
    for (int m = 0; m < 6; ++m) moff[m] = -1;
    *dim = 0;
    for (int i = 0; i < h->n_obs_modules; ++i) {
        const int m = h->obs_modules[i];
        moff[m] = *dim;
        *dim += m == GLGYM_OBS_FORECAST ? 5 * Np : OBS_MODULE_SIZE[m];
    }
}
static void obs_clock_increments(glgym_handle h, double* doy_inc, double* hod_inc)
{
    *doy_inc = std::fmod(h->dt / 86400.0, 365.0);
    *hod_inc = h->dt / 3600.0;
}
// the observation block of a glgym_step_obs call names the step's own buffers, in full mode, with rows the epilogue's float4 stores can take
static bool obs_same_buffers(const glgym_step_args* a, const glgym_obs_args* oa)
{
    return oa && !oa->mask && oa->B == a->B && oa->ld == a->ld && oa->x == a->x && oa->u == a->u && oa->weather == a->weather &&
           oa->weather_rows == a->weather_rows && oa->w_off == a->w_off && oa->timestep == a->timestep && ((uintptr_t)oa->obs & 15) == 0;
}
// the reset block of a glgym_step_obs_reset call names the step's and the observation's own buffers and carries a start table
static bool reset_same_buffers(const glgym_step_args* a, const glgym_obs_args* oa, const glgym_reset_args* ra)
{
    return ra && ra->B == a->B && ra->ld == a->ld && ra->x == a->x && ra->u == a->u && ra->timestep == a->timestep &&
           ra->weather == a->weather && ra->weather_rows == a->weather_rows && ra->w_off == a->w_off && ra->start_rows &&
           ra->start_days && ra->n_starts > 0 && ra->start_day && ra->start_day == oa->start_day && ra->episode;
}

static_assert(glsel::WAVE == WAVE && glsel::SCH_OBS == GL_SCH_OBS && glsel::SCH_RESET == GL_SCH_RESET && glsel::RK4 == GLGYM_SCHEME_RK4 &&
              glsel::OBS_MAX_DIM_OCC1 == STEP_OBS_MAX_DIM_OCC1 && glsel::OBS_MAX_DIM_OCC2 == STEP_OBS_MAX_DIM_OCC2, "gl_step_select.hpp");
template <int EPI> static typename StepObsSel<EPI>::type epilogue_args(const StepObsResetArgs& ob)
{
    if constexpr (EPI == 0) return {}; else return ob;
}

// The step launcher: the build is chosen by glsel::select_step (gl_step_select.hpp, where the rules and the list of builds are) and
// mapped to its kernel through that list.
// oa (glgym_step_obs): full-mode observation arguments.  Where the chosen build has the observation epilogue, *fused is set and the
// rows are written by this launch (*fused = 1); everywhere else the step is launched as ever and the caller launches obs_kernel behind it.
// ra (glgym_step_obs_reset, with oa): the reset of the environments the step finishes.  Where the build also has the auto-reset epilogue
// (*fused = 2) nothing is left for the caller to launch.
// (No fp64 build with the default block compiled in: measured without the scheduler flag that used to break it -- csrc/Makefile --
// it buys 0.7 % over the LDS-staged block, 1.379e6 against 1.369e6 env-steps/s at config 2, for six more 500-register kernels.)
template <class T>
static int launch_step(glgym_handle h, const glgym_step_args* a, const ModelConst<T>& m, const RewardConst<T>& rw,
                       hipStream_t st, const glgym_obs_args* oa = nullptr, int* fused = nullptr, const glgym_reset_args* ra = nullptr)
{
    StepArgsT<T> k;
    k.B = a->B; k.ld = a->ld;
    k.x = (T*)a->x; k.u = (T*)a->u; k.action = a->action; k.control = (const T*)a->control;
    k.weather = (const T*)a->weather; k.weather_rows = a->weather_rows;
    k.w_off = a->w_off; k.timestep = a->timestep; k.crop_p = (const T*)a->crop_p; k.N = a->N;
    k.reward = (T*)a->reward; k.info = (T*)a->info; k.done = a->done; k.metrics = a->metrics; k.step_flags = a->step_flags;
    k.dt = T(h->dt); k.n_sub = h->n_sub; k.gasR = T(h->p[39]); k.tCanMin = T(h->p[162]); k.nd = h->nd;
    k.du = h->du;
    for (int j = 0; j < NU; ++j) { k.u_min[j] = h->u_min[j]; k.u_max[j] = h->u_max[j]; }
    // AUTO: verified wherever the control can jump -- raw controls (step_raw_control, the rule-based controller), or an action
    // path whose delta_u_max is wider than the reference's 0.1 (TomatoEnv.yml; base_env.py:74)
    k.pipe = h->variant == GLGYM_ODE_PIPE ? 1 : 0;
    k.window = h->window;
    k.verify = h->verify_mode == GLGYM_VERIFY_ALWAYS || (h->verify_mode == GLGYM_VERIFY_AUTO && (!a->action || h->du > 0.1001f));
    // glgym_set_layout / _occupancy are handle state since round 5; the environment variables GLGYM_LAYOUT / GLGYM_OCC are only their
    // INITIAL values, read once at glgym_create (changing os.environ afterwards has no effect on an existing handle).
    glsel::StepSelectIn in;
    in.f64 = sizeof(T) == 8; in.scheme = h->scheme; in.pipe = k.pipe != 0; in.crop = a->crop_p != nullptr;
    in.def = h->use_specialised && std::memcmp(&m, &DefaultConst<T>::value, sizeof m) == 0;
    in.layout = h->layout; in.occupancy = h->occupancy; in.B = a->B; in.n_simd = h->n_simd;
    in.verify = k.verify != 0; in.ladder_parallel = h->ladder_parallel != 0;
    StepObsResetArgs ob;
    in.obs_ok = !glsel::takes_quad(in) && obs_same_buffers(a, oa);      // the quad builds have no epilogue: nothing of oa / ra is looked at
    in.obs_dim = 0;
    if (in.obs_ok) {
        ob.obs = oa->obs; ob.start_day = oa->start_day; ob.Np = oa->Np;
        obs_clock_increments(h, &ob.doy_inc, &ob.hod_inc);
        obs_layout(h, oa->Np, ob.moff, &ob.dim);
        in.obs_dim = ob.dim;
    }
    in.reset_ok = in.obs_ok && reset_same_buffers(a, oa, ra);
    if (in.reset_ok) {
        ob.term_obs = oa->term_obs; ob.w_off_rw = ra->w_off; ob.start_day_rw = ra->start_day; ob.episode = ra->episode;
        ob.start_rows = ra->start_rows; ob.start_days = ra->start_days; ob.n_starts = ra->n_starts;
        ob.seed = (unsigned long long)ra->seed;
    }
    const glsel::StepChoice c = glsel::select_step(in);
    if (c.error) { g_err = c.error; return GLGYM_EINVAL; }
    const dim3 grid(c.grid), block(WAVE);
    const glsel::StepBuild& b = c.build;
    bool launched = false;
    with_scheme(b.sch, [&](auto sch) {
        constexpr int SCH = decltype(sch)::value;
#define GL_LAUNCH_QUAD(F64, DEF, PIPE, CROP, PAIR)                                                                                    \
        if constexpr (F64 == (sizeof(T) == 8))                                                                                       \
            if (!launched && b == glsel::StepBuild{PAIR ? glsel::QUAD_PAIR : glsel::QUAD, F64, CROP, DEF, PIPE, SCH, 0, 1}) {        \
                hipLaunchKernelGGL((step_kernel_quad<T, DEF, SCH, PIPE, CROP, PAIR>), grid, block, 0, st, k, m, rw);                 \
                launched = true;                                                                                                     \
            }
        GL_STEP_QUAD_BUILDS(GL_LAUNCH_QUAD)
#undef GL_LAUNCH_QUAD
#define GL_LAUNCH_ONE(CROP, DEF, PIPE, EPI, OCC)                                                                                      \
        if constexpr (sizeof(T) == 4 && glsel::one_lane_build_exists(PIPE, SCH))                                                     \
            if (!launched && b == glsel::StepBuild{glsel::ONE_LANE, false, CROP, DEF, PIPE, SCH, EPI, OCC}) {                        \
                hipLaunchKernelGGL((step_kernel<T, CROP, DEF, PIPE, SCH | EPI, OCC>), grid, block, 0, st, k, m, rw, epilogue_args<EPI>(ob)); \
                launched = true;                                                                                                     \
            }
        GL_STEP_ONE_LANE_BUILDS(GL_LAUNCH_ONE)
#undef GL_LAUNCH_ONE
    });
    // unreachable: every build select_step returns is in the lists (tests/test_step_select_host.py asserts it over the full product)
    if (!launched) { g_err = "glgym_step: no kernel was built for the selected configuration (gl_step_select.hpp)"; return GLGYM_EINVAL; }
    HIPCHK(hipGetLastError());
    if (c.fused && fused) *fused = c.fused;
    return GLGYM_OK;
}

// glgym_set_step_integrator(h, GLGYM_INTEGRATOR_BDF): one wavefront per environment in glgym_bdf.hip, fp64 integration for either dtype
template <class T>
static int launch_step_bdf(glgym_handle h, const glgym_step_args* a, const RewardConst<T>& rw, hipStream_t st)
{
    if (h->variant == GLGYM_ODE_PIPE) {
        g_err = "glgym_step: GLGYM_INTEGRATOR_BDF does not support GLGYM_ODE_PIPE";
        return GLGYM_EINVAL;
    }
    glbdf::BdfEnvArgs<T> k;
    k.ld = a->ld;
    k.x = (T*)a->x; k.u = (T*)a->u; k.action = a->action; k.control = (const T*)a->control;
    k.weather = (const T*)a->weather; k.weather_rows = a->weather_rows; k.nd = h->nd;
    k.w_off = a->w_off; k.timestep = a->timestep; k.crop_p = (const T*)a->crop_p; k.N = a->N;
    k.reward = (T*)a->reward; k.info = (T*)a->info; k.done = a->done; k.step_flags = a->step_flags;
    k.dt = h->dt; k.rtol = h->rtol; k.atol = h->atol; k.max_steps = h->max_steps;
    k.gasR = h->p[39]; k.tCanMin = h->p[162];
    k.du = h->du;
    for (int j = 0; j < NU; ++j) { k.u_min[j] = h->u_min[j]; k.u_max[j] = h->u_max[j]; }
    HIPCHK(bdf_env_launch<T>(k, a->B, h->md, rw, a->metrics, st));
    return GLGYM_OK;
}

static int step_impl(glgym_handle h, const glgym_step_args* a, void* stream, const glgym_obs_args* oa, int* fused,
                     const glgym_reset_args* ra = nullptr)
{
    if (!h || !a) { g_err = "glgym_step: null handle / arguments"; return GLGYM_EINVAL; }
    if (a->struct_size != (int32_t)sizeof(glgym_step_args)) {     // checked before any pointer member is read
        g_err = "glgym_step: glgym_step_args.struct_size is " + std::to_string(a->struct_size) + ", this library expects " +
                std::to_string(sizeof(glgym_step_args)) + " (ABI " + std::to_string(GLGYM_ABI_VERSION) + "): rebuild against include/glgym.h";
        return GLGYM_EINVAL;
    }
    if (a->B < 1 || a->ld < a->B || !a->x || !a->u || !a->weather || !a->w_off || !a->timestep ||
        !a->reward || !a->done || (!a->action) == (!a->control) || a->weather_rows < 1) {
        g_err = "glgym_step: bad arguments (exactly one of action/control, ld >= B, non-null state/outputs)";
        return GLGYM_EINVAL;
    }
    if (h->step_integrator == GLGYM_INTEGRATOR_BDF) {
        DeviceGuard dev_guard(h);
        return h->dtype == GLGYM_F32 ? launch_step_bdf<float>(h, a, h->rf, (hipStream_t)stream)
                                     : launch_step_bdf<double>(h, a, h->rd, (hipStream_t)stream);
    }
    if (h->integrator != GLGYM_INTEGRATOR_EXPLICIT) {
        g_err = "glgym_step: GLGYM_INTEGRATOR_BDF is available to glgym_evalF only; set GLGYM_INTEGRATOR_EXPLICIT for env-steps";
        return GLGYM_EINVAL;
    }
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    return h->dtype == GLGYM_F32 ? launch_step<float>(h, a, h->mf, h->rf, st, oa, fused, ra)
                                 : launch_step<double>(h, a, h->md, h->rd, st);
}

extern "C" int glgym_step(glgym_handle h, const glgym_step_args* a, void* stream)
{
    return step_impl(h, a, stream, nullptr, nullptr);
}

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
    if (h->dtype == GLGYM_F32)
        hipLaunchKernelGGL((pchip_eval_kernel<float>), grid, dim3(256), 0, st, n, 10, a->n_out, a->nd, a->time, W, D,
                           (float*)a->out);
    else
        hipLaunchKernelGGL((pchip_eval_kernel<double>), grid, dim3(256), 0, st, n, 10, a->n_out, a->nd, a->time, W, D,
                           (double*)a->out);
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
        if (h->dtype == GLGYM_F32)
            hipLaunchKernelGGL((vecnorm_returns_kernel<float>), dim3((B + 255) / 256), dim3(256), 0, st,
                               (const float*)a->reward, a->returns, B, a->gamma, acc2);
        else
            hipLaunchKernelGGL((vecnorm_returns_kernel<double>), dim3((B + 255) / 256), dim3(256), 0, st,
                               (const double*)a->reward, a->returns, B, a->gamma, acc2);
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
        if (h->dtype == GLGYM_F32)
            hipLaunchKernelGGL((vecnorm_reward_kernel<float>), dim3((B + 255) / 256), dim3(256), 0, st,
                               (const float*)a->reward, a->reward_out, a->returns, a->done, B, a->ret_stats, a->epsilon,
                               a->clip_reward, a->norm_reward);
        else
            hipLaunchKernelGGL((vecnorm_reward_kernel<double>), dim3((B + 255) / 256), dim3(256), 0, st,
                               (const double*)a->reward, a->reward_out, a->returns, a->done, B, a->ret_stats, a->epsilon,
                               a->clip_reward, a->norm_reward);
    }
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

extern "C" {

static bool obs_args_ok(glgym_handle h, const glgym_obs_args* a)
{
    return h && a && a->B >= 1 && a->ld >= a->B && a->x && a->u && a->weather && a->weather_rows >= 1 && a->w_off && a->timestep &&
           a->start_day && a->obs && a->Np >= 0 && a->Np <= OBS_MAX_NP;      // weather_rows < 1: the row clamp would yield row -1
}

int glgym_obs(glgym_handle h, const glgym_obs_args* a, void* stream)
{
    DeviceGuard dev_guard(h);
    if (!obs_args_ok(h, a)) {
        g_err = "glgym_obs: bad arguments (null pointer, ld < B, weather_rows < 1, or Np outside 0..128)";
        return GLGYM_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    return h->dtype == GLGYM_F32 ? launch_obs<float>(h, a, st) : launch_obs<double>(h, a, st);
}

int glgym_step_obs(glgym_handle h, const glgym_step_args* a, const glgym_obs_args* oa, void* stream)
{
    if (!h || !a || !oa) { g_err = "glgym_step_obs: null handle / arguments"; return GLGYM_EINVAL; }
    if (oa->mask) { g_err = "glgym_step_obs: full-mode observations only (glgym_obs_args.mask must be NULL)"; return GLGYM_EINVAL; }
    if (!obs_args_ok(h, oa)) {         // before the step is launched: nothing runs on bad arguments
        g_err = "glgym_step_obs: bad observation arguments (null pointer, ld < B, weather_rows < 1, or Np outside 0..128)";
        return GLGYM_EINVAL;
    }
    int fused = 0;
    const int rc = step_impl(h, a, stream, oa, &fused);
    if (rc != GLGYM_OK || fused) return rc;
    return glgym_obs(h, oa, stream);
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

static bool reset_args_ok(const glgym_reset_args* a)
{
    return a && a->B >= 1 && a->ld >= a->B && a->x && a->u && a->timestep && a->weather && a->weather_rows >= 1 && a->w_off;
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
    if (h->dtype == GLGYM_F32)
        hipLaunchKernelGGL((reset_kernel<float>), grid, block, 0, st, a->B, a->ld, a->mask, (float*)a->x, (float*)a->u,
                           a->timestep, (const float*)a->weather, a->weather_rows, a->w_off, a->start_rows, a->start_days,
                           a->n_starts, a->start_day, a->episode, (unsigned long long)a->seed, h->nd);
    else
        hipLaunchKernelGGL((reset_kernel<double>), grid, block, 0, st, a->B, a->ld, a->mask, (double*)a->x,
                           (double*)a->u, a->timestep, (const double*)a->weather, a->weather_rows, a->w_off,
                           a->start_rows, a->start_days, a->n_starts, a->start_day, a->episode,
                           (unsigned long long)a->seed, h->nd);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_step_obs_reset(glgym_handle h, const glgym_step_args* a, const glgym_obs_args* oa, const glgym_reset_args* ra, void* stream,
                         int32_t* fused_out)
{
    if (fused_out) *fused_out = 0;
    if (!h || !a || !oa || !ra) { g_err = "glgym_step_obs_reset: null handle / arguments"; return GLGYM_EINVAL; }
    if (a->struct_size != (int32_t)sizeof(glgym_step_args)) return step_impl(h, a, stream, nullptr, nullptr);      // its message, nothing launched
    if ((oa->mask && oa->mask != a->done) || (ra->mask && ra->mask != a->done)) {
        g_err = "glgym_step_obs_reset: the masks of the observation and reset blocks must be NULL or the step's `done`";
        return GLGYM_EINVAL;
    }
    if (!obs_args_ok(h, oa) || !reset_args_ok(ra)) {
        g_err = "glgym_step_obs_reset: bad observation or reset arguments (null pointer, ld < B, weather_rows < 1, or Np outside 0..128)";      // before the step is launched: nothing runs on bad arguments
        return GLGYM_EINVAL;
    }
    glgym_obs_args full = *oa, masked = *oa;
    full.mask = nullptr; full.term_obs = oa->term_obs;
    masked.mask = a->done;
    glgym_reset_args rst = *ra;
    rst.mask = a->done;
    int fused = 0;
    int rc = step_impl(h, a, stream, &full, &fused, &rst);
    if (rc == GLGYM_OK && fused == 2 && fused_out) *fused_out = 1;
    if (rc != GLGYM_OK || fused == 2) return rc;
    if (!fused && (rc = glgym_obs(h, &full, stream)) != GLGYM_OK) return rc;
    if ((rc = glgym_reset(h, &rst, stream)) != GLGYM_OK) return rc;
    return glgym_obs(h, &masked, stream);
}

int glgym_crop_noise(glgym_handle h, void* crop_p, int B, int ld, double scale, uint64_t seed, uint64_t draw_index,
                     void* stream)
{
    DeviceGuard dev_guard(h);
    if (!h || !crop_p || B < 1 || ld < B) return GLGYM_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((B + 255) / 256), block(256);
    if (h->dtype == GLGYM_F32)
        hipLaunchKernelGGL((crop_noise_kernel<float>), grid, block, 0, st, (float*)crop_p, B, ld, h->p0_crop_dev,
                           (float)scale, (unsigned long long)seed, (unsigned long long)draw_index);
    else
        hipLaunchKernelGGL((crop_noise_kernel<double>), grid, block, 0, st, (double*)crop_p, B, ld, h->p0_crop_dev,
                           (float)scale, (unsigned long long)seed, (unsigned long long)draw_index);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_rng_crop_noise(glgym_handle h, void* crop_p, int B, int ld, double scale, uint64_t* rng_state, void* stream)
{
    DeviceGuard dev_guard(h);
    if (!h || !rng_state || B < 1 || ld < B || !(scale >= 0.0)) {
        g_err = "glgym_rng_crop_noise: bad arguments (null handle or stream buffer, ld < B, or a negative scale)";
        return GLGYM_EINVAL;
    }
    hipStream_t st = (hipStream_t)stream;
    if (h->dtype == GLGYM_F32) HIPCHK(rng_crop_noise_launch<float>((float*)crop_p, B, ld, h->p0_crop_dev, scale, rng_state, st));
    else HIPCHK(rng_crop_noise_launch<double>((double*)crop_p, B, ld, h->p0_crop_dev, scale, rng_state, st));
    return GLGYM_OK;
}

int glgym_rng_reset_draw(glgym_handle h, int B, int ld, const unsigned char* mask, uint64_t* rng_state, int n_years, int n_days,
                         const int32_t* start_rows, const float* start_days, int32_t* w_off, float* start_day, void* stream)
{
    DeviceGuard dev_guard(h);
    if (!h || !rng_state || B < 1 || ld < B || n_years < 1 || n_days < 1 || !start_rows || !w_off) {
        g_err = "glgym_rng_reset_draw: bad arguments (null pointer, ld < B, or an empty start grid)";
        return GLGYM_EINVAL;
    }
    HIPCHK(rng_reset_draw_launch(B, ld, mask, rng_state, n_years, n_days, start_rows, start_days, w_off, start_day, (hipStream_t)stream));
    return GLGYM_OK;
}

// ---- device-side planning (glgym_plan.hip): host side only -- argument checks, and glgym_plan_rollout's loop over glgym_step ----
static bool plan_size_ok(const char* who, int32_t got, size_t want)
{
    if (got == (int32_t)want) return true;
    g_err = std::string(who) + ": struct_size is " + std::to_string(got) + ", this library expects " + std::to_string(want) +
            " (ABI " + std::to_string(GLGYM_ABI_VERSION) + "): rebuild against include/glgym.h";
    return false;
}

int glgym_plan_fork(glgym_handle h, const glgym_plan_fork_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_fork: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_fork", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->n_children < 1 || a->n_parents < 1 || a->ld_parent < a->n_parents || a->ld_child < a->n_children ||
        (!a->parent && (a->K < 1 || (int64_t)a->n_parents * a->K < a->n_children)) ||
        !a->x_parent || !a->u_parent || !a->timestep_parent || !a->w_off_parent || !a->x || !a->u || !a->timestep || !a->w_off ||
        !a->ret || !a->viol || !a->n_steps || !a->alive || !a->failed) {
        g_err = "glgym_plan_fork: bad arguments (null pointer, ld < batch, or without a parent table K < 1 or fewer than C = P * K slots)";
        return GLGYM_EINVAL;
    }
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->dtype == GLGYM_F32) HIPCHK(plan_fork_launch<float>(*a, st));
    else HIPCHK(plan_fork_launch<double>(*a, st));
    return GLGYM_OK;
}

int glgym_plan_accumulate(glgym_handle h, const glgym_plan_accumulate_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_accumulate: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_accumulate", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->B < 1 || a->ld < a->B || !a->reward || !a->info || !a->done || !a->ret || !a->viol || !a->n_steps || !a->alive || !a->failed) {
        g_err = "glgym_plan_accumulate: bad arguments (null pointer or ld < B)";
        return GLGYM_EINVAL;
    }
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->dtype == GLGYM_F32) HIPCHK(plan_accumulate_launch<float>(*a, st));
    else HIPCHK(plan_accumulate_launch<double>(*a, st));
    return GLGYM_OK;
}

int glgym_plan_rollout(glgym_handle h, const glgym_plan_rollout_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_rollout: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_rollout", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->H < 1 || !(a->gamma >= 0.0) || !std::isfinite(a->gamma) || (!a->actions) == (!a->controls) || a->step.B < 1 ||
        a->step.ld < a->step.B || !a->step.reward || !a->step.info || !a->step.done || !a->ret || !a->viol || !a->n_steps ||
        !a->alive || !a->failed) {
        g_err = "glgym_plan_rollout: bad arguments (H < 1, gamma, exactly one of actions / controls, ld >= B, non-null reward / info / done / accumulators)";
        return GLGYM_EINVAL;
    }
    glgym_step_args s = a->step;                 // glgym_step checks its struct_size and the remaining members
    s.metrics = nullptr;
    glgym_plan_accumulate_args acc;
    acc.struct_size = (int32_t)sizeof acc;
    acc.B = s.B; acc.ld = s.ld; acc.reward = s.reward; acc.info = s.info; acc.done = s.done; acc.step_flags = s.step_flags;
    acc.ret = a->ret; acc.viol = a->viol; acc.n_steps = a->n_steps; acc.alive = a->alive; acc.failed = a->failed;
    const size_t plane = (size_t)NU * (size_t)s.ld * (h->dtype == GLGYM_F32 ? sizeof(float) : sizeof(double));
    double w = 1.0;
    for (int k = 0; k < a->H; ++k) {
        s.action = a->actions ? a->actions + (size_t)k * (size_t)s.B * NU : nullptr;
        s.control = a->controls ? (const void*)((const char*)a->controls + (size_t)k * plane) : nullptr;
        const int rc = glgym_step(h, &s, stream);
        if (rc != GLGYM_OK) return rc;
        acc.w = w;
        const int ra = glgym_plan_accumulate(h, &acc, stream);
        if (ra != GLGYM_OK) return ra;
        w = w * a->gamma;
    }
    return GLGYM_OK;
}

int glgym_plan_select(glgym_handle h, const glgym_plan_select_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_select: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_select", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    const bool wants_actions = a->best_action || a->best_sequence || a->mean_sequence;
    if (a->P < 1 || a->K < 1 || a->H < 1 || a->H > 65535 || (int64_t)a->P * a->K > INT32_MAX || !a->ret || !a->failed || !a->best_k ||
        !a->best_ret || (wants_actions && !a->actions) || (a->mean_sequence && !(a->temperature > 0.0 && std::isfinite(a->temperature)))) {
        g_err = "glgym_plan_select: bad arguments (P, K, H < 1, H > 65 535, null pointer, action outputs without actions, or mean_sequence "
                "without a finite temperature > 0)";
        return GLGYM_EINVAL;
    }
    // the kernel multiplies by 1 / temperature: at 2^-1024 and below that is +inf and the best candidate's own (ret - max) * inf = 0 * inf a NaN
    if (a->mean_sequence && !std::isfinite(1.0 / a->temperature)) {
        g_err = "glgym_plan_select: temperature is too small (1 / temperature is not finite: it must be above 2^-1024, about 5.6e-309)";
        return GLGYM_EINVAL;
    }
    DeviceGuard dev_guard(h);
    HIPCHK(plan_select_launch(*a, (hipStream_t)stream));
    return GLGYM_OK;
}

// the cross-entropy method's stages (gl_cem.hpp): every check that needs no device memory happens here, before anything is launched
int glgym_plan_sample(glgym_handle h, const glgym_plan_sample_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_sample: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_sample", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->P < 1 || a->K < 1 || a->H < 1 || (int64_t)a->P * a->K > INT32_MAX - 255 || !a->mean || !a->std || !a->actions ||
        !(a->beta >= 0.0 && a->beta < 1.0) || a->carry < 0 ||
        (a->carry > 0 && (!a->prev_actions || !a->prev_elite_k || !a->prev_n_elite || a->prev_E < a->carry || a->prev_actions == a->actions))) {
        g_err = "glgym_plan_sample: bad arguments (P, K, H < 1, null pointer, beta outside [0, 1), carry < 0, or with carry > 0: a missing "
                "prev_ member, carry > prev_E, or prev_actions == actions -- sample into the other of two blocks)";
        return GLGYM_EINVAL;
    }
    DeviceGuard dev_guard(h);
    HIPCHK(plan_sample_launch(*a, (hipStream_t)stream));
    return GLGYM_OK;
}

int glgym_plan_elites(glgym_handle h, const glgym_plan_elites_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_elites: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_elites", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->P < 1 || a->K < 1 || a->E < 1 || a->E > a->K || (int64_t)a->P * a->K > INT32_MAX - 255 || !a->ret || !a->failed || !a->elite_k ||
        !a->n_elite) {
        g_err = "glgym_plan_elites: bad arguments (P, K < 1, E outside 1..K, or null pointer)";
        return GLGYM_EINVAL;
    }
    DeviceGuard dev_guard(h);
    HIPCHK(plan_elites_launch(*a, (hipStream_t)stream));
    return GLGYM_OK;
}

int glgym_plan_refit(glgym_handle h, const glgym_plan_refit_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_refit: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_refit", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->P < 1 || a->K < 1 || a->H < 1 || a->H > 65535 || a->E < 1 || a->E > a->K || (int64_t)a->P * a->K > INT32_MAX - 255 ||
        !a->actions || !a->elite_k || !a->n_elite || !a->mean || !a->std || !a->mean_out || !a->std_out ||
        !(a->alpha >= 0.0 && a->alpha < 1.0) || !(a->min_std >= 0.0 && std::isfinite(a->min_std))) {
        g_err = "glgym_plan_refit: bad arguments (P, K, H < 1, H > 65 535, E outside 1..K, null pointer, alpha outside [0, 1), or min_std "
                "negative or not finite)";
        return GLGYM_EINVAL;
    }
    DeviceGuard dev_guard(h);
    HIPCHK(plan_refit_launch(*a, (hipStream_t)stream));
    return GLGYM_OK;
}

// robust planning (gl_scen.hpp).  The arguments are checked before the handle is looked at, so that a caller without a device gets the
// refusal that names its mistake.
static bool scenario_shape_ok(int32_t P, int32_t K, int32_t S, int32_t hold, double scale)
{
    return P >= 1 && K >= 1 && S >= 1 && S <= 256 && (int64_t)P * K * S <= INT32_MAX && (hold == 0 || hold == 1) && scale >= 0.0 &&
           std::isfinite(scale);
}

int glgym_plan_scenario(glgym_handle h, const glgym_plan_scenario_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_scenario: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_scenario", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (!scenario_shape_ok(a->P, a->K, a->S, a->hold, a->scale) || (int64_t)a->ld < (int64_t)a->P * a->K * a->S || a->h_step < 0 ||
        a->h_step > 65535 || !a->crop || (!a->actions_in) != (!a->actions_out)) {
        g_err = "glgym_plan_scenario: bad arguments (P, K, S < 1, S > 256, P*K*S > INT32_MAX, ld < P*K*S, h_step outside 0 .. 65 535, hold "
                "not 0 | 1, scale negative or not finite, null crop, or one of actions_in / actions_out without the other)";
        return GLGYM_EINVAL;
    }
    if (!h) { g_err = "glgym_plan_scenario: null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->dtype == GLGYM_F32) HIPCHK(plan_scenario_launch<float>(*a, h->p0_crop_dev, st));
    else HIPCHK(plan_scenario_launch<double>(*a, h->p0_crop_dev, st));
    return GLGYM_OK;
}

int glgym_plan_aggregate(glgym_handle h, const glgym_plan_aggregate_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_aggregate: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_aggregate", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->J < 1 || a->S < 1 || a->S > 256 || a->m < 1 || a->m > a->S || (int64_t)a->J * a->S > INT32_MAX || !a->ret || !a->failed ||
        !a->ret_cand || !a->failed_cand || (a->viol_cand && (!a->viol || (int64_t)a->ld < (int64_t)a->J * a->S || a->ld_cand < a->J)) ||
        (a->steps_cand && !a->n_steps)) {
        g_err = "glgym_plan_aggregate: bad arguments (J, S < 1, S > 256, m outside 1 .. S, J*S > INT32_MAX, null pointer, or with viol_cand: "
                "ld < J*S or ld_cand < J)";
        return GLGYM_EINVAL;
    }
    if (!h) { g_err = "glgym_plan_aggregate: null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    HIPCHK(plan_aggregate_launch(*a, (hipStream_t)stream));
    return GLGYM_OK;
}

int glgym_plan_rollout_scenarios(glgym_handle h, const glgym_plan_rollout_scenarios_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_rollout_scenarios: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_rollout_scenarios", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    const glgym_plan_rollout_args& r = a->rollout;
    if (!plan_size_ok("glgym_plan_rollout_scenarios: rollout", r.struct_size, sizeof r)) return GLGYM_EINVAL;
    if (r.controls) {
        g_err = "glgym_plan_rollout_scenarios: raw-control scenario rollouts are not supported (rollout.controls must be NULL)";
        return GLGYM_EINVAL;
    }
    glgym_step_args s = r.step;
    if (!scenario_shape_ok(a->P, a->K, a->S, a->hold, a->scale) || !a->staging || r.H < 1 || r.H > 65536 || !(r.gamma >= 0.0) ||
        !std::isfinite(r.gamma) || !r.actions || (int64_t)s.B != (int64_t)a->P * a->K * a->S || s.ld < s.B || !s.crop_p || !s.reward ||
        !s.info || !s.done || !r.ret || !r.viol || !r.n_steps || !r.alive || !r.failed) {
        g_err = "glgym_plan_rollout_scenarios: bad arguments (P, K, S < 1, S > 256, hold not 0 | 1, scale negative or not finite, null "
                "staging / actions / crop_p / reward / info / done / accumulators, H outside 1 .. 65 536, gamma, step.B != P*K*S, or ld < B)";
        return GLGYM_EINVAL;
    }
    if (!h) { g_err = "glgym_plan_rollout_scenarios: null handle"; return GLGYM_EINVAL; }
    s.metrics = nullptr;
    s.action = a->staging;
    s.control = nullptr;
    // what glgym_step refuses without launching is refused by it, in its own words, before the first prologue is launched: a struct
    // or pointer it checks itself, GLGYM_ODE_PIPE with a crop block (either step integrator), a BDF glgym_evalF setting on explicit steps
    if (s.struct_size != (int32_t)sizeof s || !s.x || !s.u || !s.weather || !s.w_off || !s.timestep || s.weather_rows < 1 ||
        h->variant == GLGYM_ODE_PIPE || (h->step_integrator != GLGYM_INTEGRATOR_BDF && h->integrator != GLGYM_INTEGRATOR_EXPLICIT)) {
        const int rc = glgym_step(h, &s, stream);
        if (rc != GLGYM_OK) return rc;
        g_err = "glgym_plan_rollout_scenarios: glgym_step accepted a call it was expected to refuse";        // unreachable
        return GLGYM_EINVAL;
    }
    glgym_plan_scenario_args sc;
    sc.struct_size = (int32_t)sizeof sc;
    sc.P = a->P; sc.K = a->K; sc.S = a->S; sc.ld = s.ld; sc.hold = a->hold; sc.scale = a->scale; sc.seed = a->seed;
    sc.draw_index = a->draw_index; sc.draw_base = a->draw_base; sc.crop = (void*)s.crop_p; sc.actions_out = a->staging;
    glgym_plan_accumulate_args acc;
    acc.struct_size = (int32_t)sizeof acc;
    acc.B = s.B; acc.ld = s.ld; acc.reward = s.reward; acc.info = s.info; acc.done = s.done; acc.step_flags = s.step_flags;
    acc.ret = r.ret; acc.viol = r.viol; acc.n_steps = r.n_steps; acc.alive = r.alive; acc.failed = r.failed;
    const size_t plane = (size_t)a->P * (size_t)a->K * NU;             // the candidates' action plane of one step
    double w = 1.0;
    for (int k = 0; k < r.H; ++k) {
        sc.h_step = k;
        sc.actions_in = r.actions + (size_t)k * plane;
        int rc = glgym_plan_scenario(h, &sc, stream);
        if (rc != GLGYM_OK) return rc;
        if ((rc = glgym_step(h, &s, stream)) != GLGYM_OK) return rc;
        acc.w = w;
        if ((rc = glgym_plan_accumulate(h, &acc, stream)) != GLGYM_OK) return rc;
        w = w * r.gamma;
    }
    return GLGYM_OK;
}

// weather-forecast scenarios (gl_wscen.hpp): checked before the handle is looked at, like the entry points above
int glgym_plan_weather(glgym_handle h, const glgym_plan_weather_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_weather: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_weather", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    bool sigma_ok = true;
    for (int j = 0; j < 7; ++j) sigma_ok = sigma_ok && a->sigma[j] >= 0.0 && std::isfinite(a->sigma[j]);
    if (a->P < 1 || a->K < 1 || a->S < 1 || a->S > 256 || a->H < 1 || a->H > 65536 || (int64_t)a->P * a->S * a->H > INT32_MAX ||
        (int64_t)a->P * a->K * a->S > INT32_MAX || a->weather_rows < 1 || !sigma_ok || !(a->phi >= 0.0 && a->phi < 1.0) || !a->weather ||
        !a->w_off_parent || !a->timestep_parent || !a->window) {
        g_err = "glgym_plan_weather: bad arguments (P, K, S, H < 1, S > 256, H > 65 536, P*S*H or P*K*S > INT32_MAX, weather_rows < 1, a sigma "
                "negative or not finite, phi outside [0, 1), or a null weather / w_off_parent / timestep_parent / window)";
        return GLGYM_EINVAL;
    }
    if (!h) { g_err = "glgym_plan_weather: null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->dtype == GLGYM_F32) HIPCHK(plan_weather_launch<float>(*a, h->nd, st));
    else HIPCHK(plan_weather_launch<double>(*a, h->nd, st));
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
    if (h->dtype == GLGYM_F32)
        hipLaunchKernelGGL((rule_based_kernel<float>), grid, block, 0, st, *cfg, a->B, a->ld, (const float*)a->x,
                           (const float*)a->weather, a->weather_rows, a->w_off, a->timestep, a->start_day, a->hour, a->doy,
                           doy_inc, hod_inc, (float*)a->control, h->nd);
    else
        hipLaunchKernelGGL((rule_based_kernel<double>), grid, block, 0, st, *cfg, a->B, a->ld, (const double*)a->x,
                           (const double*)a->weather, a->weather_rows, a->w_off, a->timestep, a->start_day, a->hour,
                           a->doy, doy_inc, hod_inc, (double*)a->control, h->nd);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_timer_start(glgym_handle h, void* stream)
{
    DeviceGuard dev_guard(h);
    if (!h) return GLGYM_EINVAL;
    HIPCHK(hipEventRecord(h->ev0, (hipStream_t)stream));
    return GLGYM_OK;
}

int glgym_timer_stop(glgym_handle h, void* stream, float* elapsed_ms)
{
    DeviceGuard dev_guard(h);
    if (!h || !elapsed_ms) return GLGYM_EINVAL;
    HIPCHK(hipEventRecord(h->ev1, (hipStream_t)stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(elapsed_ms, h->ev0, h->ev1));
    return GLGYM_OK;
}

}  // extern "C"
