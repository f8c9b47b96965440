// glgym.hip -- the integrating gfx950 kernels and the part of the C ABI (include/glgym.h) that launches them.  ONLY what instantiates an
// integrating kernel lives here: every other kernel and its entry points have a translation unit of their own (glgym_env.hip,
// glgym_ancillary.hip, glgym_plan.hip, glgym_search.hip, glgym_rng.hip, glgym_bdf.hip), so that an edit over there neither recompiles nor can change
// the kernels below.  A change to this file owes their instruction-for-instruction comparison (tools/isa_compare.py).
//
// Kernels (one lane = one environment; a 64-lane wavefront = one workgroup = 64 environments):
//   step_kernel   fused TomatoEnv.step(): action->control, weather-row gather, tier-2 precompute,
//                 n_sub x RK4 of the GreenLight ODE (gl_model.hpp), failure check, reward / violation /
//                 info epilogue, terminal test, wave-level metric reduction.   [VALU/transcendental bound]
//                 OBS builds (glgym_step_obs): the same, and each wavefront then also writes the observation rows of its 64 environments
//                 (and, behind them, resets its finished ones: glgym_step_obs_reset) with gl_envlayer.hpp's device functions.
//   step_kernel_quad                          the same step, four lanes per environment (gl_model_quad.hpp).
//   evalf_kernel* / rhs_kernel                row-major double I/O for the reference-compatible evalF and tests.
// Host side: the default-constant image, handle create / destroy / setters, glgym_evalF, glgym_rhs, glgym_step, glgym_step_obs,
// glgym_step_obs_reset, the timer, and the definition of the error string (glgym_internal.h).
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
#include "glgym_internal.h"
#include "gl_envlayer.hpp"

using namespace glm;
using namespace glenv;

thread_local std::string g_err;      // glgym_last_error's string; every TU's entry points write it (glgym_internal.h)

namespace {

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
// registers of the observation epilogue's clamp-free path (step_kernel, OBS builds with default parameters): per pass p the byte offset of
// element q = lane + 64 p inside a forecast window, and one strip's gathered elements
constexpr int OBS_FAST_PASSES = 4;          // nf <= 256: Np <= 51 (the default horizon, Np = 48, has nf = 240)
template <bool ON> struct ObsFastRegs {
    unsigned toff[OBS_FAST_PASSES];
    float fv[OBS_FAST_PASSES][OBS_ROWS];
    int nf, n_full;
    bool fast;
};
template <> struct ObsFastRegs<false> {};
// all gathers of the strip that starts at lane s0 (wave-uniform), issued back to back: row r's window is a scalar base
__device__ __forceinline__ void obs_gather_strip(ObsFastRegs<true>& fr, const float* weather, int nd, int base, int s0)
{
    const char* rowp[OBS_ROWS];
#pragma unroll
    for (int r = 0; r < OBS_ROWS; ++r)
        rowp[r] = reinterpret_cast<const char*>(weather + (size_t)(__builtin_amdgcn_readlane(base, s0 + r) + 1) * nd);
#pragma unroll
    for (int p = 0; p < OBS_FAST_PASSES; ++p) {
        if (p * WAVE < fr.nf) {                 // wave-uniform
            // (the offset is made opaque here so that its zero-extension is not hoisted out of the strip loop as a 64-bit value:
            // scalar base + 32-bit vector offset is one addressing form, base + 64-bit vector a v_lshl_add_u64 per load)
            unsigned t = fr.toff[p];
            asm volatile("" : "+v"(t));
#pragma unroll
            for (int r = 0; r < OBS_ROWS; ++r) fr.fv[p][r] = *reinterpret_cast<const float*>(rowp[r] + t);
        }
    }
}
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
        // ---- the forecast block of a wavefront none of whose windows touches an end of the table (one ballot; every other wavefront
        // takes the clamped strips below for all of its rows).  This launch runs ONE wavefront per SIMD: nothing hides an instruction or
        // a memory round trip of the epilogue, so what does not depend on the row is computed once -- a lane's elements q = lane + 64 p
        // and their byte offsets (i * nd + c) * 4 inside a window -- a row is a scalar base, a gathered element one load with that
        // base and no vector address arithmetic, and all of a strip's gathers (OBS_ROWS x OBS_FAST_PASSES per lane) are in flight
        // together: the first strip's from here, across the core features, the next strip's across the streaming-out of the current one.
        // Compiled into the default-parameter builds only: in the handle-parameter builds, whose integrator the compiler fits into 256 +
        // 150-200 registers, this code moved the register allocation of the sub-step loops, and they keep the epilogue they had.
        ObsFastRegs<DEFAULT_P> fr;
        if constexpr (DEFAULT_P) {
            fr.nf = o.moff[5] >= 0 ? 5 * o.Np : 0;
            fr.n_full = min(WAVE, a.B - b0) / OBS_ROWS;     // wave-uniform
            fr.fast = fr.nf > 0 && fr.nf <= OBS_FAST_PASSES * WAVE && fr.n_full > 0 &&
                      __builtin_amdgcn_ballot_w64(base < -1 || base >= a.weather_rows - o.Np) == 0;
            if (fr.fast) {
#pragma unroll
                for (int p = 0; p < OBS_FAST_PASSES; ++p) {  // lanes past nf re-read element nf - 1 and do not write it
                    const int q = min(lane + p * WAVE, fr.nf - 1), i = q / 5;
                    fr.toff[p] = (unsigned)(i * a.nd + (q - i * 5)) * 4u;
                }
                obs_gather_strip(fr, a.weather, a.nd, base, 0);
            }
        }
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
        int s_begin = 0;
        if constexpr (DEFAULT_P) if (fr.fast) {
            // the features that are a loaded value as it stands (controls, weather) have arrived before the strip loop: a wait for
            // them inside it would, from the second strip on, wait for the stores of the strip before
#pragma unroll
            for (int j = 0; j < OBS_NCORE; ++j) asm volatile("" : : "v"(f[j]));
            // full strips of a clamp-free wavefront: no per-row branch anywhere; the ragged last strip, if any, is left to the loop below
            for (int s0 = 0; s0 < fr.n_full * OBS_ROWS; s0 += OBS_ROWS) {
                const int r_me = lane - s0;
                if (r_me >= 0 && r_me < OBS_ROWS) {
#pragma unroll
                    for (int j = 0; j < OBS_NCORE; ++j) {
                        const int mo = o.moff[obs_core_module(j)];
                        if (mo >= 0) span[r_me * dim + mo + obs_core_col(j)] = f[j];
                    }
                }
#pragma unroll
                for (int p = 0; p < OBS_FAST_PASSES; ++p) {
                    const int q = lane + p * WAVE;
                    if (q < fr.nf) {
#pragma unroll
                        for (int r = 0; r < OBS_ROWS; ++r) span[r * dim + o.moff[5] + q] = fr.fv[p][r];
                    }
                }
                if (s0 + OBS_ROWS < fr.n_full * OBS_ROWS) obs_gather_strip(fr, a.weather, a.nd, base, s0 + OBS_ROWS);     // into the registers just written out
                __syncthreads();
                // the span, 16 bytes per lane: OBS_STREAM_DEPTH LDS reads in flight before the stores that consume them
                constexpr int OBS_STREAM_DEPTH = 8;
                const int n4 = (OBS_ROWS * dim) >> 2;
                const v4f* src4 = reinterpret_cast<const v4f*>(span);
                v4f* dst4 = reinterpret_cast<v4f*>(o.obs + (size_t)(b0 + s0) * dim);
                int c0 = 0;                                 // wave-uniform
                for (; c0 + OBS_STREAM_DEPTH * WAVE <= n4; c0 += OBS_STREAM_DEPTH * WAVE) {
                    v4f t[OBS_STREAM_DEPTH];
#pragma unroll
                    for (int k = 0; k < OBS_STREAM_DEPTH; ++k) t[k] = src4[c0 + k * WAVE + lane];
#pragma unroll
                    for (int k = 0; k < OBS_STREAM_DEPTH; ++k) __builtin_nontemporal_store(t[k], &dst4[c0 + k * WAVE + lane]);
                }
                for (int e = c0 + lane; e < n4; e += WAVE) __builtin_nontemporal_store(src4[e], &dst4[e]);
                __syncthreads();
            }
            s_begin = fr.n_full * OBS_ROWS;
        }
        for (int s0 = s_begin; s0 < n_live; s0 += OBS_ROWS) {     // wave-uniform
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
                                                     const double* crop, int B, T dt, int n_sub, double gasR, double tCanMin,
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
        // the row's crop constants from its double block, rounded to T once: what make_model_const computes on the host for a shared
        // block, so that a block gives the same constants whether it arrives per row or as the handle's (tests/test_gpu_evalf_builds.py)
        double pc[NCROP];
        for (int i = 0; i < NCROP; ++i) pc[i] = crop[(size_t)b * NCROP + i];
        make_crop_const<T, double>(pc, gasR, tCanMin, crLocal);
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
        x_next[(size_t)b * NX + i] = failed ? __builtin_nan("") : x[(size_t)b * NX + i] + (double)del[i];      // the caller's x: include/glgym.h
    if (failed) atomicAdd(n_failed, 1);
}

}  // namespace

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
// the handle's constants in the precision of with_dtype's tag (glgym_internal.h)
static const ModelConst<float>& model_const(glgym_handle h, float) { return h->mf; }
static const ModelConst<double>& model_const(glgym_handle h, double) { return h->md; }
static const RewardConstBase<float>& reward_const(glgym_handle h, float) { return h->rf; }
static const RewardConstBase<double>& reward_const(glgym_handle h, double) { return h->rd; }

// The evalF launcher: the build is chosen by glsel::select_evalf (gl_step_select.hpp, where the rules and the list of builds are) and
// mapped to its kernel through that list.
template <class T>
static int run_evalf(glgym_handle h, const ModelConst<T>& m, const double* p_used, const double* dx, const double* du,
                     const double* dd, const double* dcrop, int B, double* dout, int rhs_only)
{
    const int pipe = h->variant == GLGYM_ODE_PIPE ? 1 : 0;
    if (rhs_only) {                      // the right-hand side at one state per row (test hook): one lane per row in either dtype
        const dim3 grid((B + WAVE - 1) / WAVE), block(WAVE);
        if (pipe) hipLaunchKernelGGL((rhs_kernel<T, false, true>), grid, block, 0, (hipStream_t)0, dx, du, dd, dcrop, B, T(p_used[39]), T(p_used[162]), m, dout, h->nd);
        else if (dcrop) hipLaunchKernelGGL((rhs_kernel<T, true, false>), grid, block, 0, (hipStream_t)0, dx, du, dd, dcrop, B, T(p_used[39]), T(p_used[162]), m, dout, h->nd);
        else hipLaunchKernelGGL((rhs_kernel<T, false, false>), grid, block, 0, (hipStream_t)0, dx, du, dd, dcrop, B, T(p_used[39]), T(p_used[162]), m, dout, h->nd);
        HIPCHK(hipGetLastError());
        return GLGYM_OK;
    }
    const int verify = h->verify_mode != GLGYM_VERIFY_NEVER;
    glsel::EvalfSelectIn in;
    in.f64 = sizeof(T) == 8; in.scheme = h->scheme; in.pipe = pipe != 0; in.crop = dcrop != nullptr; in.layout = h->layout;
    in.B = B; in.n_simd = h->n_simd; in.verify = verify != 0; in.ladder_parallel = h->ladder_parallel != 0;
    const glsel::EvalfChoice c = glsel::select_evalf(in);
    if (c.error) { g_err = c.error; return GLGYM_EINVAL; }
    const dim3 grid(c.grid), block(WAVE);
    const glsel::EvalfBuild& b = c.build;
    const auto go = [&](auto kernel, auto gasR, auto tCanMin, auto... tail) {
        hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)0, dx, du, dd, dcrop, B, T(h->dt), h->n_sub, gasR, tCanMin, m, dout, tail...);
    };
    bool launched = false;
    with_scheme(b.sch, [&](auto sch) {
        constexpr int SCH = decltype(sch)::value;
#define GL_LAUNCH_QUAD(F64, PIPE, CROP, PAIR)                                                                                         \
        if constexpr (F64 == (sizeof(T) == 8))                                                                                       \
            if (!launched && b == glsel::EvalfBuild{PAIR ? glsel::QUAD_PAIR : glsel::QUAD, F64, CROP, PIPE, SCH}) {                   \
                go(evalf_kernel_quad<T, SCH, PIPE, CROP, PAIR>, T(p_used[39]), T(p_used[162]), h->nd, h->fail_dev, verify, pipe, h->window); \
                launched = true;                                                                                                     \
            }
        GL_EVALF_QUAD_BUILDS(GL_LAUNCH_QUAD)
#undef GL_LAUNCH_QUAD
#define GL_LAUNCH_ONE(CROP, PIPE)                                                                                                     \
        if constexpr (sizeof(T) == 4 && glsel::one_lane_build_exists(PIPE, SCH))                                                     \
            if (!launched && b == glsel::EvalfBuild{glsel::ONE_LANE, false, CROP, PIPE, SCH}) {                                      \
                go(evalf_kernel<T, CROP, PIPE, SCH>, p_used[39], p_used[162], 0, h->nd, h->fail_dev, verify, h->window); \
                launched = true;                                                                                                     \
            }
        GL_EVALF_ONE_LANE_BUILDS(GL_LAUNCH_ONE)
#undef GL_LAUNCH_ONE
    });
    // unreachable: every build select_evalf returns is in the lists (tests/test_step_select_host.py asserts it over the full product)
    if (!launched) { g_err = "glgym_evalF: no kernel was built for the selected configuration (gl_step_select.hpp)"; return GLGYM_EINVAL; }
    HIPCHK(hipGetLastError());
    h->last_evalf = c; h->last_evalf_pipe = pipe; h->last_evalf_rows = B; h->has_last_evalf = true;
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
        h->last_evalf = glsel::EvalfChoice{nullptr, {-1, false, false, false, 0}, 0}; h->last_evalf_pipe = 0; h->last_evalf_rows = B;
        h->has_last_evalf = true;
    } else {
        rc = with_dtype(h->dtype, [&](auto t) {
            using T = decltype(t);
            ModelConst<T> m = model_const(h, t);
            if (p) make_model_const<T>(p_used, m);
            return run_evalf<T>(h, m, p_used, dx, du, dd, dcrop, B, dout, rhs_only);
        });
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

int glgym_last_evalf_build(glgym_handle h, int32_t out[8])
{
    if (!h || !out) { g_err = "glgym_last_evalf_build: null handle / output"; return GLGYM_EINVAL; }
    if (!h->has_last_evalf) { g_err = "glgym_last_evalf_build: the handle has not launched a glgym_evalF yet"; return GLGYM_EINVAL; }
    const glsel::EvalfBuild& b = h->last_evalf.build;
    const int32_t v[8] = {b.family, b.f64, b.crop, b.pipe, h->last_evalf_pipe, b.sch, (int32_t)h->last_evalf.grid, h->last_evalf_rows};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return GLGYM_OK;
}

}  // extern "C"

// ---- device-pointer hot path ----------------------------------------------------------------------
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
static int launch_step(glgym_handle h, const glgym_step_args* a, const ModelConst<T>& m, const RewardConstBase<T>& rw_base,
                       hipStream_t st, const glgym_obs_args* oa = nullptr, int* fused = nullptr, const glgym_reset_args* ra = nullptr)
{
    const RewardConst<T> rw{rw_base};       // the kernels' own argument type (their names carry it); the handle stores the base
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
    h->last_step = c; h->has_last_step = true;
    if (c.fused && fused) *fused = c.fused;
    return GLGYM_OK;
}

// glgym_set_step_integrator(h, GLGYM_INTEGRATOR_BDF): one wavefront per environment in glgym_bdf.hip, fp64 integration for either dtype
template <class T>
static int launch_step_bdf(glgym_handle h, const glgym_step_args* a, const RewardConstBase<T>& rw, hipStream_t st)
{
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
    h->last_step = glsel::StepChoice{nullptr, {-1, false, false, false, false, 0, 0, 0}, 0, 0}; h->has_last_step = true;
    return GLGYM_OK;
}

// What glgym_step refuses, all of it, decided on the host before anything is launched: GLGYM_OK, or GLGYM_EINVAL with the text in g_err.
// step_impl begins with it; the rollouts of glgym_plan.hip call it on the step block they are about to use, before their first prologue
// (glgym_internal.h).
int step_refusal(glgym_handle h, const glgym_step_args* a)
{
    if (!h || !a) return refuse("glgym_step: null handle / arguments");
    if (a->struct_size != (int32_t)sizeof(glgym_step_args))       // checked before any pointer member is read
        return refuse("glgym_step: glgym_step_args.struct_size is " + std::to_string(a->struct_size) + ", this library expects " +
                      std::to_string(sizeof(glgym_step_args)) + " (ABI " + std::to_string(GLGYM_ABI_VERSION) + "): rebuild against include/glgym.h");
    if (a->B < 1 || a->ld < a->B || !a->x || !a->u || !a->weather || !a->w_off || !a->timestep ||
        !a->reward || !a->done || (!a->action) == (!a->control) || a->weather_rows < 1)
        return refuse("glgym_step: bad arguments (exactly one of action/control, ld >= B, non-null state/outputs)");
    const bool pipe = h->variant == GLGYM_ODE_PIPE;
    if (h->step_integrator == GLGYM_INTEGRATOR_BDF)
        return pipe ? refuse("glgym_step: GLGYM_INTEGRATOR_BDF does not support GLGYM_ODE_PIPE") : (int)GLGYM_OK;
    if (h->integrator != GLGYM_INTEGRATOR_EXPLICIT)
        return refuse("glgym_step: GLGYM_INTEGRATOR_BDF is available to glgym_evalF only; set GLGYM_INTEGRATOR_EXPLICIT for env-steps");
    const char* why = glsel::step_pipe_error(pipe, a->crop_p != nullptr, h->scheme);
    return why ? refuse(why) : (int)GLGYM_OK;
}

static int step_impl(glgym_handle h, const glgym_step_args* a, void* stream, const glgym_obs_args* oa, int* fused,
                     const glgym_reset_args* ra = nullptr)
{
    if (const int rc = step_refusal(h, a)) return rc;
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    if (h->step_integrator == GLGYM_INTEGRATOR_BDF)
        return with_dtype(h->dtype, [&](auto t) { return launch_step_bdf<decltype(t)>(h, a, reward_const(h, t), st); });
    return h->dtype == GLGYM_F32 ? launch_step<float>(h, a, h->mf, h->rf, st, oa, fused, ra)
                                 : launch_step<double>(h, a, h->md, h->rd, st);
}

extern "C" int glgym_step(glgym_handle h, const glgym_step_args* a, void* stream)
{
    return step_impl(h, a, stream, nullptr, nullptr);
}

extern "C" {

int glgym_last_step_build(glgym_handle h, int32_t out[10])
{
    if (!h || !out) { g_err = "glgym_last_step_build: null handle / output"; return GLGYM_EINVAL; }
    if (!h->has_last_step) { g_err = "glgym_last_step_build: the handle has not launched an env-step yet"; return GLGYM_EINVAL; }
    const glsel::StepBuild& b = h->last_step.build;
    const int32_t v[10] = {b.family, b.f64, b.crop, b.def, b.pipe, b.sch, b.epi, b.occ, (int32_t)h->last_step.grid, h->last_step.fused};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return GLGYM_OK;
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
