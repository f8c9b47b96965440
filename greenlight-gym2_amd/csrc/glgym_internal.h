// glgym_internal.h -- what the C entry points of every translation unit share: the handle, the thread-local error string behind
// glgym_last_error, HIPCHK, DeviceGuard, the dtype dispatch and the host helpers of the observation / reset argument blocks.  Host code
// only: nothing in here ends up in a kernel.  (No using-directive for glm:: -- glgym_plan.hip, glgym_search.hip and glgym_rng.hip have
// NX / NU / NCROP of their own.)
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "glgym.h"
#include "gl_model.hpp"
#include "gl_reward.hpp"
#include "gl_step_select.hpp"

extern thread_local std::string g_err;      // defined in glgym.hip

#define HIPCHK(expr)                                                                                   \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                                 \
            return GLGYM_EHIP;                                                                         \
        }                                                                                              \
    } while (0)

// ---------------------------------------------------------------------------------------------------
// handle
// ---------------------------------------------------------------------------------------------------
struct glgym_handle_s {
    int device = 0;
    int dtype = GLGYM_F32;
    int n_sub = 256;
    double dt = 900.0;
    double p[glm::NP];
    glm::ModelConst<float> mf;
    glm::ModelConst<double> md;
    glgym_reward_cfg rcfg;
    glm::RewardConstBase<float> rf;     // (the base: RewardConst<T>, which the step kernels' names carry, is glgym.hip's own)
    glm::RewardConstBase<double> rd;
    double max_profit = 0, min_profit = 0, fixed_costs = 0;
    float* p0_crop_dev = nullptr;       // shared p[128..161] as f32 (noise kernel input)
    int* fail_dev = nullptr;            // glgym_evalF: number of rows whose integration failed
    int nd = glm::ND;                   // weather / disturbance row stride: 10, or up to 16 (ODE_pipe reads columns 10, 12)
    int variant = GLGYM_ODE;            // GLGYM_ODE | GLGYM_ODE_PIPE
    int scheme = GLGYM_SCHEME_RK4;      // GLGYM_SCHEME_RK4 | GLGYM_SCHEME_RK2 | GLGYM_SCHEME_RK3
    int verify_mode = GLGYM_VERIFY_AUTO;   // glgym_set_verify
    int use_specialised = 1;            // GLGYM_GENERIC=1 in the environment forces the generic kernels (A/B tests)
    int window = 0;                     // glgym_set_window: 0 = the scheme's own
    int layout = GLGYM_LAYOUT_AUTO;     // glgym_set_layout (fp32); initial value from GLGYM_LAYOUT at glgym_create
    int occupancy = 0;                  // glgym_set_occupancy (one-lane fp32 kernel): 0 = by batch size; initial value from GLGYM_OCC at glgym_create
    int ladder_parallel = 1;            // glgym_set_ladder_parallel: verified glgym_evalF calls may run two rungs of the ladder side by side
    int n_simd = 1024;                  // SIMDs of the device (4 per CU)
    glsel::StepChoice last_step{};      // what the last env-step launched (glgym_last_step_build); family -1: a BDF env-step
    bool has_last_step = false;
    glsel::EvalfChoice last_evalf{};    // what the last glgym_evalF launched (glgym_last_evalf_build); family -1: a BDF call
    int last_evalf_pipe = 0, last_evalf_rows = 0;      // whether that launch integrated ODE_pipe; its rows
    bool has_last_evalf = false;
    float du = 0.1f, u_min[glm::NU] = {0, 0, 0, 0, 0, 0}, u_max[glm::NU] = {1, 1, 1, 1, 1, 1};   // glgym_set_control_limits
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

// What glgym_step refuses, decided without launching anything (glgym.hip, where glgym_step begins with it): GLGYM_OK, or GLGYM_EINVAL
// with glgym_step's text in g_err.  The rollouts of glgym_plan.hip ask it before their first prologue.  Not part of the C ABI.
__attribute__((visibility("hidden"))) int step_refusal(glgym_handle h, const glgym_step_args* a);

// g_err = why, and the GLGYM_EINVAL an entry point returns with it
static inline int refuse(std::string why)
{
    g_err = std::move(why);
    return GLGYM_EINVAL;
}

// struct_size of an argument block against this library's; `who` begins the message (the planning and search entry points)
static inline bool plan_size_ok(const char* who, int32_t got, size_t want)
{
    if (got == (int32_t)want) return true;
    g_err = std::string(who) + ": struct_size is " + std::to_string(got) + ", this library expects " + std::to_string(want) +
            " (ABI " + std::to_string(GLGYM_ABI_VERSION) + "): rebuild against include/glgym.h";
    return false;
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

// the handle's dtype as a type: f(float{}) or f(double{}), and what f returns (with_scheme's sibling; here because every TU dispatches)
template <class F> static auto with_dtype(int dtype, F&& f)
{
    if (dtype == GLGYM_F32) return f(float{});
    return f(double{});
}

constexpr int OBS_MAX_NP = 128;         // obs_kernel's LDS span = rows * (23 + 5 Np) floats <= 42 KB
constexpr int OBS_MODULE_SIZE[6] = {4, 3, 6, 5, 5, 0};      // observations.py:64,84,102,123,143; forecast = 5 * Np (:168)
// first column of each observation module in the handle's module order (-1 = absent) and the row width
inline void obs_layout(glgym_handle h, int Np, int moff[6], int* dim)
{
    for (int m = 0; m < 6; ++m) moff[m] = -1;
    *dim = 0;
    for (int i = 0; i < h->n_obs_modules; ++i) {
        const int m = h->obs_modules[i];
        moff[m] = *dim;
        *dim += m == GLGYM_OBS_FORECAST ? 5 * Np : OBS_MODULE_SIZE[m];
    }
}
inline void obs_clock_increments(glgym_handle h, double* doy_inc, double* hod_inc)
{
    *doy_inc = std::fmod(h->dt / 86400.0, 365.0);
    *hod_inc = h->dt / 3600.0;
}
inline bool obs_args_ok(glgym_handle h, const glgym_obs_args* a)
{
    return h && a && a->B >= 1 && a->ld >= a->B && a->x && a->u && a->weather && a->weather_rows >= 1 && a->w_off && a->timestep &&
           a->start_day && a->obs && a->Np >= 0 && a->Np <= OBS_MAX_NP;      // weather_rows < 1: the row clamp would yield row -1
}
inline bool reset_args_ok(const glgym_reset_args* a)
{
    return a && a->B >= 1 && a->ld >= a->B && a->x && a->u && a->timestep && a->weather && a->weather_rows >= 1 && a->w_off;
}
