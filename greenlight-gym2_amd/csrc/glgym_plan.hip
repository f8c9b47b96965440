// glgym_plan.hip -- the part of device-side planning that drives env-steps (include/glgym.h glgym_plan_fork .. _rollout_policy), kernels and
// C entry points: fork children from parent environments, accumulate a step's reward into the children's returns, the scenario and
// weather prologues, the rule and policy rows, and the four rollouts.  What ranks and searches over the finished returns is
// glgym_search.hip.  The scalar logic is the gl_*.hpp headers' (gl_plan.hpp instantiated on the host by tests/planhost/planhost.cpp); the
// env-steps in between are glgym_step's own kernels (glgym.hip), reached through the C ABI -- nothing of them is instantiated or fused
// here, and what glgym_step refuses is asked of glgym.hip's step_refusal, never restated.  Each entry point checks its arguments and
// launches its kernels itself, at the bottom of this file.
//
// Layouts.  fork / accumulate: one lane per child; every child-side access is coalesced (SoA planes, lane c at base[i*ld + c]), the
// parent side of a fork is a broadcast read (the K children of a parent sit in adjacent lanes and read one address).  No LDS; no
// kernel here uses atomics, all stores are plain vector stores.
//
// Robust planning's prologue (glgym_plan_scenario; scalar logic in gl_scen.hpp, instantiated on the host by tests/scenhost/scenhost.cpp):
// lane = child, the prologue of one env-step of a scenario rollout -- the child's crop block for this step and its row of the expanded
// action plane.
//
// Weather-forecast scenarios (glgym_plan_weather; scalar logic in gl_wscen.hpp, instantiated on the host by
// tests/wscenhost/wscenhost.cpp).  window: lane = (greenhouse-scenario ps, j') with j' < 8 fastest; lanes 0..6 run their column's
// error recurrence over the horizon -- sequential in h by its nature, one Philox block per step --, lane 7 copies the columns the
// model leaves alone, so that eight adjacent lanes write one contiguous row of nd values per step and a wavefront eight rows.  The
// source rows are shared by the S scenarios of a greenhouse (L2 hits).  No LDS: nothing is exchanged between lanes.  The child
// offsets are a second launch, lane = child.
//
// Closed-loop rule-based rollouts (glgym_rule_rows / glgym_plan_rollout_rule; scalar logic in gl_rule.hpp, instantiated on the host by
// tests/rulehost/rulehost.cpp).  rows: lane = row, the rule-based controller with the row's own 29 constants, decoded from its row of
// the candidates' parameter block.  The rollout is rollout_steps with that kernel (after the scenario prologue, if any) in front of
// every env-step, writing the control plane the step then reads.
//
// Closed-loop neural-policy rollouts (glgym_policy_rows / glgym_plan_rollout_policy; scalar logic in gl_mlp.hpp, instantiated on the host
// by tests/mlphost/mlphost.cpp).  rows: lane = row, one wavefront per block, the MLP with the row's own weights.  A lane's activations
// live in LDS as [neuron][lane] -- a wavefront's access to one neuron is 64 consecutive floats, conflict-free, and no lane ever reads
// another lane's column, so there is no barrier -- in two buffers sized by the net (at most 2 x 64 x 64 floats = 32 KB); nothing is
// indexed by a run-time value in registers, so there is no scratch.  Weights are read once, in the order of the flat parameter vector:
// 6 consecutive floats per lane and plane, neighbouring rows adjacent, lanes that share a row one address, four planes in flight; the walk (gl_mlp.hpp dot)
// is the same for all lanes and stays in scalar registers.  The rollout is rollout_steps with glgym_obs and that kernel (after the
// scenario prologue, if any) in front of every env-step, writing the action plane the step then reads.
#include <cmath>
#include <string>

#include "glgym_internal.h"

#include "gl_mlp.hpp"
#include "gl_plan.hpp"
#include "gl_rule.hpp"
#include "gl_scen.hpp"
#include "gl_wscen.hpp"

namespace {

constexpr int NX = GLGYM_NX, NU = GLGYM_NU, NCROP = GLGYM_NCROP;
constexpr int WAVE = glplan::WAVE;

template <class T>
__global__ __launch_bounds__(256) void plan_fork_kernel(glgym_plan_fork_args a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.n_children) return;
    int p = a.parent ? a.parent[c] : c / a.K;
    const bool bad = p < 0 || p >= a.n_parents;
    if (bad) p = 0;
    const size_t ldp = (size_t)a.ld_parent, ldc = (size_t)a.ld_child;
    const T* xp = (const T*)a.x_parent;
    T* x = (T*)a.x;
    for (int i = 0; i < NX; ++i) x[i * ldc + c] = xp[i * ldp + p];
    const T* up = (const T*)a.u_parent;
    T* u = (T*)a.u;
    for (int i = 0; i < NU; ++i) u[i * ldc + c] = up[i * ldp + p];
    if (a.crop && a.crop_parent) {
        const T* cp = (const T*)a.crop_parent;
        T* cc = (T*)a.crop;
        for (int i = 0; i < NCROP; ++i) cc[i * ldc + c] = cp[i * ldp + p];
    }
    a.timestep[c] = a.timestep_parent[p];
    a.w_off[c] = a.w_off_parent[p];
    if (a.start_day && a.start_day_parent) a.start_day[c] = a.start_day_parent[p];
    a.ret[c] = 0.0;
    for (int i = 0; i < 3; ++i) a.viol[i * ldc + c] = 0.0;
    a.n_steps[c] = 0;
    a.alive[c] = bad ? 0 : 1;
    a.failed[c] = bad ? 1 : 0;
}

template <class T>
__global__ __launch_bounds__(256) void plan_accumulate_kernel(glgym_plan_accumulate_args a)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.B) return;
    uint8_t alive = a.alive[c];
    if (!alive) return;
    const size_t ld = (size_t)a.ld;
    const T* info = (const T*)a.info;
    double ret = a.ret[c], v0 = a.viol[c], v1 = a.viol[ld + c], v2 = a.viol[2 * ld + c];
    int32_t n = a.n_steps[c];
    uint8_t failed = a.failed[c];
    glplan::accumulate(ret, v0, v1, v2, n, alive, failed, a.w, (double)((const T*)a.reward)[c],
                       (double)info[glplan::INFO_CO2 * ld + c], (double)info[glplan::INFO_TEMP * ld + c],
                       (double)info[glplan::INFO_RH * ld + c], a.done[c], a.step_flags ? a.step_flags[c] : 0);
    a.ret[c] = ret;
    a.viol[c] = v0; a.viol[ld + c] = v1; a.viol[2 * ld + c] = v2;
    a.n_steps[c] = n;
    a.alive[c] = alive;
    a.failed[c] = failed;
}

// grid = ceil(C / 256), lane = child c = (p*K + k)*S + s: nine Philox blocks keyed by (p*S + s, step) -- the S children of a candidate
// draw S different futures, the K candidates of a greenhouse the same S -- then 34 plane stores, coalesced along c; with an action
// plane, the candidate's row is copied to the child's row of the staging plane (6 consecutive floats per lane, 1 536 contiguous
// bytes per wavefront; the S children of a candidate read one row, a broadcast).
template <class T>
__global__ __launch_bounds__(256) void plan_scenario_kernel(glgym_plan_scenario_args a, const float* p0, int n_children)
{
    const int64_t c64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;      // n_children may be INT32_MAX: the last block's tail is not
    if (c64 >= n_children) return;
    const int c = (int)c64;
    uint32_t ps;
    int cand;
    glscen::split_child(c, a.K, a.S, &ps, &cand);
    const uint64_t D = a.draw_index + (a.draw_base ? *a.draw_base : 0ull);
    float v[glscen::NCROP];
    glscen::crop_block(ps, a.h_step, a.hold, D, a.seed, a.scale, p0, v);
    T* crop = (T*)a.crop;
    const size_t ld = (size_t)a.ld;
#pragma unroll
    for (int i = 0; i < glscen::NCROP; ++i) crop[i * ld + c] = (T)v[i];
    if (a.actions_in) {
        const float* in = a.actions_in + (size_t)cand * NU;
        float* out = a.actions_out + (size_t)c * NU;
        for (int j = 0; j < NU; ++j) out[j] = in[j];
    }
}

// grid = ceil(P*S*8 / 256), lane = ps*8 + j'.  P*S*8 may pass 2^31: the index is taken in 64 bits, the last block's tail does nothing.
template <class T>
__global__ __launch_bounds__(256) void plan_weather_kernel(glgym_plan_weather_args a, int nd, double innov, int64_t n_lanes)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_lanes) return;
    const uint32_t ps = (uint32_t)(t / glwscen::LANES);
    const int jj = (int)(t - (int64_t)ps * glwscen::LANES);
    const uint64_t D = a.draw_index + (a.draw_base ? *a.draw_base : 0ull);
    glwscen::window_lane<T>(ps, jj, a.S, a.H, nd, (const T*)a.weather, a.weather_rows, a.w_off_parent, a.timestep_parent, a.sigma, a.phi, innov,
                            D, a.seed, (T*)a.window);
}

// grid = ceil(C / 256), lane = child c = (p*K + k)*S + s
__global__ __launch_bounds__(256) void plan_weather_offsets_kernel(glgym_plan_weather_args a, int n_children)
{
    const int64_t c64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c64 >= n_children) return;
    const int c = (int)c64;
    uint32_t ps;
    int cand;
    glscen::split_child(c, a.K, a.S, &ps, &cand);
    a.w_off_child[c] = glwscen::child_offset(ps, a.H, a.timestep_parent[cand / a.K]);
}

// grid = ceil(B / 256), lane = row b.  The row's 29 constants are decoded from theta row b / max(S, 1) into registers (the space comes
// by field, gl_rule.hpp: no run-time field index); the theta reads are 6 consecutive floats per row and plane, the S children of a
// candidate read one row (a broadcast).  x, the clocks and the six control planes are coalesced along b; the weather row is a gather.
template <class T>
__global__ __launch_bounds__(256) void rule_rows_kernel(glrule::Space sp, const float* __restrict__ theta, int J, int S, int B, int ld,
                                                        const T* __restrict__ x, const T* __restrict__ weather, int weather_rows,
                                                        const int* __restrict__ w_off, const int* __restrict__ timestep,
                                                        const float* __restrict__ start_day, const double* hour, const double* doy_in,
                                                        double doy_inc, double hod_inc, T* __restrict__ control, int nd)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int ts = timestep[b];
    int row = w_off[b] + ts;
    row = row >= weather_rows ? weather_rows - 1 : (row < 0 ? 0 : row);
    const T* w = weather + (size_t)row * nd;
    const double hod = hour ? hour[b] : fmod((double)ts * hod_inc, 24.0);
    const double doy = doy_in ? doy_in[b] : (double)start_day[b] + (double)ts * doy_inc;
    double c[glrule::NF], u[NU];
    glrule::row_cfg(sp, theta, J, glrule::theta_row(b, S), c);
    glrule::controls(c, (double)w[0], (double)w[1], (double)w[7], (double)w[8], (double)w[9], (double)x[b], (double)x[(size_t)2 * ld + b],
                     (double)x[(size_t)15 * ld + b], hod, doy, u);
#pragma unroll
    for (int i = 0; i < NU; ++i) control[(size_t)i * ld + b] = (T)u[i];
}

// grid = ceil(B / 64) blocks of one wavefront, lane = row b; dynamic LDS = 2 * rows * 64 floats, rows = glmlp::buffer_rows(net).  Float k
// of buffer `which` of this lane is lds[(which * rows + k) * 64 + lane].  No barrier: a lane touches its own column only.
__global__ __launch_bounds__(WAVE) void policy_rows_kernel(glgym_mlp_net net, int rows, const float* __restrict__ obs,
                                                           const float* __restrict__ theta, int J, int S, int mode, int B,
                                                           float* __restrict__ action)
{
    extern __shared__ float policy_lds[];
    const int b = blockIdx.x * WAVE + threadIdx.x;
    if (b >= B) return;
    float* mine = policy_lds + threadIdx.x;
    auto buf = [mine, rows](int which, int k) -> float& { return mine[(which * rows + k) * WAVE]; };
    const int j = glmlp::policy_row(b, S, J, mode);
    float a[NU];
    glmlp::forward(net, obs + (size_t)b * (size_t)net.in_dim, theta + (size_t)j * NU, (size_t)J * NU, buf, a);
#pragma unroll
    for (int i = 0; i < NU; ++i) action[(size_t)b * NU + i] = a[i];
}

}  // namespace

// The loop of glgym_plan_rollout and glgym_plan_rollout_scenarios: per horizon step k the caller's prologue(k) -- it points s at the step's
// actions, or launches the scenario prologue --, glgym_step, then glgym_plan_accumulate with the weight gamma^k.  The first refusal ends it.
template <class F>
static int rollout_steps(glgym_handle h, glgym_step_args& s, const glgym_plan_rollout_args& r, void* stream, F&& prologue)
{
    glgym_plan_accumulate_args acc;
    acc.struct_size = (int32_t)sizeof acc;
    acc.B = s.B; acc.ld = s.ld; acc.reward = s.reward; acc.info = s.info; acc.done = s.done; acc.step_flags = s.step_flags;
    acc.ret = r.ret; acc.viol = r.viol; acc.n_steps = r.n_steps; acc.alive = r.alive; acc.failed = r.failed;
    double w = 1.0;
    for (int k = 0; k < r.H; ++k) {
        int rc = prologue(k);
        if (rc != GLGYM_OK) return rc;
        if ((rc = glgym_step(h, &s, stream)) != GLGYM_OK) return rc;
        acc.w = w;
        if ((rc = glgym_plan_accumulate(h, &acc, stream)) != GLGYM_OK) return rc;
        w = w * r.gamma;
    }
    return GLGYM_OK;
}

// ---- what the rollouts check and build alike, once each.  `who` is the entry point's name: every message begins with it. ----
static bool scenario_shape_ok(int32_t P, int32_t K, int32_t S, int32_t hold, double scale)
{
    return P >= 1 && K >= 1 && S >= 1 && S <= 256 && (int64_t)P * K * S <= INT32_MAX && (hold == 0 || hold == 1) && scale >= 0.0 &&
           std::isfinite(scale);
}

static bool horizon_ok(const char* who, int32_t H, double gamma)
{
    if (H >= 1 && gamma >= 0.0 && std::isfinite(gamma)) return true;
    g_err = std::string(who) + ": H < 1, or gamma negative or not finite";
    return false;
}

// what glgym_plan_accumulate reads and writes: the step's reward / info / done and the five accumulators
static bool outputs_ok(const char* who, const glgym_plan_rollout_args& r)
{
    if (r.step.reward && r.step.info && r.step.done && r.ret && r.viol && r.n_steps && r.alive && r.failed) return true;
    g_err = std::string(who) + ": null reward / info / done / accumulators";
    return false;
}

static bool scenario_count_ok(const char* who, int32_t S)
{
    if (S >= 0 && S <= 256) return true;
    g_err = std::string(who) + ": S outside 0 .. 256";
    return false;
}

// a closed-loop rollout with S >= 1 (A: its argument block); J must be j_want, which j_rule puts in words
template <class A>
static bool with_scenarios_ok(const char* who, const A& a, int32_t H, const glgym_step_args& s, int64_t j_want, const char* j_rule)
{
    if (scenario_shape_ok(a.P, a.K, a.S, a.hold, a.scale) && H <= 65536 && (int64_t)s.B == (int64_t)a.P * a.K * a.S &&
        (int64_t)a.J == j_want && s.crop_p)
        return true;
    g_err = std::string(who) + ": with scenarios P, K >= 1, hold 0 | 1, scale finite and >= 0, H <= 65 536, step.B == P*K*S, " + j_rule +
            " and a crop block (step.crop_p) are needed";
    return false;
}

// the scenario prologue's arguments from a rollout's block (A: any of the three) and its step; h_step is set per step, actions_in / _out
// by the rollout that expands an action plane
template <class A>
static glgym_plan_scenario_args scenario_args_of(const A& a, const glgym_step_args& s)
{
    glgym_plan_scenario_args sc;
    sc.struct_size = (int32_t)sizeof sc;
    sc.P = a.P; sc.K = a.K; sc.S = a.S; sc.ld = s.ld; sc.hold = a.hold; sc.scale = a.scale; sc.seed = a.seed;
    sc.draw_index = a.draw_index; sc.draw_base = a.draw_base; sc.crop = (void*)s.crop_p; sc.actions_in = nullptr; sc.actions_out = nullptr;
    return sc;
}

// the scenario prologue of horizon step k; nothing without scenarios (S = 0)
static int scenario_prologue(glgym_handle h, glgym_plan_scenario_args& sc, int k, void* stream)
{
    sc.h_step = k;
    return sc.S >= 1 ? glgym_plan_scenario(h, &sc, stream) : (int)GLGYM_OK;
}

extern "C" {

// ---- the C entry points: argument checks, the launches, and the rollouts' loop over glgym_step (glgym.hip's, through the C ABI) ----
int glgym_plan_fork(glgym_handle h, const glgym_plan_fork_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_fork: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_fork", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->n_children < 1 || a->n_parents < 1 || a->ld_parent < a->n_parents || a->ld_child < a->n_children ||
        (!a->parent && (a->K < 1 || (int64_t)a->n_parents * a->K < a->n_children)) ||
        !a->x_parent || !a->u_parent || !a->timestep_parent || !a->w_off_parent || !a->x || !a->u || !a->timestep || !a->w_off ||
        !a->ret || !a->viol || !a->n_steps || !a->alive || !a->failed)
        return refuse("glgym_plan_fork: bad arguments (null pointer, ld < batch, or without a parent table K < 1 or fewer than C = P * K slots)");
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    with_dtype(h->dtype, [&](auto t) { hipLaunchKernelGGL(plan_fork_kernel<decltype(t)>, dim3((a->n_children + 255) / 256), dim3(256), 0, st, *a); });
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_plan_accumulate(glgym_handle h, const glgym_plan_accumulate_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_accumulate: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_accumulate", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->B < 1 || a->ld < a->B || !a->reward || !a->info || !a->done || !a->ret || !a->viol || !a->n_steps || !a->alive || !a->failed)
        return refuse("glgym_plan_accumulate: bad arguments (null pointer or ld < B)");
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    with_dtype(h->dtype, [&](auto t) { hipLaunchKernelGGL(plan_accumulate_kernel<decltype(t)>, dim3((a->B + 255) / 256), dim3(256), 0, st, *a); });
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_plan_rollout(glgym_handle h, const glgym_plan_rollout_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_rollout: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_rollout", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (!horizon_ok("glgym_plan_rollout", a->H, a->gamma)) return GLGYM_EINVAL;
    if ((!a->actions) == (!a->controls) || a->step.B < 1 || a->step.ld < a->step.B)
        return refuse("glgym_plan_rollout: bad arguments (exactly one of actions / controls, step.B >= 1, step.ld >= step.B)");
    if (!outputs_ok("glgym_plan_rollout", *a)) return GLGYM_EINVAL;
    glgym_step_args s = a->step;                 // glgym_step checks its struct_size and the remaining members
    s.metrics = nullptr;
    const size_t plane = (size_t)NU * (size_t)s.ld * (h->dtype == GLGYM_F32 ? sizeof(float) : sizeof(double));
    return rollout_steps(h, s, *a, stream, [&](int k) {
        s.action = a->actions ? a->actions + (size_t)k * (size_t)s.B * NU : nullptr;
        s.control = a->controls ? (const void*)((const char*)a->controls + (size_t)k * plane) : nullptr;
        return (int)GLGYM_OK;
    });
}

// robust planning (gl_scen.hpp).  The arguments are checked before the handle is looked at, so that a caller without a device gets the
// refusal that names its mistake.
int glgym_plan_scenario(glgym_handle h, const glgym_plan_scenario_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_scenario: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_scenario", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (!scenario_shape_ok(a->P, a->K, a->S, a->hold, a->scale) || (int64_t)a->ld < (int64_t)a->P * a->K * a->S || a->h_step < 0 ||
        a->h_step > 65535 || !a->crop || (!a->actions_in) != (!a->actions_out))
        return refuse("glgym_plan_scenario: bad arguments (P, K, S < 1, S > 256, P*K*S > INT32_MAX, ld < P*K*S, h_step outside 0 .. 65 535, hold "
                      "not 0 | 1, scale negative or not finite, null crop, or one of actions_in / actions_out without the other)");
    if (!h) { g_err = "glgym_plan_scenario: null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    const int n_children = a->P * a->K * a->S;             // <= INT32_MAX: checked above
    with_dtype(h->dtype, [&](auto t) {
        hipLaunchKernelGGL(plan_scenario_kernel<decltype(t)>, dim3((unsigned)(((int64_t)n_children + 255) / 256)), dim3(256), 0, st, *a, h->p0_crop_dev, n_children);
    });
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_plan_rollout_scenarios(glgym_handle h, const glgym_plan_rollout_scenarios_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_rollout_scenarios: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_rollout_scenarios", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    const glgym_plan_rollout_args& r = a->rollout;
    if (!plan_size_ok("glgym_plan_rollout_scenarios: rollout", r.struct_size, sizeof r)) return GLGYM_EINVAL;
    if (r.controls)
        return refuse("glgym_plan_rollout_scenarios: raw-control scenario rollouts are not supported (rollout.controls must be NULL)");
    glgym_step_args s = r.step;
    if (!scenario_shape_ok(a->P, a->K, a->S, a->hold, a->scale) || !a->staging)
        return refuse("glgym_plan_rollout_scenarios: bad arguments (P, K, S < 1, S > 256, P*K*S > INT32_MAX, hold not 0 | 1, scale negative or "
                      "not finite, or null staging)");
    if (!horizon_ok("glgym_plan_rollout_scenarios", r.H, r.gamma)) return GLGYM_EINVAL;
    if (r.H > 65536 || !r.actions || (int64_t)s.B != (int64_t)a->P * a->K * a->S || s.ld < s.B || !s.crop_p)
        return refuse("glgym_plan_rollout_scenarios: bad arguments (H > 65 536, null actions / crop_p, step.B != P*K*S, or ld < B)");
    if (!outputs_ok("glgym_plan_rollout_scenarios", r)) return GLGYM_EINVAL;
    if (!h) { g_err = "glgym_plan_rollout_scenarios: null handle"; return GLGYM_EINVAL; }
    s.metrics = nullptr;
    s.action = a->staging;
    s.control = nullptr;
    // what glgym_step refuses is refused in its own words before the first prologue is launched
    if (const int rc = step_refusal(h, &s)) return rc;
    glgym_plan_scenario_args sc = scenario_args_of(*a, s);
    sc.actions_out = a->staging;
    const size_t plane = (size_t)a->P * (size_t)a->K * NU;             // the candidates' action plane of one step
    return rollout_steps(h, s, r, stream, [&](int k) {
        sc.actions_in = r.actions + (size_t)k * plane;
        return scenario_prologue(h, sc, k, stream);
    });
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
        !a->w_off_parent || !a->timestep_parent || !a->window)
        return refuse("glgym_plan_weather: bad arguments (P, K, S, H < 1, S > 256, H > 65 536, P*S*H or P*K*S > INT32_MAX, weather_rows < 1, a sigma "
                      "negative or not finite, phi outside [0, 1), or a null weather / w_off_parent / timestep_parent / window)");
    if (!h) { g_err = "glgym_plan_weather: null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    const double innov = glwscen::innov_of(a->phi);       // the one square root, on the host
    const int64_t n_lanes = (int64_t)a->P * a->S * glwscen::LANES;
    with_dtype(h->dtype, [&](auto t) {
        hipLaunchKernelGGL(plan_weather_kernel<decltype(t)>, dim3((unsigned)((n_lanes + 255) / 256)), dim3(256), 0, st, *a, h->nd, innov, n_lanes);
    });
    HIPCHK(hipGetLastError());
    if (!a->w_off_child) return GLGYM_OK;
    const int n_children = a->P * a->K * a->S;
    hipLaunchKernelGGL(plan_weather_offsets_kernel, dim3((unsigned)(((int64_t)n_children + 255) / 256)), dim3(256), 0, st, *a, n_children);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

// closed-loop rule-based rollouts (gl_rule.hpp): checked before the handle is looked at, like the entry points above
static bool rule_space_ok(const char* who, const glgym_rule_space* sp)
{
    const char* why = glrule::space_error(sp);
    if (why) g_err = std::string(who) + ": bad search space (" + why + ")";
    return !why;
}

// the launch behind both entry points: arguments already checked
static int launch_rule_rows(glgym_handle h, const glrule::Space& sp, const float* theta, int J, int S, const glgym_rule_args& r, hipStream_t st)
{
    DeviceGuard dev_guard(h);
    const double doy_inc = std::fmod(h->dt / 86400.0, 365.0), hod_inc = h->dt / 3600.0;       // glgym_rule_based's
    with_dtype(h->dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((rule_rows_kernel<T>), dim3((r.B + 255) / 256), dim3(256), 0, st, sp, theta, J, S, r.B, r.ld, (const T*)r.x,
                           (const T*)r.weather, r.weather_rows, r.w_off, r.timestep, r.start_day, r.hour, r.doy, doy_inc, hod_inc,
                           (T*)r.control, h->nd);
    });
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_rule_rows(glgym_handle h, const glgym_rule_rows_args* a, void* stream)
{
    if (!a) { g_err = "glgym_rule_rows: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_rule_rows", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (!rule_space_ok("glgym_rule_rows", &a->space)) return GLGYM_EINVAL;
    const glgym_rule_args& r = a->rule;
    if (!a->theta || !r.control) { g_err = "glgym_rule_rows: null theta or control"; return GLGYM_EINVAL; }
    if (r.B < 1 || r.ld < r.B) { g_err = "glgym_rule_rows: B < 1 or ld < B"; return GLGYM_EINVAL; }
    if (!scenario_count_ok("glgym_rule_rows", a->S)) return GLGYM_EINVAL;
    if (a->J < 1 || (int64_t)r.B > (int64_t)a->J * (a->S > 1 ? a->S : 1))
        return refuse("glgym_rule_rows: J < 1, or more rows than parameters (B > J * max(S, 1))");
    if (!r.x || !r.weather || !r.w_off || !r.timestep || r.weather_rows < 1 || (!r.start_day && !r.doy))
        return refuse("glgym_rule_rows: bad arguments (null x / weather / w_off / timestep, weather_rows < 1, or neither start_day nor doy)");
    if (!h) { g_err = "glgym_rule_rows: null handle"; return GLGYM_EINVAL; }
    return launch_rule_rows(h, glrule::make_space(a->space), a->theta, a->J, a->S, r, (hipStream_t)stream);
}

int glgym_plan_rollout_rule(glgym_handle h, const glgym_plan_rollout_rule_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_rollout_rule: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_rollout_rule", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    const glgym_plan_rollout_args& r = a->rollout;
    if (!plan_size_ok("glgym_plan_rollout_rule: rollout", r.struct_size, sizeof r)) return GLGYM_EINVAL;
    if (!rule_space_ok("glgym_plan_rollout_rule", &a->space)) return GLGYM_EINVAL;
    if (r.actions) return refuse("glgym_plan_rollout_rule: the controller makes the controls (rollout.actions must be NULL)");
    if (!a->theta || !r.controls) { g_err = "glgym_plan_rollout_rule: null theta or controls"; return GLGYM_EINVAL; }
    if (a->record != 0 && a->record != 1) { g_err = "glgym_plan_rollout_rule: record must be 0 or 1"; return GLGYM_EINVAL; }
    if (!horizon_ok("glgym_plan_rollout_rule", r.H, r.gamma)) return GLGYM_EINVAL;
    if (!scenario_count_ok("glgym_plan_rollout_rule", a->S)) return GLGYM_EINVAL;
    glgym_step_args s = r.step;
    if (s.B < 1 || s.ld < s.B) { g_err = "glgym_plan_rollout_rule: step.B < 1 or step.ld < step.B"; return GLGYM_EINVAL; }
    if (a->S == 0) {
        if (a->J < 1 || s.B > a->J) { g_err = "glgym_plan_rollout_rule: without scenarios step.B <= J is needed (and J >= 1)"; return GLGYM_EINVAL; }
    } else if (!with_scenarios_ok("glgym_plan_rollout_rule", *a, r.H, s, (int64_t)a->P * a->K, "J == P*K")) {
        return GLGYM_EINVAL;
    }
    if (!a->start_day) { g_err = "glgym_plan_rollout_rule: null start_day"; return GLGYM_EINVAL; }
    if (!outputs_ok("glgym_plan_rollout_rule", r)) return GLGYM_EINVAL;
    if (!h) { g_err = "glgym_plan_rollout_rule: null handle"; return GLGYM_EINVAL; }
    const size_t plane = (size_t)NU * (size_t)s.ld * (h->dtype == GLGYM_F32 ? sizeof(float) : sizeof(double));
    s.metrics = nullptr;
    s.action = nullptr;
    s.control = r.controls;
    // what glgym_step refuses is refused in its own words before the first prologue is launched
    if (const int rc = step_refusal(h, &s)) return rc;
    const glrule::Space sp = glrule::make_space(a->space);
    glgym_rule_args rule;
    rule.B = s.B; rule.ld = s.ld; rule.x = s.x; rule.weather = s.weather; rule.weather_rows = s.weather_rows; rule.w_off = s.w_off;
    rule.timestep = s.timestep; rule.start_day = a->start_day; rule.hour = nullptr; rule.doy = nullptr;
    glgym_plan_scenario_args sc = scenario_args_of(*a, s);
    return rollout_steps(h, s, r, stream, [&](int k) {
        if (const int rc = scenario_prologue(h, sc, k, stream)) return rc;
        rule.control = (char*)const_cast<void*>(r.controls) + (a->record ? (size_t)k * plane : 0);
        s.control = rule.control;
        return launch_rule_rows(h, sp, a->theta, a->J, a->S, rule, (hipStream_t)stream);
    });
}

// closed-loop neural-policy rollouts (gl_mlp.hpp): checked before the handle is looked at, like the entry points above
static bool policy_net_ok(const char* who, const glgym_mlp_net* net)
{
    const char* why = glmlp::net_error(net);
    if (why) g_err = std::string(who) + ": bad net (" + why + ")";
    return !why;
}

// S, the row mode and J against the B rows that read theta
static bool policy_rows_ok(const char* who, int32_t B, int32_t J, int32_t S, int32_t mode)
{
    if (!scenario_count_ok(who, S)) return false;
    if (B > INT32_MAX - (WAVE - 1)) {                            // the last block's lane indices must not wrap
        g_err = std::string(who) + ": more than 2^31 - 64 rows";
        return false;
    }
    if (mode != GLGYM_POLICY_ROW_CHILD && mode != GLGYM_POLICY_ROW_CANDIDATE) {
        g_err = std::string(who) + ": row_mode is not GLGYM_POLICY_ROW_CHILD or _CANDIDATE";
        return false;
    }
    if (J < 1 || (mode == GLGYM_POLICY_ROW_CHILD && (int64_t)B > (int64_t)J * (S > 1 ? S : 1))) {
        g_err = std::string(who) + ": J < 1, or in CHILD mode more rows than parameters (B > J * max(S, 1))";
        return false;
    }
    return true;
}

// the launch behind both entry points: arguments already checked
static int launch_policy_rows(glgym_handle h, const glgym_mlp_net& net, const float* obs, const float* theta, int J, int S, int mode, int B,
                              float* action, hipStream_t st)
{
    DeviceGuard dev_guard(h);
    const int rows = glmlp::buffer_rows(net);
    const size_t lds = (size_t)2 * rows * WAVE * sizeof(float);
    hipLaunchKernelGGL(policy_rows_kernel, dim3((B + WAVE - 1) / WAVE), dim3(WAVE), lds, st, net, rows, obs, theta, J, S, mode, B, action);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_policy_rows(glgym_handle h, const glgym_policy_rows_args* a, void* stream)
{
    if (!a) { g_err = "glgym_policy_rows: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_policy_rows", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (!policy_net_ok("glgym_policy_rows", &a->net)) return GLGYM_EINVAL;
    if (!a->obs || !a->theta || !a->action) { g_err = "glgym_policy_rows: null obs, theta or action"; return GLGYM_EINVAL; }
    if (a->B < 1) { g_err = "glgym_policy_rows: B < 1"; return GLGYM_EINVAL; }
    if (!policy_rows_ok("glgym_policy_rows", a->B, a->J, a->S, a->row_mode)) return GLGYM_EINVAL;
    if (!h) { g_err = "glgym_policy_rows: null handle"; return GLGYM_EINVAL; }
    return launch_policy_rows(h, a->net, a->obs, a->theta, a->J, a->S, a->row_mode, a->B, a->action, (hipStream_t)stream);
}

int glgym_plan_rollout_policy(glgym_handle h, const glgym_plan_rollout_policy_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_rollout_policy: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_rollout_policy", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    const glgym_plan_rollout_args& r = a->rollout;
    if (!plan_size_ok("glgym_plan_rollout_policy: rollout", r.struct_size, sizeof r)) return GLGYM_EINVAL;
    if (!policy_net_ok("glgym_plan_rollout_policy", &a->net)) return GLGYM_EINVAL;
    if (r.actions || r.controls)
        return refuse("glgym_plan_rollout_policy: the policy makes the actions (rollout.actions and rollout.controls must be NULL)");
    if (!a->theta || !a->obs || !a->actions) { g_err = "glgym_plan_rollout_policy: null theta, obs or actions"; return GLGYM_EINVAL; }
    if (a->record != 0 && a->record != 1) { g_err = "glgym_plan_rollout_policy: record must be 0 or 1"; return GLGYM_EINVAL; }
    if (!horizon_ok("glgym_plan_rollout_policy", r.H, r.gamma)) return GLGYM_EINVAL;
    if (a->Np < 0 || a->Np > OBS_MAX_NP) { g_err = "glgym_plan_rollout_policy: Np outside 0 .. 128"; return GLGYM_EINVAL; }
    glgym_step_args s = r.step;
    if (s.B < 1 || s.ld < s.B) { g_err = "glgym_plan_rollout_policy: step.B < 1 or step.ld < step.B"; return GLGYM_EINVAL; }
    if (!policy_rows_ok("glgym_plan_rollout_policy", s.B, a->J, a->S, a->row_mode)) return GLGYM_EINVAL;
    if (a->S >= 1 && !with_scenarios_ok("glgym_plan_rollout_policy", *a, r.H, s,
                                        a->row_mode == GLGYM_POLICY_ROW_CHILD ? (int64_t)a->P * a->K : (int64_t)a->K,
                                        "J == P*K (CHILD mode) or K (CANDIDATE mode)"))
        return GLGYM_EINVAL;
    if (!a->start_day) { g_err = "glgym_plan_rollout_policy: null start_day"; return GLGYM_EINVAL; }
    if (!outputs_ok("glgym_plan_rollout_policy", r)) return GLGYM_EINVAL;
    if (!h) { g_err = "glgym_plan_rollout_policy: null handle"; return GLGYM_EINVAL; }
    const int dim = glgym_obs_dim(h, a->Np);
    if (dim != a->net.in_dim)
        return refuse("glgym_plan_rollout_policy: net.in_dim is " + std::to_string(a->net.in_dim) + ", the handle's observation row at Np = " +
                      std::to_string(a->Np) + " has " + std::to_string(dim) + " columns (glgym_obs_dim)");
    const size_t plane = (size_t)NU * (size_t)s.B;               // floats per action plane
    s.metrics = nullptr;
    s.control = nullptr;
    s.action = a->actions;
    // what glgym_step refuses is refused in its own words before the first prologue is launched
    if (const int rc = step_refusal(h, &s)) return rc;
    glgym_obs_args ob;
    ob.B = s.B; ob.ld = s.ld; ob.x = s.x; ob.u = s.u; ob.weather = s.weather; ob.weather_rows = s.weather_rows; ob.w_off = s.w_off;
    ob.timestep = s.timestep; ob.start_day = a->start_day; ob.Np = a->Np; ob.obs = a->obs; ob.mask = nullptr; ob.term_obs = nullptr;
    glgym_plan_scenario_args sc = scenario_args_of(*a, s);
    return rollout_steps(h, s, r, stream, [&](int k) {
        int rc = scenario_prologue(h, sc, k, stream);
        if (rc != GLGYM_OK || (rc = glgym_obs(h, &ob, stream)) != GLGYM_OK) return rc;
        float* act = a->actions + (a->record ? (size_t)k * plane : 0);
        s.action = act;
        return launch_policy_rows(h, a->net, a->obs, a->theta, a->J, a->S, a->row_mode, s.B, act, (hipStream_t)stream);
    });
}

}  // extern "C"
