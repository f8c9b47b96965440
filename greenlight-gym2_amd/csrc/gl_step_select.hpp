// gl_step_select.hpp -- which build of the env-step kernel a glgym_step* call runs, as a pure function of what the call and the handle
// say, and the one list of the builds that exist.  glgym.hip's launcher and tests/test_step_select_host.py both take the builds from
// here.  Below it the same for glgym_evalF's integrator kernels: select_evalf and the list of the 29 evalF builds.
// Plain C++17, no HIP types: compiles with a plain host compiler like gl_reward.hpp.
#pragma once

namespace glsel {

constexpr int WAVE = 64;
constexpr int SCH_OBS = 8, SCH_RESET = 16;                       // epilogue bits on step_kernel's scheme argument (GL_SCH_* in glgym.hip)
constexpr int OBS_MAX_DIM_OCC1 = 512, OBS_MAX_DIM_OCC2 = 292;    // widest observation row an epilogue stages (STEP_OBS_MAX_DIM_* in glgym.hip)
constexpr int RK4 = 0;                                           // GLGYM_SCHEME_RK4; 1 RK2, 2 RK3, 3 LS5

// ---- the builds that exist ------------------------------------------------------------------------------------------------------
// One lane per environment, fp32 only: step_kernel<float, CROP, DEF, PIPE, SCH | EPI, OCC> for every scheme SCH; the ODE_pipe build
// for GLGYM_SCHEME_RK4 only (one_lane_build_exists).  CROP: per-env crop block; DEF: the default parameter block compiled in;
// EPI: 0, SCH_OBS (observation epilogue) or SCH_OBS | SCH_RESET (auto-reset epilogue behind it); OCC: waves per SIMD compiled for.
#define GL_STEP_ONE_LANE_BUILDS(X)                                                                                       \
    /* CROP   DEF    PIPE   EPI  OCC */                                                                                  \
    X(false, false, false, 0, 1) X(false, true, false, 0, 1) X(true, false, false, 0, 1) X(true, true, false, 0, 1)      \
    X(false, true, false, 0, 2)                                                                                          \
    X(false, false, false, 8, 1) X(false, true, false, 8, 1) X(true, false, false, 8, 1) X(true, true, false, 8, 1)      \
    X(false, true, false, 8, 2)                                                                                          \
    X(false, false, false, 24, 1) X(false, true, false, 24, 1) X(false, true, false, 24, 2)                              \
    X(false, false, true, 0, 1)
constexpr bool one_lane_build_exists(bool pipe, int sch) { return !pipe || sch == RK4; }
// Four lanes per environment: step_kernel_quad<T, DEF, SCH, PIPE, CROP, PAIR> for every scheme SCH.  fp64: ODE_pipe compiled in
// (selected at run time), never the default block, per-env crop blocks.  fp32: shared crop parameters, default ODE.  PAIR: two quads
// per environment, the verification ladder two rungs at a time.
#define GL_STEP_QUAD_BUILDS(X)                                                                                           \
    /* F64    DEF    PIPE   CROP   PAIR */                                                                               \
    X(true, false, true, false, false) X(true, false, true, true, false) X(true, false, true, false, true)              \
    X(false, false, false, false, false) X(false, true, false, false, false)                                             \
    X(false, false, false, false, true) X(false, true, false, false, true)

enum Family { ONE_LANE = 0, QUAD = 1, QUAD_PAIR = 2 };

struct StepBuild {
    int family;
    bool f64, crop, def, pipe;
    int sch, epi, occ;                       // epi / occ: one-lane builds only (0 / 1 on the quad builds)
};
constexpr bool operator==(const StepBuild& a, const StepBuild& b)
{
    return a.family == b.family && a.f64 == b.f64 && a.crop == b.crop && a.def == b.def && a.pipe == b.pipe && a.sch == b.sch &&
           a.epi == b.epi && a.occ == b.occ;
}

// ---- the selection --------------------------------------------------------------------------------------------------------------
struct StepSelectIn {
    bool f64;                    // handle dtype
    int scheme;                  // GLGYM_SCHEME_*
    bool pipe;                   // the handle's ODE variant is GLGYM_ODE_PIPE
    bool crop;                   // the call carries a per-env crop block
    bool def;                    // the handle's parameters are bit-identical to the default block (and specialised builds are allowed)
    int layout, occupancy;       // glgym_set_layout 0 auto / 1 one lane / 2 quad; glgym_set_occupancy 0 auto / 1 / 2
    int B, n_simd;
    bool verify;                 // this call integrates with the step-doubling ladder (glgym_set_verify, already resolved for the call)
    bool ladder_parallel;        // glgym_set_ladder_parallel
    bool obs_ok; int obs_dim;    // glgym_step_obs: the observation block names the step's buffers (full mode); its row width
    bool reset_ok;               // glgym_step_obs_reset: the reset block names the step's buffers and carries a start table
};
struct StepChoice {
    const char* error;           // non-null: GLGYM_EINVAL with this text, nothing to launch
    StepBuild build;
    unsigned grid;               // workgroups of WAVE lanes
    int fused;                   // 0: the step alone; 1: the launch also writes the observation rows; 2: ... and does the auto-reset
};

// Rules, in the order they apply:
//  * ODE_pipe takes neither a per-env crop block nor a scheme other than RK4: an error.
//  * pair: a verified call with ladder_parallel, no crop block and 8 * B <= WAVE * n_simd lanes (at most one wavefront per SIMD at eight
//    lanes per environment) takes the PAIR build wherever it takes a quad build at all.
//  * fp64 is always quad, never with the default block compiled in, ODE_pipe compiled in; it takes per-env crop blocks.  (It scales
//    with the batch in rounds of 16 384 environments, 2.86 ms per round at n_sub 240.)
//  * fp32 takes a quad build when the layout is forced to quad, or left to auto with B <= 16 * n_simd (one round of quad wavefronts),
//    but only for the default ODE without a crop block.
//  * fp32 ODE_pipe beyond that: the single generic RK4 build, no epilogue.
//  * The two-waves-per-SIMD build (OCC 2) exists for default parameters without a crop block; it is taken when the occupancy is
//    forced to 2, or left to auto with B >= 2 * WAVE * n_simd: 256 registers so that two waves share a SIMD, measured 1.08x at
//    131 072 environments and 1.11x from 524 288 on MI355X (profiles/r05_occupancy2.txt).
//  * The observation epilogue needs obs_ok and a row of 1 .. 512 columns (1 .. 292 on the OCC 2 build); the auto-reset epilogue needs
//    the observation epilogue, reset_ok and no crop block.  Only these two set `fused`.

// whether the call takes a four-lanes-per-environment build (then no epilogue exists, and obs_ok / obs_dim / reset_ok are not read)
inline bool takes_quad(const StepSelectIn& s)
{
    return s.f64 || (!s.pipe && !s.crop && (s.layout == 2 || (s.layout == 0 && s.B <= 16 * s.n_simd)));
}

// the first rule on its own -- the error's text, or null --, for glgym.hip's step_refusal, which decides before anything is launched
inline const char* step_pipe_error(bool pipe, bool crop, int scheme)
{
    return pipe && (crop || scheme != RK4)
               ? "glgym_step: GLGYM_ODE_PIPE supports neither per-env crop parameters nor schemes other than GLGYM_SCHEME_RK4"
               : nullptr;
}

inline StepChoice select_step(const StepSelectIn& s)
{
    if (const char* error = step_pipe_error(s.pipe, s.crop, s.scheme)) return {error, {}, 0, 0};
    const auto blocks = [&](int lanes_per_env) { return (unsigned)(((unsigned long long)lanes_per_env * s.B + WAVE - 1) / WAVE); };
    const bool pair = s.verify && s.ladder_parallel && !s.crop && 8ull * s.B <= (unsigned long long)WAVE * s.n_simd;
    if (takes_quad(s))
        return {nullptr, {pair ? QUAD_PAIR : QUAD, s.f64, s.f64 && s.crop, !s.f64 && s.def, s.f64, s.scheme, 0, 1}, blocks(pair ? 8 : 4), 0};
    if (s.pipe) return {nullptr, {ONE_LANE, false, false, false, true, RK4, 0, 1}, blocks(1), 0};
    const bool occ2 = s.def && !s.crop && (s.occupancy == 2 || (s.occupancy == 0 && s.B >= 2 * WAVE * s.n_simd));
    const bool obs = s.obs_ok && s.obs_dim > 0 && s.obs_dim <= (occ2 ? OBS_MAX_DIM_OCC2 : OBS_MAX_DIM_OCC1);
    const bool reset = obs && s.reset_ok && !s.crop;
    const int fused = reset ? 2 : obs ? 1 : 0;
    return {nullptr, {ONE_LANE, false, s.crop, s.def, false, s.scheme, reset ? SCH_OBS | SCH_RESET : obs ? SCH_OBS : 0, occ2 ? 2 : 1},
            blocks(1), fused};
}

// ---- glgym_evalF: the builds that exist -----------------------------------------------------------------------------------------
// Four lanes per row: evalf_kernel_quad<T, SCH, PIPE, CROP, PAIR> for every scheme SCH.  fp64: ODE_pipe compiled in (selected at run
// time), plain, per-row crop blocks, PAIR.  fp32: the default ODE, shared crop parameters, plain and PAIR.
#define GL_EVALF_QUAD_BUILDS(X)                                                                                          \
    /* F64    PIPE   CROP   PAIR */                                                                                      \
    X(true, true, false, false) X(true, true, true, false) X(true, true, false, true)                                    \
    X(false, false, false, false) X(false, false, false, true)
// One lane per row, fp32 only: evalf_kernel<float, CROP, PIPE, SCH> for every scheme SCH; the ODE_pipe build for GLGYM_SCHEME_RK4 only
// (one_lane_build_exists).
#define GL_EVALF_ONE_LANE_BUILDS(X)                                                                                      \
    /* CROP   PIPE */                                                                                                    \
    X(false, false) X(true, false) X(false, true)

struct EvalfBuild {
    int family;
    bool f64, crop, pipe;                    // crop: per-row crop blocks compiled in; pipe: ODE_pipe compiled in
    int sch;
};
constexpr bool operator==(const EvalfBuild& a, const EvalfBuild& b)
{
    return a.family == b.family && a.f64 == b.f64 && a.crop == b.crop && a.pipe == b.pipe && a.sch == b.sch;
}

struct EvalfSelectIn {
    bool f64;                    // handle dtype
    int scheme;                  // GLGYM_SCHEME_*
    bool pipe;                   // the handle's ODE variant is GLGYM_ODE_PIPE
    bool crop;                   // the call carries per-row parameter blocks (which differ inside the crop block only)
    int layout;                  // glgym_set_layout 0 auto / 1 one lane / 2 quad
    int B, n_simd;
    bool verify;                 // glgym_set_verify is not GLGYM_VERIFY_NEVER
    bool ladder_parallel;        // glgym_set_ladder_parallel
};
struct EvalfChoice {
    const char* error;           // non-null: GLGYM_EINVAL with this text, nothing to launch
    EvalfBuild build;
    unsigned grid;               // workgroups of WAVE lanes
};

// Rules, in the order they apply:
//  * ODE_pipe takes neither per-row parameter blocks nor a scheme other than RK4: an error.
//  * pair: a verified call with ladder_parallel, no per-row blocks and 8 * B <= WAVE * n_simd lanes (at most one wavefront per SIMD at
//    eight lanes per row), on an fp64 handle or an fp32 handle whose layout is not forced to one lane.
//  * fp64 is always quad, ODE_pipe compiled in: the PAIR build under `pair`, else the per-row-crop build where the call carries
//    blocks, else the plain one.
//  * fp32 ODE_pipe: the single one-lane RK4 build, before anything else (no fp32 quad build has the pipe equation).
//  * fp32 under `pair`: the PAIR build.
//  * fp32 without per-row blocks takes the quad build when the layout is forced to quad, or left to auto with B <= 16 * n_simd (one
//    round of quad wavefronts, as glgym_step).
//  * fp32 beyond that: one lane per row, the crop build where the call carries blocks, else the plain one.
inline EvalfChoice select_evalf(const EvalfSelectIn& s)
{
    if (s.pipe && (s.crop || s.scheme != RK4))
        return {"glgym_evalF: GLGYM_ODE_PIPE supports neither per-row parameter blocks nor schemes other than GLGYM_SCHEME_RK4", {}, 0};
    const auto blocks = [&](int lanes_per_row) { return (unsigned)(((unsigned long long)lanes_per_row * s.B + WAVE - 1) / WAVE); };
    const bool pair = s.verify && s.ladder_parallel && !s.crop && 8ull * s.B <= (unsigned long long)WAVE * s.n_simd &&
                      (s.f64 || s.layout != 1);
    if (s.f64) return {nullptr, {pair ? QUAD_PAIR : QUAD, true, s.crop, true, s.scheme}, blocks(pair ? 8 : 4)};
    if (s.pipe) return {nullptr, {ONE_LANE, false, false, true, RK4}, blocks(1)};
    if (pair) return {nullptr, {QUAD_PAIR, false, false, false, s.scheme}, blocks(8)};
    if (!s.crop && (s.layout == 2 || (s.layout == 0 && s.B <= 16 * s.n_simd))) return {nullptr, {QUAD, false, false, false, s.scheme}, blocks(4)};
    return {nullptr, {ONE_LANE, false, s.crop, false, s.scheme}, blocks(1)};
}

}  // namespace glsel
