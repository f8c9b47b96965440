// gl_bdf_env.hpp -- one row of the BDF integrator (gl_bdf.hpp) with its inputs, and one env-step of TomatoEnv.step /
// step_raw_control around it (GLGYM_INTEGRATOR_BDF for glgym_step), written once for a team of lanes like gl_bdf.hpp.
//   bdf_row      crop constants and tier-2 coefficients of the row, then bdf_step: what glgym_evalF's BDF kernel and the BDF
//                env-step both run, so that the two give the same bits on the same double inputs.
//   bdf_env_row  controls -> weather row and crop block -> bdf_row -> state, reward, info and terminal test in T: the meaning of
//                glgym.hip's step_kernel (tomato_env.py:115-173, rewards.py:156-231), with the integrator's failure reported as the
//                reference reports a CVODES exception (tomato_env.py:119-123): state unchanged, done = 1.
// The device instantiation is glgym_bdf.hip's bdf_env_kernel (one wavefront per environment); tests/bdfhost/envstep_host.cpp
// instantiates both functions with a team of one on the host.
#pragma once
#include <cstdint>

#include "gl_bdf.hpp"
#include "gl_reward.hpp"

namespace glbdf {

using glm::NCROP;
using glm::NU;

// The row's inputs: x0 in s.D[0]; u[6], d[7] and crop[34] (the row's p[128..161], or nullptr: the handle's crop constants) are read
// by lane 0.  Inputs the team itself staged must be ordered by a tm.sync() before the call.  cr / s are the team's storage of the row's constants
// (the team refers to them).  bad != 0 in any lane: a non-finite input, no integration (BDF_FAIL_NONFINITE, stats untouched).
template <class Team>
GL_HD int bdf_row(const Team& tm, BdfScratch& sh, const glm::ModelConst<double>& m, glm::CropConst<double>& cr, glm::StepCoef<double>& s,
                  const double* crop, double gasR, double tCanMin, const double* u, const double* d, double bad, double dt, double rtol,
                  double atol, int max_steps, int32_t* stats)
{
    if (tm.lane() == 0) {
        glm::CropConst<double> c;
        if (crop) glm::make_crop_const<double, double>(crop, gasR, tCanMin, c);
        else c = m.crop;
        cr = c;
    }
    tm.sync();
    if (tm.lane() == 0) {
        double uu[NU], dd[7];
        for (int i = 0; i < NU; ++i) uu[i] = u[i];
        for (int i = 0; i < 7; ++i) dd[i] = d[i];
        glm::StepCoef<double> c;
        glm::precompute(uu, dd, m, cr, c);
        s = c;
    }
    tm.sync();
    if (tm.sum(bad) != 0.0) return BDF_FAIL_NONFINITE;
    return bdf_step(tm, sh, dt, rtol, atol, max_steps, stats);
}

// Arguments of one batched BDF env-step: glgym_step_args' arrays (SoA [n][ld] in T, environment b at column b) and the handle's settings.
template <class T> struct BdfEnvArgs {
    int ld;
    T* x; T* u;
    const float* action; const T* control;       // exactly one is non-null
    const T* weather; int weather_rows; int nd;
    const int* w_off; int* timestep;
    const T* crop_p;                             // SoA [34][ld] or nullptr
    int N;
    T* reward; T* info; unsigned char* done; int* step_flags;
    double dt, rtol, atol; int max_steps;
    double gasR, tCanMin;                        // p[39], p[162] of the handle
    float du, u_min[NU], u_max[NU];              // action_to_control (glgym_set_control_limits)
};

// What the metric accumulators of a step take from one environment (valid in lane 0).
template <class T> struct BdfEnvResult {
    T reward, profit, viol[3];
    bool done, failed;
    int32_t stats[NSTAT];
};

// The team's shared storage of one env-step (LDS on the device).
struct BdfEnvScratch {
    BdfScratch bdf;
    double u[NU], d[7], crop[NCROP];             // the integration's inputs in double
    double x0[NX], x1[NX];                       // the state before (double of T) and after (double of the stored T value)
};

template <class T, class Team>
GL_HD BdfEnvResult<T> bdf_env_row(const Team& tm, BdfEnvScratch& sh, const glm::ModelConst<double>& m, glm::CropConst<double>& cr,
                                  glm::StepCoef<double>& s, const glm::RewardConstBase<T>& rw, const BdfEnvArgs<T>& a, int b)
{
    using M = glm::Math<T>;
    const size_t ld = (size_t)a.ld;
    const int ts = a.timestep[b];
    int row = a.w_off[b] + ts;
    row = row < 0 ? 0 : (row >= a.weather_rows ? a.weather_rows - 1 : row);
    // ---- controls (tomato_env.py:109-113, the f32 product and the clip in T as step_kernel; raw controls unclipped, :148-149), stored
    // before the integration: self.u is set before evalF and survives a failure (:117-123)
    double bad = 0.0;
    for (int j = tm.lane(); j < NU; j += Team::width) {
        T uj;
        if (a.action) {
            const float inc = a.action[(size_t)b * NU + j] * a.du;
            const T v = a.u[(size_t)j * ld + b] + T(inc);
            uj = M::min(M::max(v, T(a.u_min[j])), T(a.u_max[j]));
        } else {
            uj = a.control[(size_t)j * ld + b];
        }
        a.u[(size_t)j * ld + b] = uj;
        sh.u[j] = (double)uj;
        if (!__builtin_isfinite(sh.u[j])) bad = 1.0;
    }
    // ---- inputs in double: the weather row (zero-order hold, tomato_env.py:120), the env's crop block, the state
    for (int j = tm.lane(); j < 7; j += Team::width) {
        sh.d[j] = (double)a.weather[(size_t)row * a.nd + j];
        if (!__builtin_isfinite(sh.d[j])) bad = 1.0;
    }
    if (a.crop_p)
        for (int i = tm.lane(); i < NCROP; i += Team::width) sh.crop[i] = (double)a.crop_p[(size_t)i * ld + b];
    for (int i = tm.lane(); i < NX; i += Team::width) {
        const double v = (double)a.x[(size_t)i * ld + b];
        sh.x0[i] = v;
        sh.bdf.D[0][i] = v;
        if (!__builtin_isfinite(v)) bad = 1.0;
    }
    tm.sync();                                   // bdf_row's lane 0 reads the staged inputs of every lane
    BdfEnvResult<T> r;
    for (int k = 0; k < NSTAT; ++k) r.stats[k] = 0;
    const int rc = bdf_row(tm, sh.bdf, m, cr, s, a.crop_p ? sh.crop : nullptr, a.gasR, a.tCanMin, sh.u, sh.d, bad, a.dt, a.rtol, a.atol,
                           a.max_steps, r.stats);
    const bool failed = rc != BDF_OK;
    // ---- the new state in T (failure: unchanged); x27 = time [days since reset] exact from the step counter as step_kernel
    for (int i = tm.lane(); i < NX; i += Team::width) {
        T xi = failed ? T(sh.x0[i]) : T(sh.bdf.D[0][i]);
        if (i == NX - 1 && !failed) {
            const double per_step = (double)T(a.dt) / 86400.0;
            double t_start = sh.x0[NX - 1] - (double)ts * per_step;
            if (::fabs(t_start) < 5e-4) t_start = 0.0;
            xi = T(t_start + ((double)ts + 1.0) * per_step);
        }
        a.x[(size_t)i * ld + b] = xi;
        sh.x1[i] = (double)xi;
    }
    tm.sync();
    // ---- reward epilogue in T from the stored state (rewards.py:156-231; indoor obs conversions observations.py:70-77)
    r.failed = failed;
    r.done = failed || ts >= a.N;
    r.reward = r.profit = r.viol[0] = r.viol[1] = r.viol[2] = T(0);
    if (tm.lane() == 0) {
        const T co2Air = T(sh.x1[0]), tAir = T(sh.x1[2]), vpAir = T(sh.x1[15]);
        const T co2ppm = rw.kPpm * (tAir + T(273.15)) * co2Air;
        const T rh = M::min(M::max(T(100) * vpAir / glm::sat_vp_exact(tAir), T(0)), T(100));
        const T o3[3] = {co2ppm, tAir, rh};
        T pen = T(0);
        for (int i = 0; i < 3; ++i) {
            r.viol[i] = M::max(rw.lo[i] - o3[i], T(0)) + M::max(o3[i] - rw.hi[i], T(0));
            pen += r.viol[i] * rw.invMaxViol[i];
        }
        const T uBoil = T(sh.u[0]), uCo2 = T(sh.u[1]), uLamp = T(sh.u[4]);
        const T heat = uBoil * rw.heatK, elec = uLamp * rw.elecK, co2c = uCo2 * rw.co2K;
        const T varc = heat + co2c + elec;
        const T gains = (failed ? T(0) : T(sh.bdf.D[0][25] - sh.x0[25])) * rw.gainK;
        r.profit = gains - varc;
        r.reward = (r.profit - rw.minProfit) * rw.invRange - pen;          // lamp penalty is identically 0 (:203-212)
        a.timestep[b] = ts + 1;
        a.reward[b] = r.reward;
        a.done[b] = r.done ? 1 : 0;
        if (a.step_flags) {
            const int32_t steps = r.stats[ST_STEPS] < 32767 ? r.stats[ST_STEPS] : 32767;
            a.step_flags[b] = GLGYM_SF_BDF | (failed ? GLGYM_SF_FAILED : 0) | (steps << 16);
        }
        if (a.info) {
            const T inf[GLGYM_NINFO] = {r.profit, gains, varc, rw.fixedCosts, co2c, heat, elec, r.viol[1], r.viol[0], r.viol[2], T(0)};
            for (int i = 0; i < GLGYM_NINFO; ++i) a.info[(size_t)i * ld + b] = inf[i];
        }
    }
    return r;
}

}  // namespace glbdf
