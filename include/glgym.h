/*
 * glgym.h -- C ABI of libglgym.so: the MI355X (gfx950) implementation of GreenLight-Gym's
 * per-timestep ODE integration, i.e. the path TomatoEnv.step() drives.
 *
 * Plain C, pointers and sizes only (no torch / pybind types).  One handle = one HIP device + one
 * parameter block + one dtype.  The library never allocates per call on the hot path and never
 * synchronises the stream in glgym_step / glgym_obs / glgym_step_obs / glgym_step_obs_reset / glgym_reset (safe to capture in a hipGraph);
 * the host-pointer convenience entry points (glgym_evalF, glgym_rhs) do synchronise.
 * Every function returns a glgym_status; nothing throws.  There is NO CPU fallback: without a HIP
 * device glgym_create() returns GLGYM_ENODEV.
 *
 * Reference interface each entry point replaces (paths relative to the GreenLight-Gym2 repo):
 *   glgym_create   <- GreenLight::GreenLight(nx,nu,nd,np,dt)   gl_gym/environments/models/greenlight_model.cpp:31-94
 *                     + env.p = init_default_params(np)         gl_gym/environments/tomato_env.py:62
 *   glgym_evalF    <- GreenLight::evalF(x,u,d,p) -> x_next      gl_gym/environments/models/greenlight_model.cpp:96-120
 *                     (pybind binding                            gl_gym/environments/models/greenlight_model.cpp:130-136)
 *   glgym_step     <- TomatoEnv.step / step_raw_control         gl_gym/environments/tomato_env.py:115-173
 *                     (action_to_control :109-113, evalF call :120, terminal test :131-132,
 *                      reward rewards.py:218-231, info tomato_env.py:208-222), batched over B envs
 *   glgym_obs      <- TomatoEnv._get_obs + 6 observation modules gl_gym/environments/observations.py:59-182
 *   glgym_step_obs <- the two above in one call (one launch where the step kernel can write the observation rows itself)
 *   glgym_step_obs_reset <- the same, then the auto-reset of a vectorised environment: terminal observation kept, finished
 *                     environments re-initialised, their rows recomputed (one launch where the step kernel can do all of it)
 *   glgym_reset    <- TomatoEnv.reset (state part)               gl_gym/environments/tomato_env.py:262-266,
 *                     init_state                                  gl_gym/environments/utils.py:13-46
 *   glgym_crop_noise <- parametric_crop_uncertainty               gl_gym/environments/noise.py:3-23
 *   glgym_rng_crop_noise / glgym_rng_reset_draw <- the same two draws from the environment's own NumPy generator
 *                     (gymnasium seeding: Generator(PCG64(SeedSequence(seed)))), bit for bit: tomato_env.py:118, 236-241
 *   glgym_rule_based <- RuleBasedController.predict              gl_gym/environments/baseline.py:68-227
 *                     (constants gl_gym/configs/agents/rule_based.yml; caller experiments/evaluate_baseline.py:22)
 *   glgym_weather  <- load_weather_data (array part)              gl_gym/environments/utils.py:48-125
 *   glgym_rhs      <- ODE(x,u,d,p) (test hook; no reference binding) gl_gym/environments/models/ode.hpp:6-124
 *   glgym_plan_fork / _accumulate / _rollout / _select, glgym_plan_sample / _elites / _refit <- no counterpart (the reference's
 *                     README lists MPC as a next step): sampling MPC on forked copies of the environments, one-shot (random
 *                     shooting, MPPI) and iterated (the cross-entropy method: sample, rank the elites, refit), all on the device
 *   glgym_plan_es_sample / _es_utilities / _es_update <- no counterpart: an evolution strategy over the same blocks (mirrored
 *                     sampling, centred ranks of the whole population, a search-gradient step on mean and spread), for policy search
 *   glgym_plan_cma_sample / _cma_update <- no counterpart: CMA-ES with a full covariance matrix per row (a correlated sample, rank-one
 *                     and rank-mu update, step-size control, a Cholesky factorisation), for the few constants of the rule-based controller
 *   glgym_plan_scenario / _rollout_scenarios / _aggregate <- the draw of noise.py:3-23 (parametric_crop_uncertainty) inside the
 *                     planning horizon, with common random numbers across candidates, and a risk score over the sampled futures
 *
 * Layouts.  "SoA [n][ld]" = n planes of ld elements, element (i, b) at base[i*ld + b]; lane b of a
 * wavefront touches consecutive addresses.  Element type T is float (GLGYM_F32) or double (GLGYM_F64).
 */
#ifndef GLGYM_H
#define GLGYM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLGYM_NX 28
#define GLGYM_NU 6
#define GLGYM_ND 10        /* columns the model reads; glgym_create accepts nd = 10..16 = row stride of weather / d */
#define GLGYM_NP 208
#define GLGYM_NCROP 34      /* p[128..161], the block noise.py perturbs */
#define GLGYM_NINFO 11      /* EPI, revenue, variable_costs, fixed_costs, co2_cost, heat_cost, elec_cost,
                               temp_violation, co2_violation, rh_violation, lamp_violation (tomato_env.py:208-222) */
#define GLGYM_NMETRIC 14    /* sum reward, sum EPI, n done, n failed integrations, sum co2/temp/rh violation, n env-steps,
                               n guard retries (extra attempts of the n_sub, 2x, 4x, 8x ladder: unverified or -- verified
                               mode -- every env-step's second attempt), n refined sub-steps (sub-steps beyond n_sub that the
                               stability control inserted: storms, wet screens pinned to the air temperature), then why
                               first attempts were unverified: n error-estimate flags, n branch-invariant flags, n cap /
                               non-finite flags, n heavy (>= 3x the nominal sub-steps) */
#define GLGYM_METRIC_BDF 14 /* env-steps with GLGYM_INTEGRATOR_BDF (glgym_set_step_integrator) add slots 0..7 as above, leave slots 8..13
                               at 0 and add to slots 14..17 = sum BDF steps, right-hand-side evaluations, Jacobians, LU factorisations.
                               GLGYM_NMETRIC stays the count of the explicit kernels' slots. */
#define GLGYM_METRIC_REPLICAS 64   /* accumulator blocks, one 128-byte line each (atomics onto a single line serialise) */
#define GLGYM_METRIC_STRIDE 32     /* floats per replica */

typedef struct glgym_handle_s* glgym_handle;

typedef enum { GLGYM_F32 = 0, GLGYM_F64 = 1 } glgym_dtype;

/* Right-hand side variants of gl_gym/environments/models/ode.hpp.  GLGYM_ODE = ODE (:6-124), what the reference's
 * compiled module integrates.  GLGYM_ODE_PIPE = ODE_pipe (:126-263): columns 10..13 of each weather / d row are
 * (tPipe, tGroPipe, pipeSwitchOff, groPipeSwitchOff); dxdt(9) = d10 - x9 unless d10 < 1 or d12 > 0, dxdt(19) = 0.
 * Its tracking term has rate 1 1/s, which the stability control accounts for (smaller sub-steps while tracking when
 * dt / n_sub > 2.5 s; none needed at dt = 300, n_sub = 256, experiments/gl_predefined_controls.py's setting). */
typedef enum { GLGYM_ODE = 0, GLGYM_ODE_PIPE = 1 } glgym_variant;

/* Sub-stepping scheme of glgym_step / glgym_evalF (greenlight_model.cpp:46-63 uses CVODES BDF, error-controlled and
 * implicit; any scheme that meets the accuracy bar against it is admissible).  n_sub is the NOMINAL (= minimum) number
 * of sub-steps per env-step.  Both schemes are stability-controlled per environment: a bound on the fastest local
 * relaxation rate (top-compartment exchange 0.2-0.7 1/s, up to 1.1 1/s in storms; a wet screen pinned to
 * the air temperature 3 ... 15 1/s) is evaluated at the start of every window of 1-4 nominal sub-steps; a window whose bound asks
 * for shorter sub-steps is itself shortened (round 5: 6 % over the limit costs 6 % more stages; a pinned surface's burst is looked at
 * again after 1-2 s), and beyond that the environment takes as many smaller sub-steps in the window as its scheme's stability
 * interval asks for; an embedded error estimate is the safety net.  An attempt that is flagged (error estimate, non-finite, rate beyond 64x the nominal count for more than 120 s,
 * a wet surface that changed sides inside its bistable regime in a capped window) or that took 3x the nominal number of sub-steps is UNVERIFIED:
 * the env-step is redone with 2x, 4x, 8x n_sub until an attempt is clean or two consecutive attempts agree on the fast states
 * (step doubling; counted in GLGYM_NMETRIC).  An environment for which no two attempts agree is reported like a failed CVODES
 * call in the reference (tomato_env.py:119-123): done = 1, state unchanged (glgym_step) / GLGYM_EODE (glgym_evalF).
 *   GLGYM_SCHEME_RK4: RK4 (stability interval 2.785) with the one fast LINEAR mode of the model taken out of it: the conduction
 *     between the two faces of the cover glass (hCovInCovE, aux_states.hpp:918 / ode.hpp:37-42; 0.65 1/s, state-independent) is
 *     integrated exactly -- Cox-Matthews' exponential RK4 on w = tCovIn - tCovE, classical RK4 on every other state.  The
 *     nominal sub-step is then set by the top compartment's air exchange: use n_sub 240 (nominal environments cover rates up to
 *     0.68 1/s).  The slow sub-expressions and the
 *     harvest flow are evaluated once per window of four nominal sub-steps in both precisions (n_sub is rounded up to a multiple of 4).
 *     That window is what sets the accuracy at a given n_sub (max scaled error on the tight one-step tuples, fp64: 6.2e-5 at 240,
 *     1.5e-5 at 480, 8.7e-6 at 640, 6.9e-6 at 720; 10-day rollout 1.5e-5 at 240): for PARITY runs against the reference's solver set
 *     n_sub 640, which sits inside the 1.3e-5 band of a BDF solve at the reference's tolerances (tests/test_gpu_parity.py).
 *   GLGYM_SCHEME_RK2: the midpoint rule of the same family (ETD2RK on the cover conduction, explicit midpoint elsewhere; stability
 *     interval 2.0): use n_sub 336.  30 % fewer right-hand sides than RK4; the slow sub-expressions and the harvest flow are shared
 *     by four nominal sub-steps (n_sub is rounded up to a multiple of 4).  Second order: the least accurate of the three (tight
 *     one-step tuples 3.2e-5, storm fixture 2.9e-5 in fp64).
 *   GLGYM_SCHEME_RK3: the three-stage, third-order member of the same exponential family (Cox-Matthews ETD3RK on the cover
 *     conduction, Kutta's RK3 -- stages at 0, h/2, h -- on every other state; stability interval 2.513): use n_sub 270.  19 % fewer
 *     right-hand sides than RK4 at RK4-like accuracy (the error of both is set by the slow tier's window, not by the order); the
 *     slow sub-expressions and the harvest flow are shared by three nominal sub-steps (n_sub is rounded up to a multiple of 3).
 *     (Rounds 2-3 shipped Bogacki-Shampine 3(2) with the conduction in its right-hand side at n_sub 354 under this name.)
 *   GLGYM_SCHEME_LS5 (round 5; the Python layer's default): a FIVE-stage FOURTH-order explicit Runge-Kutta scheme in Williamson's 2N-storage
 *     form (two registers per state: dy <- A_i dy + h f(y), y <- y + B_i dy).  The 2N five-stage fourth-order family has one free
 *     parameter, the z^5 coefficient of its stability polynomial; Carpenter-Kennedy's published member (1/200) has a real-axis stability
 *     interval of 4.657, the member used here (0.0047) 5.009 with |R| <= 0.28 at its working point: 1.00 per right-hand side against
 *     RK4's 0.70.  (Members with a longer interval settle on spurious quasi-steady states of the strongly ventilated top compartment
 *     beyond h lambda ~ 4.1; this one shows none up to its limit.)  The cover conduction is integrated exactly here too (Lawson's
 *     transformation applied to the deviation of the forcing from a linear predictor: exact for a linearly varying forcing, no stage
 *     history).  Use n_sub 128 (7.03 s sub-steps: rates up to 0.655 1/s); the slow sub-expressions and the harvest flow are shared by TWO
 *     nominal sub-steps (14 s; RK4-240: 15 s): 640 right-hand sides + 64 windows per env-step where RK4 takes 960 + 60, at RK4's accuracy
 *     or better on every fixture (tight one-step tuples 5.4e-5, 10-day rollout 1.3e-5 in fp64; RK4 at 240: 6.1e-5 / 1.5e-5) and on the wide
 *     random stress (43 of 5 954 one-step maps above 1e-4 against RK4-240's 49).  Its stability control differs from the other schemes' in
 *     two measured points: the movement limiter's allowance grows with the head-room the window's rate bound leaves below the stability
 *     limit, and a window the limiter does bind re-partitions its remainder sub-step by sub-step (the initial layer of an env-step decays
 *     within seconds).  PARITY preset: n_sub 192 with glgym_set_window(h, 1): 9.1e-6 on the tight one-step tuples, inside the 1.3e-5 band
 *     of a BDF solve at the reference's tolerances, at 960 right-hand sides + 192 windows (RK4 needs n_sub 640: 2 560 + 160).
 *     oracle/studies/lsrk_study.py, stress_ls5.py; DESIGN.md section 2.7. */
typedef enum { GLGYM_SCHEME_RK4 = 0, GLGYM_SCHEME_RK2 = 1, GLGYM_SCHEME_RK3 = 2, GLGYM_SCHEME_LS5 = 3 } glgym_scheme;

/* Step-doubling VERIFIED integration: no attempt is accepted on its own -- the result is the finer of two agreeing attempts (at
 * least n_sub and 2 n_sub: 3x the work, 4e-7 median error instead of 2e-6) -- with ONE exception, in this mode and the unverified one
 * alike: when no two attempts of the ladder agree, the finest one (8x n_sub) is taken as it stands if nothing flagged it (env-steps
 * that start on a kink or pass a bifurcation are sensitive at the 1e-4 level for any solver).  glgym_step reports that per env-step
 * (step_flags: GLGYM_SF_ACCEPT_LAST_ALONE), as it reports a result accepted by agreement on attempts that carried a flag.  The reference's solver is error-controlled
 * (greenlight_model.cpp:46-63) and its raw-control entry points apply any u with no delta-u clip (tomato_env.py:148-173; the
 * rule-based controller bang-bangs, baseline.py:68-227): after an all-actuator jump an explicit scheme near its stability limit
 * can put a wet cover on the wrong branch with every in-step check green.
 *   GLGYM_VERIFY_AUTO (default): verified wherever the control can jump -- glgym_evalF, glgym_step(control = ...), and
 *     glgym_step(action = ...) when delta_u_max > 0.1; the reference's action path (delta_u_max = 0.1) runs unverified + guard.
 *   GLGYM_VERIFY_ALWAYS / GLGYM_VERIFY_NEVER: every / no entry point. */
typedef enum { GLGYM_VERIFY_AUTO = 0, GLGYM_VERIFY_ALWAYS = 1, GLGYM_VERIFY_NEVER = 2 } glgym_verify;

typedef enum {
    GLGYM_OK = 0,
    GLGYM_EINVAL = -1,   /* bad argument (sizes other than 28/6/10/208, null pointer, n_sub < 1 ...) */
    GLGYM_ENODEV = -2,   /* no usable HIP device */
    GLGYM_EHIP = -3,     /* a HIP runtime call failed; see glgym_last_error() */
    GLGYM_ENOMEM = -4,
    GLGYM_EODE = -5      /* glgym_evalF: the integration failed for at least one row (the reference's evalF raises on a
                            CVODES failure, greenlight_model.cpp:110); failed rows of x_next are NaN, the others valid */
} glgym_status;

/* Reward constants (gl_gym/configs/envs/TomatoEnv.yml:38-67; rewards.py:47-124). */
typedef struct {
    double elec_price, heating_price, co2_price, fruit_price, dmfm;
    double fixed_greenhouse_cost, fixed_co2_cost, fixed_lamp_cost, fixed_screen_cost;
    double pen_lamp;
    double co2_min, co2_max, temp_min, temp_max, rh_min, rh_max;
} glgym_reward_cfg;

/* ABI version of this header; glgym_abi_version() returns the library's.  5: glgym_step_args starts with struct_size (round 5);
 * 7: glgym_set_integrator / glgym_set_tolerances / glgym_get_solver_stats; later, still 7 (an added entry point, backward
 * compatible; no struct changed): glgym_set_step_integrator, GLGYM_SF_BDF, GLGYM_METRIC_BDF; glgym_rng_crop_noise, glgym_rng_reset_draw;
 * glgym_plan_fork, glgym_plan_accumulate, glgym_plan_rollout, glgym_plan_select; glgym_step_obs; glgym_step_obs_reset;
 * glgym_plan_sample, glgym_plan_elites, glgym_plan_refit; glgym_plan_scenario, glgym_plan_rollout_scenarios, glgym_plan_aggregate;
 * glgym_plan_weather; glgym_rule_rows, glgym_plan_rollout_rule; glgym_policy_rows, glgym_plan_rollout_policy; glgym_plan_es_sample,
 * glgym_plan_es_utilities, glgym_plan_es_update; glgym_last_step_build; glgym_last_evalf_build; glgym_plan_cma_sample,
 * glgym_plan_cma_update; glgym_plan_constrain; glgym_ac_rows, glgym_gae; glgym_ppo_batch, glgym_ppo_loss; glgym_sac_rows,
 * glgym_sac_rows_grad, glgym_sac_batch, glgym_sac_loss, glgym_polyak; glgym_lstm_cell, glgym_lstm_cell_grad, glgym_seq_batch */
#define GLGYM_ABI_VERSION 7

/* Device-pointer arguments of one batched env-step.  Exactly one of `action` / `control` is non-null. */
typedef struct {
    int32_t struct_size;       /* sizeof(glgym_step_args) as the CALLER compiled it: glgym_step refuses (GLGYM_EINVAL) a struct of another
                                  size instead of reading pointers that are not there (the struct grew by step_flags in round 4) */
    int32_t B;                 /* environments in this shard */
    int32_t ld;                /* leading dimension of every SoA array (>= B) */
    void* x;                   /* SoA [28][ld] T, in/out: state */
    void* u;                   /* SoA [6][ld]  T, in/out: previous control in, applied control out */
    const float* action;       /* [B][6] row-major f32 in [-1,1]: u <- clip(u + 0.1f*a, 0, 1)   (step)            */
    const void* control;       /* SoA [6][ld] T: u <- control                                    (step_raw_control) */
    const void* weather;       /* [weather_rows][nd] row-major T (nd of glgym_create), shared by all envs */
    int32_t weather_rows;
    const int32_t* w_off;      /* [B] first weather row of each env's episode                    */
    int32_t* timestep;         /* [B] in/out; row integrated over = w_off[b] + timestep[b]; then ++ */
    const void* crop_p;        /* SoA [34][ld] T per-env p[128..161] (config 5) or NULL = shared  */
    int32_t N;                 /* terminal test `timestep >= N` before the increment (episode = N+1 steps) */
    void* reward;              /* [ld] T out */
    void* info;                /* SoA [11][ld] T out, order of GLGYM_NINFO */
    uint8_t* done;             /* [B] out: terminated (season end, or ODE failure -> state left unchanged) */
    float* metrics;            /* [GLGYM_METRIC_REPLICAS][GLGYM_METRIC_STRIDE] f32 accumulators or NULL: wavefront w adds
                                  its sums (GLGYM_NMETRIC order) to replica w % GLGYM_METRIC_REPLICAS; the reader sums the
                                  replicas */
    int32_t* step_flags;       /* [B] out or NULL: how this env-step's integration went (the reference has no counterpart:
                                  CVODES either returns or throws, greenlight_model.cpp:110) -- GLGYM_SF_* bits below */
} glgym_step_args;

/* step_flags[b]: bits 0..4 = why the FIRST attempt was not accepted as it stood (0 = it was): 1 rate bound beyond 64x the nominal
 * sub-step count for more than 120 s, 2 non-finite, 4 error estimate above tolerance, 8 a wet surface changed sides inside its
 * bistable regime in a capped window, 16 it took >= 3x the nominal number of sub-steps.  Bits 8..10 = extra attempts used
 * (2x, 4x, 8x n_sub).  Bits 16..30 = sub-steps taken beyond the nominal n_sub, all attempts together (saturating at 32 767; bit 31 is
 * never set, so the word is non-negative as an int32).  How the returned state was accepted: */
#define GLGYM_SF_ACCEPT_AGREE_FLAGGED 32   /* two consecutive attempts agreed, but the accepted (finer) one carried a flag itself */
#define GLGYM_SF_ACCEPT_LAST_ALONE 64      /* the finest attempt (8x n_sub), unflagged, taken as it stood although it did not agree
                                              with the attempt before it -- in verified mode as well */
#define GLGYM_SF_FAILED 128                /* failed integration: done = 1, state unchanged */
/* With GLGYM_INTEGRATOR_BDF (glgym_set_step_integrator) the word is GLGYM_SF_BDF | (GLGYM_SF_FAILED on failure) | BDF steps taken << 16
 * (bits 16..30, saturating at 32 767); bits 0..6 and 8..10 are 0.  The totals of steps, right-hand sides, Jacobians and LU
 * factorisations go to metric slots GLGYM_METRIC_BDF..+3. */
#define GLGYM_SF_BDF 2048                  /* the env-step was integrated by the BDF integrator */

/* Device-pointer arguments of observation assembly (row-major output, what SB3 / Gymnasium consume).
 * Weather rows: env b shows row w_off[b] + k, k = max(timestep[b] - 1, 0), and its forecast block rows w_off[b] + k + 1 .. + Np.
 * Every row index is clamped to [0, weather_rows - 1] on its own: a window that runs past the table repeats the last row, a negative
 * w_off reads row 0 (the reference would raise an IndexError, or wrap around for a negative index).  weather_rows < 1 is refused
 * (GLGYM_EINVAL), here and in glgym_step_obs / glgym_step_obs_reset. */
typedef struct {
    int32_t B, ld;
    const void* x;             /* SoA [28][ld] T */
    const void* u;             /* SoA [6][ld]  T */
    const void* weather;       /* [weather_rows][10] T */
    int32_t weather_rows;
    const int32_t* w_off;      /* [B] */
    const int32_t* timestep;   /* [B] value AFTER the step's increment; 0 = freshly reset env */
    const float* start_day;    /* [B] day of year at reset */
    int32_t Np;                /* forecast rows (int(pred_horizon*86400/dt)); obs_dim = 23 + 5*Np with the default modules */
    float* obs;                /* [B][glgym_obs_dim(h, Np)] row-major f32 out */
    const uint8_t* mask;       /* NULL: every row.  Else only rows with mask[b] != 0 are recomputed ...            */
    float* term_obs;           /* ... after their CURRENT content was saved here ([B][dim], SB3 "terminal_observation");
                                  may be NULL */
} glgym_obs_args;

/* Device-pointer arguments of a masked reset. */
typedef struct {
    int32_t B, ld;
    const uint8_t* mask;       /* [B] reset env b iff mask[b] != 0; NULL = all */
    void* x;                   /* SoA [28][ld] T out: init_state(weather[w_off[b]]) */
    void* u;                   /* SoA [6][ld]  T out: zeros */
    int32_t* timestep;         /* [B] out: 0 */
    const void* weather;
    int32_t weather_rows;
    int32_t* w_off;            /* [B] in/out: first weather row of the episode.  With a start table (below) the kernel
                                  draws the new episode's start itself, otherwise it uses the value found here */
    /* optional start table (TomatoEnv.reset picks (growth_year, start_day) at random, tomato_env.py:236-244):
       entry j = R[0] mod n_starts (unsigned), R = Philox4x32-10(counter = {b, (uint32)episode[b], 0x5eed, 0}, key = {seed low
       word, seed high word}), b the env's index in the batch; episode[b] (taken as 0 where `episode` is NULL) is then incremented.
       The draw of env b depends on (b, episode[b], seed) alone -- not on B, the mask or the launch geometry.  The third counter
       word 0x5eed keeps the stream apart from glgym_crop_noise's, whose counter is {b, draw low, draw high, block 0..8}.
       The state comes from row clamp(w_off[b], 0, weather_rows - 1); weather_rows < 1 is refused (GLGYM_EINVAL). */
    const int32_t* start_rows; /* [n_starts] or NULL */
    const float* start_days;   /* [n_starts] day of year of each start row */
    int32_t n_starts;
    float* start_day;          /* [B] out: day of year of the drawn start */
    int32_t* episode;          /* [B] in/out: episodes started so far per env */
    uint64_t seed;
} glgym_reset_args;

const char* glgym_version(void);
int glgym_abi_version(void);                                 /* GLGYM_ABI_VERSION the library was built with */
const char* glgym_last_error(void);

/* p: host, np doubles (the reference promotes its float32 parameter block to double before evalF). */
int glgym_create(int nx, int nu, int nd, int np, double dt, const double* p, int dtype, int n_sub, int device,
                 glgym_handle* out);
int glgym_destroy(glgym_handle h);
int glgym_set_params(glgym_handle h, const double* p);
/* The reference's `env.p = new_p` on an env that already exists (experiments/run_time.py:40-41, gl_predefined_controls.py:70-77): the model, the
 * crop block and the per-step cost coefficients of the reward follow new_p (rewards.py:164-166 read env.p at every step), but the reward's SCALE
 * -- max_profit / min_profit -- stays what it was at construction (rewards.py:82-83 computes them once, in __init__).  glgym_set_params
 * recomputes the scale too, i.e. it is "construct the env with new_p".  (ABI 6) */
int glgym_set_params_keep_reward_scale(glgym_handle h, const double* p);
int glgym_set_n_sub(glgym_handle h, int n_sub);
int glgym_set_scheme(glgym_handle h, int scheme);            /* GLGYM_SCHEME_RK4 (default) | GLGYM_SCHEME_RK2 | GLGYM_SCHEME_RK3 | GLGYM_SCHEME_LS5 */
/* Nominal sub-steps per tier-2b / harvest window.  0 (default) = the scheme's own (RK4 4, RK2 4, RK3 3, LS5 2); 1..8 overrides it at run
 * time (n_sub is rounded up to a multiple).  The window's length in seconds is what sets the accuracy at a given n_sub. */
int glgym_set_window(glgym_handle h, int window);
/* Kernel layout of glgym_step for GLGYM_F32 handles (GLGYM_F64 has one layout).  Initial value: environment variable GLGYM_LAYOUT =
 * one | quad read ONCE at glgym_create (A/B tools), else AUTO. */
typedef enum { GLGYM_LAYOUT_AUTO = 0, GLGYM_LAYOUT_ONE = 1, GLGYM_LAYOUT_QUAD = 2 } glgym_layout;
int glgym_set_layout(glgym_handle h, int layout);
/* Waves per SIMD the one-lane fp32 step kernel is built for: 1 (up to 512 registers, no scratch), 2 (256 registers, the windows' state
 * in LDS: two wavefronts share a SIMD) or 0 (default): 2 for batches of at least two wavefronts per SIMD (131 072 environments on
 * MI355X: 1.06-1.11x), 1 below.  Results of the two builds agree to rounding (tests/test_gpu_parity.py).  Initial value: GLGYM_OCC =
 * 1 | 2 read once at glgym_create. */
int glgym_set_occupancy(glgym_handle h, int waves_per_simd);
/* Verified glgym_evalF calls (GLGYM_VERIFY_AUTO / _ALWAYS) on batches that leave lanes free -- rows * 8 lanes <= one wavefront per SIMD of the
 * device: 8 192 rows on MI355X -- run the step-doubling ladder two rungs at a time on two lane groups per row (n_sub and 2 n_sub side by
 * side, then 4 n_sub and 8 n_sub if needed): the accepted attempt and the returned state are those of the sequential ladder bit for bit,
 * the elapsed time is the 2 n_sub attempt's instead of n_sub + 2 n_sub (profiles/r05_evalf_latency.txt).  Round 6: verified glgym_step
 * launches (control = ..., i.e. step_raw_control and the rule-based controller; four-lanes-per-environment kernels, shared crop block) on
 * batches of up to 8 192 environments do the same on two lane groups per environment, step_flags included.  1 (default) = where it
 * applies, 0 = always the sequential ladder (what per-row / per-env parameter blocks and larger batches run anyway). */
int glgym_set_ladder_parallel(glgym_handle h, int on);
int glgym_set_verify(glgym_handle h, int mode);              /* GLGYM_VERIFY_AUTO (default) | _ALWAYS | _NEVER */
/* action_to_control (tomato_env.py:109-113): u = clip(u_prev + action * delta_u_max, u_min, u_max), held in float32 like
 * base_env.py:72-74.  Default: the yml's [0, 1] bounds and 0.1 (configs/envs/TomatoEnv.yml:12-14).  The `control` input
 * of glgym_step (step_raw_control) is applied unclipped, as the reference does (tomato_env.py:148-149). */
int glgym_set_control_limits(glgym_handle h, const double* u_min /*[6]*/, const double* u_max /*[6]*/, double delta_u_max);
int glgym_set_model_variant(glgym_handle h, int variant);   /* GLGYM_ODE_PIPE needs a handle created with nd >= 14 */
int glgym_set_reward(glgym_handle h, const glgym_reward_cfg* cfg);
int glgym_get_reward_scale(glgym_handle h, double* max_profit, double* min_profit, double* fixed_costs);

/* Host pointers, row-major, double.  p_rows = 1 (one block for all rows) or B.  Synchronous.
 * The returned state is the caller's double x plus the increment computed in the handle's dtype: on a GLGYM_F32 handle the integration
 * starts from float(x), and the bits of x below fp32 spacing come back in x_next unchanged, in every build alike. */
int glgym_evalF(glgym_handle h, const double* x, const double* u, const double* d, const double* p, int p_rows,
                int B, double* x_next);
int glgym_rhs(glgym_handle h, const double* x, const double* u, const double* d, int B, double* dx);
/* Which build of the integrator kernels the handle's last glgym_evalF launched (the list of builds and the rules that choose among them:
 * csrc/gl_step_select.hpp, select_evalf).  out = family (0 one lane per row, 1 four lanes, 2 four lanes twice: the verification ladder
 * two rungs at a time), f64, crop (per-row crop blocks compiled in), pipe (GLGYM_ODE_PIPE compiled in), whether the launch integrated
 * GLGYM_ODE_PIPE (the fp64 builds choose at run time), sch (GLGYM_SCHEME_*), grid (workgroups of 64 lanes), rows (B of the launch).  A
 * GLGYM_INTEGRATOR_BDF call records family = -1, zeros and its rows.  A call that returns GLGYM_EINVAL leaves the record as it was, and
 * so does glgym_rhs; a call that falls back to one launch per row (parameter blocks that differ outside p[128..161]) leaves the record of
 * its last row.  Read-only host state, for tests and diagnostics; GLGYM_EINVAL before the handle's first glgym_evalF. */
int glgym_last_evalf_build(glgym_handle h, int32_t out[8]);

/* Integrator of glgym_evalF (ABI 7).  GLGYM_INTEGRATOR_EXPLICIT (default): the sub-stepping scheme above (glgym_set_scheme,
 * glgym_set_n_sub, glgym_set_window, glgym_set_verify).  GLGYM_INTEGRATOR_BDF: the algorithm family of the reference's CVODES
 * call (greenlight_model.cpp:46-63) -- adaptive, error-controlled, variable-order (1-5) BDF / NDF with modified Newton iterations
 * and a reused finite-difference Jacobian (Shampine & Reichelt 1997, the formulation of scipy.integrate.BDF), fp64 arithmetic for
 * either handle dtype, one wavefront per row; the scheme, n_sub, window and verify settings do not apply to it.  Per-row parameter
 * blocks are supported as for the explicit integrator.  A row that needs more than max_steps steps or 100 000 right-hand sides,
 * whose step size underflows (below 1e-12 dt) or that meets a non-finite value is a failed row: NaN, GLGYM_EODE.
 * glgym_evalF with GLGYM_ODE_PIPE returns GLGYM_EINVAL under BDF.  This setting governs glgym_evalF only: env-steps take theirs from
 * glgym_set_step_integrator, and a handle whose glgym_evalF integrator is BDF while its env-step integrator is explicit gets
 * GLGYM_EINVAL from glgym_step (a guard for callers that expected BDF env-steps).  glgym_rhs is unaffected. */
typedef enum { GLGYM_INTEGRATOR_EXPLICIT = 0, GLGYM_INTEGRATOR_BDF = 1 } glgym_integrator;
int glgym_set_integrator(glgym_handle h, int integrator);
/* Integrator of glgym_step.  GLGYM_INTEGRATOR_EXPLICIT (default): the sub-stepping kernels below.  GLGYM_INTEGRATOR_BDF: the same
 * row integrator as glgym_evalF's BDF (one 64-lane workgroup per environment, fp64 for either dtype) inside the env-step: controls
 * (action path clipped in T, raw controls unclipped) stored to u first, the weather row and the (shared or per-env) crop block in
 * double, the BDF step over dt at the glgym_set_tolerances settings, then the new state, reward, info and terminal test in T as the
 * explicit kernels compute them (x27 from the step counter).  On the same double inputs the state equals glgym_evalF's BDF bit for
 * bit.  A failed integration (step limit, the right-hand-side cap, step-size underflow, a singular matrix, a non-finite input)
 * leaves the state unchanged with done = 1, no gains and GLGYM_OK, as the explicit kernels do; no other environment is affected.
 * Scheme, n_sub, window, verify, layout, occupancy and ladder settings do not apply; GLGYM_ODE_PIPE gives GLGYM_EINVAL.  Launched on
 * the caller's stream without host copies or synchronisation (capturable).  Per-env step counts: step_flags; totals: metric slots
 * GLGYM_METRIC_BDF..+3. */
int glgym_set_step_integrator(glgym_handle h, int integrator);
/* Tolerances of GLGYM_INTEGRATOR_BDF, for glgym_evalF and glgym_step alike: rtol > 0, atol > 0 (the weighted RMS norm of the local
 * error, weights atol + rtol |x_i|), max_steps >= 1 steps per row (environment) and call.  Default 1e-6, 1e-6 (the reference's
 * abstol = reltol), 10 000. */
int glgym_set_tolerances(glgym_handle h, double rtol, double atol, int max_steps);
/* Solver statistics of the last glgym_evalF with GLGYM_INTEGRATOR_BDF, per row: stats[B][GLGYM_NSOLVER_STAT] = steps, right-hand
 * side evaluations, Jacobians, LU factorisations, final order.  B must be the batch size of that call.  (glgym_step does not
 * record them here: its per-env steps are in step_flags, its totals in metric slots GLGYM_METRIC_BDF..+3.) */
#define GLGYM_NSOLVER_STAT 5
int glgym_get_solver_stats(glgym_handle h, int B, int32_t* stats);

/* Observation modules (gl_gym/environments/observations.py:59-182), concatenated per row in the order of
 * TomatoEnv's `observation_modules` list (tomato_env.py:77-81, 193-198).  Default: all six in configs/envs/TomatoEnv.yml
 * order.  glgym_set_obs_modules takes 1..6 distinct ids; glgym_obs_dim returns the resulting row width (< 0 on error).
 * The reference's seventh entry, StateObservations (:35-57), cannot be constructed by TomatoEnv (its __init__ takes no env)
 * and returns random numbers; it is not offered. */
enum { GLGYM_OBS_INDOOR = 0,    /* IndoorClimateObservations  co2_air [ppm], temp_air, rh_air, pipe_temp          (4) */
       GLGYM_OBS_CROP = 1,      /* BasicCropObservations      24CanTemp (x21), cFruit (x25), tSum (x26)            (3) */
       GLGYM_OBS_CONTROL = 2,   /* ControlObservations        uBoil, uCo2, uThScr, uVent, uLamp, uBlScr            (6) */
       GLGYM_OBS_WEATHER = 3,   /* WeatherObservations        glob_rad, temp_out, rh_out, co2_out [ppm], wind      (5) */
       GLGYM_OBS_TIME = 4,      /* TimeObservations           timestep, sin/cos day of year, sin/cos hour of day   (5) */
       GLGYM_OBS_FORECAST = 5   /* WeatherForecastObservations raw weather columns 0..4 of the next Np rows    (5 Np) */ };
int glgym_set_obs_modules(glgym_handle h, const int32_t* modules, int n);
int glgym_obs_dim(glgym_handle h, int Np);

/* Device pointers; asynchronous on `stream` (a hipStream_t, NULL = default stream).
 * glgym_step picks its kernel layout per launch.  GLGYM_F64: four lanes per environment (csrc/gl_model_quad.hpp) in every scheme,
 * ODE variant and batch size -- the only fp64 integrator on the device.  GLGYM_F32: four lanes per environment for B <= 16 384 with
 * shared crop parameters and the default ODE (every scheme), one lane per environment otherwise; glgym_set_layout overrides that choice
 * (fp32 only).  Same scheme decision for decision in both layouts; results equal to fp32 rounding accumulated over the sub-steps
 * (measured on the storm / jump fixtures: <= 2.5e-4 scaled between the two fp32 layouts, tests/test_gpu_storm.py). */
int glgym_step(glgym_handle h, const glgym_step_args* a, void* stream);
/* Which build of the step kernel the handle's last successful glgym_step / glgym_step_obs / glgym_step_obs_reset launched (the list of
 * builds and the rules that choose among them: csrc/gl_step_select.hpp).  out = family (0 one lane per environment, 1 four lanes,
 * 2 four lanes twice: the verification ladder two rungs at a time), f64, crop (per-env crop blocks compiled in), def (the default
 * parameter block compiled in), pipe (GLGYM_ODE_PIPE compiled in), sch (GLGYM_SCHEME_*), epi (0, 8 observation epilogue, 24 observation
 * and auto-reset epilogue), occ (waves per SIMD the build is compiled for), grid (workgroups of 64 lanes), fused (0 the step alone,
 * 1 the launch wrote the observation rows, 2 it also did the auto-reset).  A GLGYM_INTEGRATOR_BDF env-step records family = -1 and
 * zeros.  Read-only host state, for tests and diagnostics; GLGYM_EINVAL before the handle's first step. */
int glgym_last_step_build(glgym_handle h, int32_t out[10]);
int glgym_obs(glgym_handle h, const glgym_obs_args* a, void* stream);
/* Exactly glgym_step(h, step, stream) followed by glgym_obs(h, obs, stream) in full mode; obs->mask must be NULL (GLGYM_EINVAL).
 * Both argument blocks are checked before anything is launched.  ONE launch where the handle's configuration has a step kernel with the
 * observation epilogue: GLGYM_F32, one lane per environment, the default ODE, any scheme, shared or per-env crop parameters, either
 * occupancy build, a row of at most 512 columns (292 in the two-waves build; the default modules up to Np = 97 / 53), `obs` 16-byte aligned, and x / u / weather / w_off /
 * timestep / B / ld the same in both blocks.  Each wavefront then writes the observation rows of its own 64 environments as soon as it
 * has finished integrating -- while the launch waits for its slowest wavefront anyway -- with the same bits glgym_obs writes.  Everywhere
 * else (four lanes per environment, GLGYM_F64, GLGYM_ODE_PIPE, GLGYM_INTEGRATOR_BDF env-steps, wider rows, differing buffers) the two
 * kernels are launched back to back; the caller never needs to know which.  Never synchronises (capturable like the calls it replaces). */
int glgym_step_obs(glgym_handle h, const glgym_step_args* step, const glgym_obs_args* obs, void* stream);
int glgym_reset(glgym_handle h, const glgym_reset_args* a, void* stream);
/* One env-step with auto-reset.  Exactly glgym_step_obs(h, step, obs in full mode, stream), then glgym_reset(h, reset with mask = step->done,
 * stream), then glgym_obs(h, obs with mask = step->done, stream): step->done is the mask of both, whatever the two blocks say (their
 * `mask` must be NULL or step->done itself: GLGYM_EINVAL otherwise); obs->term_obs receives the rows of the finished environments as
 * they were before the reset (may be NULL).  Afterwards x / u / timestep / w_off / start_day / episode hold the POST-RESET state of the
 * finished environments and `obs` their first observation; done, reward, info, step_flags and the metrics are the step's.
 * ONE launch where glgym_step_obs is one launch and in addition the crop parameters are shared (step->crop_p NULL), `reset` carries a
 * start table (start_rows, start_days, n_starts > 0, start_day, episode) and names the step's buffers (x, u, timestep, weather, w_off,
 * B, ld; start_day the observation's): each wavefront that holds a finished environment then does the three steps for it right after
 * writing its rows, with the same bits; a wavefront that holds none executes one test.  Everywhere else -- four lanes per environment,
 * GLGYM_F64, GLGYM_ODE_PIPE, GLGYM_INTEGRATOR_BDF env-steps, per-env crop blocks, rows wider than glgym_step_obs's limit, no start
 * table (as with glgym_rng_reset_draw) -- the kernels are launched back to back, with the same results.  All three
 * argument blocks are checked before anything is launched.  Never synchronises (capturable).
 * fused (may be NULL): set to 1 when the call was the one launch, to 0 when it launched the kernels back to back. */
int glgym_step_obs_reset(glgym_handle h, const glgym_step_args* step, const glgym_obs_args* obs, const glgym_reset_args* reset,
                         void* stream, int32_t* fused);
/* crop_p[i][b] = fl(p[128+i] * (1 + U(-scale/2, scale/2))), then p144 = p141/p142; Philox4x32-10 keyed by
 * (seed, stream_id), counter (env index, draw_index).  crop_p: SoA [34][ld] T. */
int glgym_crop_noise(glgym_handle h, void* crop_p, int B, int ld, double scale, uint64_t seed, uint64_t draw_index,
                     void* stream);

/* ---- the reference's seeded random stream on the device (csrc/gl_pcg64.hpp, csrc/glgym_rng.hip) -------------------------
 * The reference's TomatoEnv draws everything random from one NumPy generator per environment, np_random(seed) =
 * Generator(PCG64(SeedSequence(seed))) (gymnasium.utils.seeding; env `rank` of make_vec_env is seeded with seed + rank,
 * gl_gym/RL/utils.py:39).  These two entry points make the same draws from the same streams, so that a seeded run walks the
 * reference's episodes: same start days, same perturbed crop parameters, bit for bit.  Opt-in; glgym_crop_noise and glgym_reset's own
 * start draw (Philox) are unchanged.
 * rng_state: caller-owned device buffer, SoA uint64 [5][ld]: PCG64 state low / high word, increment low / high word, and NumPy's
 * 32-bit buffer as has_uint32 << 32 | uinteger -- the fields of `bit_generator.state`, filled by the caller (seeding runs on the host).
 * Asynchronous on `stream`, no host synchronisation (capturable).
 *
 * glgym_rng_crop_noise <- parametric_crop_uncertainty(self.p, self.uncertainty_scale, self._np_random) (noise.py:16-22, called at
 *   tomato_env.py:118, 150 in EVERY step, also with scale 0): noise = uniform(-scale/2, scale/2, 34), i.e. lo + (hi - lo) *
 *   (next_uint64 >> 11) * 2^-53; crop_p[i][b] = float32(double(p_i) + noise_i * double(p_i)) for p_i = float32(p[128+i]), product and
 *   sum rounded separately; then p144 = p141 / p142 in float32.  crop_p: SoA [34][ld] T as glgym_step_args.crop_p reads it, or NULL:
 *   the streams only advance by the 34 draws (the step then uses the handle's parameters, as with uncertainty_scale = 0).
 * glgym_rng_reset_draw <- growth_year = choice(years); start_day = choice(days) (tomato_env.py:236-241): for every environment with
 *   mask[b] != 0 (mask NULL: all) iy = bounded(n_years), id = bounded(n_days) -- Generator.choice of a list of n draws nothing for
 *   n = 1 and otherwise one buffered 32-bit word through Lemire's rejection method -- and entry j = iy * n_days + id of the year-major
 *   start table [n_years * n_days]: w_off[b] = start_rows[j], start_day[b] = start_days[j] (start_day / start_days may be NULL).
 *   Call glgym_reset afterwards WITHOUT a start table (start_rows NULL): it initialises from w_off[b]. */
int glgym_rng_crop_noise(glgym_handle h, void* crop_p, int B, int ld, double scale, uint64_t* rng_state, void* stream);
int glgym_rng_reset_draw(glgym_handle h, int B, int ld, const unsigned char* mask, uint64_t* rng_state, int n_years, int n_days,
                         const int32_t* start_rows, const float* start_days, int32_t* w_off, float* start_day, void* stream);

/* ---- device-side planning: fork, horizon rollouts, selection (csrc/gl_plan.hpp, csrc/glgym_plan.hip; selection: csrc/glgym_search.hip)
 * Sampling-based MPC (random shooting, MPPI) on the device: from the current state of each of P parent environments, K candidate
 * control sequences are simulated over H env-steps on COPIES of the parent (children, C = P * K of them, in caller-owned buffers of
 * their own leading dimension), scored by their discounted return, and the best is picked per parent.  The parents' buffers are only
 * read.  The reference has no counterpart (its README lists MPC as a next step).  Every args struct starts with struct_size and is
 * refused (GLGYM_EINVAL) on a mismatch, like glgym_step_args.  Asynchronous on `stream`, no host synchronisation, no allocation
 * (capturable).  Opt-in: no other entry point changes.
 *
 * Child accumulators, all caller-owned device arrays indexed by child: ret double [C] (discounted return), viol double SoA [3][ld]
 * (sums of co2 / temp / rh violation: info rows 8, 7, 9), n_steps int32 [C], alive uint8 [C] (1 until the step that reports done),
 * failed uint8 [C] (a step carried GLGYM_SF_FAILED). */
typedef struct {
    int32_t struct_size;
    int32_t n_children;          /* C */
    int32_t n_parents;           /* P */
    int32_t K;                   /* parent == NULL: the parent of child c is c / K (needs C <= P * K) */
    int32_t ld_parent, ld_child; /* leading dimensions of the parent / child SoA arrays (>= P / >= C) */
    const int32_t* parent;       /* [C] parent index per child, or NULL.  A child whose index is outside 0..P-1 copies parent 0 and
                                    starts with alive = 0, failed = 1 */
    const void* x_parent;        /* SoA [28][ld_parent] T */
    const void* u_parent;        /* SoA [6][ld_parent] T */
    const int32_t* timestep_parent;   /* [P] */
    const int32_t* w_off_parent;      /* [P] */
    const float* start_day_parent;    /* [P] or NULL (then start_day is not written) */
    const void* crop_parent;     /* SoA [34][ld_parent] T or NULL (then crop is not written) */
    void* x;                     /* SoA [28][ld_child] T out */
    void* u;                     /* SoA [6][ld_child] T out */
    int32_t* timestep;           /* [C] out */
    int32_t* w_off;              /* [C] out */
    float* start_day;            /* [C] out or NULL */
    void* crop;                  /* SoA [34][ld_child] T out or NULL */
    double* ret;                 /* [C] out: 0 */
    double* viol;                /* SoA [3][ld_child] out: 0 */
    int32_t* n_steps;            /* [C] out: 0 */
    uint8_t* alive;              /* [C] out: 1 */
    uint8_t* failed;             /* [C] out: 0 */
} glgym_plan_fork_args;

/* After ONE glgym_step on the children: for every child that was alive BEFORE that step, ret += w * (double)reward (product and sum
 * rounded separately), viol += (double)info rows 8, 7, 9, n_steps += 1, failed |= step_flags & GLGYM_SF_FAILED, alive &= !done.  The
 * step that reports done is counted and nothing after it (the reference's episode of N + 1 steps). */
typedef struct {
    int32_t struct_size;
    int32_t B, ld;               /* children, leading dimension of info / viol (reward is [ld]) */
    double w;                    /* weight of this step's reward (gamma^k) */
    const void* reward;          /* [ld] T: glgym_step_args.reward */
    const void* info;            /* SoA [11][ld] T: glgym_step_args.info */
    const uint8_t* done;         /* [B]: glgym_step_args.done */
    const int32_t* step_flags;   /* [B]: glgym_step_args.step_flags, or NULL (failed is then left alone) */
    double* ret;
    double* viol;
    int32_t* n_steps;
    uint8_t* alive;
    uint8_t* failed;
} glgym_plan_accumulate_args;

/* H env-steps of the children in one call: for k = 0 .. H-1 glgym_step(step with the action / control of step k, metrics = NULL),
 * then glgym_plan_accumulate with w_0 = 1, w_{k+1} = w_k * gamma (a running product in double).  The handle's settings apply as
 * they do to glgym_step (parameters, reward, scheme, n_sub, verify mode, explicit or BDF step integrator, GLGYM_ODE_PIPE with raw
 * controls); the handle's metric accumulators are not touched.  No reset and no noise draw happens (a per-env crop block is held over
 * the horizon; glgym_plan_rollout_scenarios below is the rollout that draws): a child past its season end keeps stepping on weather
 * rows clamped to the table and is ignored through alive.  Exactly one of actions / controls is non-null. */
typedef struct {
    int32_t struct_size;
    int32_t H;                   /* env-steps (>= 1) */
    double gamma;                /* discount factor (finite, >= 0) */
    glgym_step_args step;        /* the children's buffers; reward, info, done are required, step_flags may be NULL;
                                    step.action, step.control and step.metrics are ignored (set per step / NULL) */
    const float* actions;        /* [H][B][6] row-major f32: step k takes actions + k*B*6 (action path) */
    const void* controls;        /* [H] planes of SoA [6][ld] T: step k takes its plane (raw controls) */
    double* ret;                 /* accumulators as initialised by glgym_plan_fork */
    double* viol;
    int32_t* n_steps;
    uint8_t* alive;
    uint8_t* failed;
} glgym_plan_rollout_args;

/* One wavefront per parent over its K children.  best_k[p] = argmax of ret over the candidates that have not failed and whose ret is
 * finite, ties to the lowest k; best_ret[p] its return.  A parent without such a candidate gets best_k = -1, best_ret = NaN and
 * zeros (the action that holds the controls) in best_action / best_sequence / mean_sequence.  temperature > 0 with mean_sequence:
 * the MPPI mean, w_k = exp((ret_k - max) / temperature) over the same candidates, normalised; mean_sequence[h][p][j] =
 * sum_k w_k * actions[h][p*K + k][j], accumulated in double, stored f32. */
typedef struct {
    int32_t struct_size;
    int32_t P, K, H;
    const double* ret;           /* [P*K] */
    const uint8_t* failed;       /* [P*K] */
    const float* actions;        /* [H][P*K][6] f32, or NULL when none of the three action outputs is asked for */
    int32_t* best_k;             /* [P] out */
    double* best_ret;            /* [P] out */
    float* best_action;          /* [P][6] out = actions[0][p*K + best_k], or NULL */
    float* best_sequence;        /* [H][P][6] out or NULL */
    double temperature;          /* finite and > 0 with a finite 1 / temperature (above 2^-1024) with mean_sequence, else GLGYM_EINVAL;
                                    ignored otherwise */
    float* mean_sequence;        /* [H][P][6] out or NULL */
} glgym_plan_select_args;

int glgym_plan_fork(glgym_handle h, const glgym_plan_fork_args* a, void* stream);
int glgym_plan_accumulate(glgym_handle h, const glgym_plan_accumulate_args* a, void* stream);
int glgym_plan_rollout(glgym_handle h, const glgym_plan_rollout_args* a, void* stream);
int glgym_plan_select(glgym_handle h, const glgym_plan_select_args* a, void* stream);

/* ---- iterated sampling MPC: the cross-entropy method's stages between two rollouts (csrc/gl_cem.hpp, csrc/glgym_search.hip) ----
 * One CEM iteration is glgym_plan_sample -> glgym_plan_fork + glgym_plan_rollout -> glgym_plan_elites -> glgym_plan_refit: draw K
 * candidate sequences per parent from a Gaussian per (horizon step, parent, actuator), simulate them, rank each parent's returns,
 * refit mean and spread to the E best.  Same conventions as above: struct_size first, GLGYM_EINVAL before anything is launched,
 * asynchronous on `stream`, no allocation, no host synchronisation (capturable), plain vector stores, no atomics.  Opt-in: no other
 * entry point changes.  mean / std are [H][P][6] f32 (the layout of best_sequence), the action block [H][P*K][6] f32.
 *
 * glgym_plan_sample, one lane per child c = p*K + k.  Generator: Philox4x32-10; for child c, step h and D = draw_index + *draw_base
 * the counter is (c, 2h + blk, lo32(D), hi32(D)) for blk = 0, 1 and the key (lo32(seed), hi32(seed) ^ 0x43454d31), which gives the
 * words r0..r7.  In double, products and sums rounded separately: u_i = (r_i + 0.5) * 2^-32; e_2m = sqrt(-2 ln u_2m) cos(2 pi u_2m+1),
 * e_2m+1 the same with sin, m = 0, 1, 2 (r6, r7 unused); coloured noise per actuator n_0 = e_0, n_h = beta n_{h-1} +
 * sqrt(1 - beta^2) e_h; actions[h][c][j] = (float) clip(mean[h][p][j] + std[h][p][j] * n_h[j], -1, 1).  The words are exact; ln, cos
 * and sin are the device library's (a few double ulps from another libm: at most one float32 ulp in the stored action).
 * Reserved candidates: k = 0 is the clipped mean itself; with carry >= 1 candidate 1 <= k <= carry with k-1 < prev_n_elite[p] copies
 * the sequence of the previous population's elite k-1 from prev_actions (which must not be `actions`: ping-pong two blocks). */
typedef struct {
    int32_t struct_size;
    int32_t P, K, H;
    const float* mean;           /* [H][P][6] */
    const float* std;            /* [H][P][6] */
    double beta;                 /* 0 <= beta < 1: lag-1 correlation of the noise along the horizon */
    uint64_t seed;
    uint64_t draw_index;         /* which population this is: another value, other noise */
    const uint64_t* draw_base;   /* device word added to draw_index, or NULL: a replayed graph advances it instead of repeating itself */
    float* actions;              /* [H][P*K][6] out */
    int32_t carry;               /* >= 0; > 0 needs the four prev_ members and carry <= prev_E */
    int32_t prev_E;              /* row length of prev_elite_k */
    const float* prev_actions;   /* [H][P*K][6]: the previous population */
    const int32_t* prev_elite_k; /* [P][prev_E]: glgym_plan_elites of the previous population */
    const int32_t* prev_n_elite; /* [P] */
} glgym_plan_sample_args;

/* Per parent: elite_k[p][0..n-1] = the candidates that have not failed and whose ret is finite (glgym_plan_select's rule), by return
 * descending, ties to the lower k -- np.argsort(-ret, kind="stable") restricted to them -- cut at E; the rest of the row is -1;
 * n_elite[p] = n = min(E, number of such candidates).  Rank by counting over tiles of 256 returns staged in LDS: exact, O(K^2) per
 * parent, any K.  1 <= E <= K. */
typedef struct {
    int32_t struct_size;
    int32_t P, K, E;
    const double* ret;           /* [P*K] */
    const uint8_t* failed;       /* [P*K] */
    int32_t* elite_k;            /* [P][E] out */
    int32_t* n_elite;            /* [P] out */
} glgym_plan_elites_args;

/* One wavefront per (parent, horizon step).  Over a = actions[h][p*K + elite_k[p][e]][j], e < n = n_elite[p]: m = (1/n) sum a,
 * s = sqrt((1/n) sum (a - m)^2) (two passes, double); mean_out = (float)(alpha*mean + (1-alpha)*m), std_out =
 * (float) max(alpha*std + (1-alpha)*s, min_std).  A parent with n = 0 (or an elite index outside 0..K-1) keeps its mean and std.
 * mean_out / std_out may be mean / std.  0 <= alpha < 1, min_std >= 0, H <= 65 535. */
typedef struct {
    int32_t struct_size;
    int32_t P, K, H, E;
    const float* actions;        /* [H][P*K][6] */
    const int32_t* elite_k;      /* [P][E] */
    const int32_t* n_elite;      /* [P] */
    double alpha, min_std;
    const float* mean;           /* [H][P][6] */
    const float* std;
    float* mean_out;             /* [H][P][6] out */
    float* std_out;
} glgym_plan_refit_args;

int glgym_plan_sample(glgym_handle h, const glgym_plan_sample_args* a, void* stream);
int glgym_plan_elites(glgym_handle h, const glgym_plan_elites_args* a, void* stream);
int glgym_plan_refit(glgym_handle h, const glgym_plan_refit_args* a, void* stream);

/* ---- evolution strategy: mirrored sampling, centred ranks, search-gradient step (csrc/gl_es.hpp, csrc/glgym_search.hip) ---------
 * One ES iteration is glgym_plan_es_sample -> a rollout -> glgym_plan_es_utilities -> glgym_plan_es_update.  Same layouts and
 * conventions as the CEM stages above (mean / std [H][P][6] f32, the block [H][P*K][6] f32; struct_size first; every argument is
 * checked, GLGYM_EINVAL with a glgym_last_error text, before the handle is looked at and before anything is launched; asynchronous on
 * `stream`, no allocation, no host synchronisation (capturable), plain vector stores, no atomics).  Opt-in: no other entry point
 * changes.  K is EVEN and >= 2, M = K/2 pairs per distribution row p; pair m is the children c+ = p*K + 2m and c- = c+ + 1.
 * P*K <= INT32_MAX - 255, H <= 65 535.  Arithmetic in double, products and sums rounded separately.
 *
 * glgym_plan_es_sample, one lane per pair.  The six normals e of pair m at plane h are the CEM stream's of the EVEN child: words
 * r0..r7 of (c+, h, D = draw_index + *draw_base, seed) and the Box-Muller formula of glgym_plan_sample, drawn once.
 * actions[h][c+][j] = (float) clip(mean[h][p][j] + std[h][p][j] * e_j, -1, 1), actions[h][c-][j] the same with -e_j.  No reserved
 * candidates, no carry, no colouring: for even k >= 2 row c+ is bit for bit what glgym_plan_sample (beta = 0, carry = 0) stores.  A
 * lane stores its pair's 48 contiguous bytes as three 16-byte stores: `actions` must be 16-byte aligned. */
typedef struct {
    int32_t struct_size;
    int32_t P, K, H;
    const float* mean;           /* [H][P][6] */
    const float* std;            /* [H][P][6] */
    uint64_t seed;
    uint64_t draw_index;         /* which population this is */
    const uint64_t* draw_base;   /* device word added to draw_index, or NULL */
    float* actions;              /* [H][P*K][6] out, 16-byte aligned */
} glgym_plan_es_sample_args;

/* Centred ranks over the WHOLE population.  Admissibility and order are glgym_plan_elites': per row p, the n candidates that have
 * not failed and whose ret is finite, by np.argsort(-ret, kind="stable").  The candidate of rank r (0 = best) gets
 * u = 0.5 - (double) r / (double)(n - 1) (one subtraction, one division); an inadmissible candidate gets -0.5; with n < 2 every u of
 * the row is 0.  n_adm[p] = n.  Rank by counting over tiles of 256 returns staged in LDS, as glgym_plan_elites. */
typedef struct {
    int32_t struct_size;
    int32_t P, K;
    const double* ret;           /* [P*K] */
    const uint8_t* failed;       /* [P*K] */
    double* u;                   /* [P*K] out */
    int32_t* n_adm;              /* [P] out */
} glgym_plan_es_utilities_args;

/* One wavefront per (row p, plane h); it reads the plane's K rows of `actions` and the row's K utilities once.
 * With sigma_j = (double) std[h][p][j], per pair m: d_j = ((double) theta+_j - (double) theta-_j) * 0.5 (exact),
 *   the gradient term  (u+ - u-) * d_j,
 *   the spread term    (u+ + u-) * (z * z - 1) with z = d_j / sigma_j -- no term where sigma_j is not > 0.
 * Lane l adds its terms for m = l, l + 64, ... in ascending order, starting from 0; the 64 partial sums are combined by the butterfly
 * (xor 32, 16, .. 1) and divided by (double) M: g_j and s_j.  The step ASCENDS the return.  t = t_index + *t_base.
 *   GLGYM_ES_SGD:   step = lr * g.
 *   GLGYM_ES_ADAM:  m1 = beta1 * m1 + (1 - beta1) * g;  m2 = beta2 * m2 + (1 - beta2) * (g * g);
 *                   step = (lr * (m1 / (1 - beta1^t))) / (sqrt(m2 / (1 - beta2^t)) + eps), every operation rounded on its own, left to
 *                   right as bracketed.  b^t by square-and-multiply from the least significant bit of t: r = 1, q = b; while t != 0
 *                   { if t is odd r = r * q;  t = t >> 1;  if t != 0 q = q * q }.  m1, m2 [H][P][6] f64 belong to the caller (zero
 *                   them before t = 1).
 *   mean_out = (float)((double) mean + step)
 *   std_out  = (float) min(max((sigma * std_decay) * exp((0.5 * lr_std) * s), min_std), max_std)     (exp is the device library's)
 * The six components of (p, h) keep their mean, std and moments if n_adm[p] < 2, if any of the six g_j or s_j is not finite (a NaN in
 * theta), or if t = 0.  mean_out / std_out may be mean / std.  `actions` and `u` must be 16-byte aligned (a lane reads its pair's 48
 * bytes as three 16-byte loads, its two utilities as one).
 * Refused: lr or lr_std negative or not finite; std_decay not finite or not > 0; min_std negative, max_std not finite, min_std >
 * max_std; t_index = 0; with GLGYM_ES_ADAM beta1 or beta2 outside [0, 1), eps not finite or not > 0, m1 or m2 NULL (with GLGYM_ES_SGD
 * the three numbers and both pointers are ignored). */
enum { GLGYM_ES_SGD = 0, GLGYM_ES_ADAM = 1 };
typedef struct {
    int32_t struct_size;
    int32_t P, K, H;
    int32_t optimizer;           /* GLGYM_ES_SGD | GLGYM_ES_ADAM */
    const float* actions;        /* [H][P*K][6]: the population the utilities belong to */
    const double* u;             /* [P*K]: glgym_plan_es_utilities */
    const int32_t* n_adm;        /* [P] */
    double lr, lr_std, std_decay, min_std, max_std;
    double beta1, beta2, eps;
    uint64_t t_index;            /* >= 1: the step count */
    const uint64_t* t_base;      /* device word added to t_index, or NULL: a replayed graph advances it */
    double* m1;                  /* [H][P][6] in / out (GLGYM_ES_ADAM) */
    double* m2;
    const float* mean;           /* [H][P][6] */
    const float* std;
    float* mean_out;             /* [H][P][6] out */
    float* std_out;
} glgym_plan_es_update_args;

int glgym_plan_es_sample(glgym_handle h, const glgym_plan_es_sample_args* a, void* stream);
int glgym_plan_es_utilities(glgym_handle h, const glgym_plan_es_utilities_args* a, void* stream);
int glgym_plan_es_update(glgym_handle h, const glgym_plan_es_update_args* a, void* stream);

/* ---- CMA-ES with a full covariance matrix over few, strongly interacting components (csrc/gl_cma.hpp, csrc/glgym_search.hip) ----
 * One iteration is glgym_plan_cma_sample -> a rollout -> glgym_plan_elites -> glgym_plan_cma_update.  For the N <= GLGYM_CMA_NMAX
 * searched components of a rule-based controller (glgym_plan_rollout_rule); a policy net's hundreds of weights stay with the
 * separable stages above.  Same layouts and conventions as the ES stages: the block theta [Ht][P*K][6] f32 with Ht = ceil(N / 6),
 * component i at plane h = i / 6, slot j = i % 6; mean [Ht][P][6] f32; struct_size first; every argument is checked, GLGYM_EINVAL with
 * a glgym_last_error text, before the handle is looked at and before anything is launched; asynchronous on `stream`, no allocation,
 * no host synchronisation (capturable), plain vector stores, no atomics.  Opt-in: no other entry point changes.  Row p is one search
 * distribution with K candidates c = p*K + k and E elites.  1 <= N <= GLGYM_CMA_NMAX, 1 <= E <= K, P*K <= INT32_MAX - 255.
 * Arithmetic in double, every product and every sum rounded on its own, in the orders stated here.
 *
 * State per row, the caller's, updated in place: mean; sigma [P] f64 (the step size); cov [P][N][N] f64, symmetric, both triangles
 * stored (start: I); chol [P][N][N] f64, its lower Cholesky factor, the upper triangle zero (start: I); the evolution paths p_sigma
 * and p_c [P][N] f64 (start: 0).
 *
 * glgym_plan_cma_sample, one lane per child, the children of a block from one row.  z_i is component i of the normals of
 * glgym_plan_sample's stream: z_{6h+j} = e_j of (c, h, D = draw_index + *draw_base, seed).  y_i = sum_{j <= i} chol[p][i][j] * z_j,
 * from 0.0, j ascending, each product rounded, then added.  theta[h][c][j] = (float) clip(mean[h][p][j] + sigma[p] * y_i, -1, 1)
 * (product, then sum); the padding slots i >= N store 0.0f.  No reserved candidate, no carry, no colouring: with chol = I and std =
 * sigma the rows are bit for bit those of glgym_plan_sample (beta = 0, carry = 0) for k >= 1. */
#define GLGYM_CMA_NMAX 32
typedef struct {
    int32_t struct_size;
    int32_t P, K, N;
    const float* mean;           /* [Ht][P][6] */
    const double* sigma;         /* [P] */
    const double* chol;          /* [P][N][N] */
    uint64_t seed;
    uint64_t draw_index;         /* which population this is */
    const uint64_t* draw_base;   /* device word added to draw_index, or NULL */
    float* theta;                /* [Ht][P*K][6] out */
} glgym_plan_cma_sample_args;

/* One block per row.  It reads the STORED population (clipping and float32 rounding included) and no RNG.  x_e is the row of elite e
 * = elite_k[p][e] (glgym_plan_elites), e < E; t = t_index + *t_base; "old" is the row's state on entry.
 *   1. y_e[d] = ((double) x_e[d] - (double) mean[d]) / sigma                          (one subtraction, one division)
 *   2. yw[d] = sum_e w[e] * y_e[d]                                                    (from 0.0, e ascending)
 *   3. zw = chol_old^-1 yw by forward substitution: zw[i] = (yw[i] - sum_{j<i} chol[i][j] * zw[j]) / chol[i][i], each product
 *      subtracted in turn, j ascending
 *   4. q_s = sqrt((c_sigma * (2 - c_sigma)) * mu_eff);  p_sigma'[d] = (1 - c_sigma) * p_sigma[d] + q_s * zw[d]
 *   5. n2 = sum_d p_sigma'[d] * p_sigma'[d] (from 0.0, d ascending);  nrm = sqrt(n2)
 *   6. g = 1 - (1 - c_sigma)^(2t), the power by glgym_plan_es_update's square-and-multiply;
 *      h_sigma = nrm / sqrt(g) < (1.4 + 2 / (N + 1)) * chi_n
 *   7. q_c = sqrt((c_c * (2 - c_c)) * mu_eff);  p_c'[d] = (1 - c_c) * p_c[d] + (h_sigma ? q_c * yw[d] : 0.0)
 *   8. a0 = ((1 - c_1) - c_mu) + (h_sigma ? 0.0 : (c_1 * c_c) * (2 - c_c))
 *   9. for b <= a: R[a][b] = sum_e (w[e] * y_e[a]) * y_e[b] (from 0.0, e ascending);
 *      cov'[a][b] = (a0 * cov[a][b] + c_1 * (p_c'[a] * p_c'[b])) + c_mu * R[a][b];  cov'[b][a] is a copy
 *  10. mean'[d] = (float) clip((double) mean[d] + sigma * yw[d], -1, 1)
 *  11. sigma' = min(max(sigma * exp((c_sigma / d_sigma) * (nrm / chi_n - 1)), min_sigma), max_sigma)      (exp is the device library's)
 *  12. chol' = the Cholesky factor of cov', row-oriented: for j = 0 .. N-1: s = cov'[j][j] - sum_{k<j} chol'[j][k] * chol'[j][k],
 *      chol'[j][j] = sqrt(s); for i > j: chol'[i][j] = (cov'[i][j] - sum_{k<j} chol'[i][k] * chol'[j][k]) / chol'[j][j]; each
 *      product subtracted in turn, k ascending; the upper triangle is 0.
 * A row is updated whole or not at all; status[p] says which, the first of these that applies:
 *   4  t = 0
 *   1  n_elite[p] < E, or one of the E elite indices outside 0..K-1
 *   2  one of p_sigma', p_c', cov', mean', sigma' is not finite (a NaN in an elite's theta, say)
 *   3  a pivot s is not > 0
 *   2  an entry of chol' is not finite
 *   0  updated
 * In every case but 0 each piece of the row's state keeps its bits.
 * The weights are given twice: w, E doubles in HOST memory, read and checked by the call, and w_dev, the same E doubles in DEVICE
 * memory, which the kernel reads (the call copies nothing, so that it can be captured).  The library computes no logarithm: the
 * caller supplies the weights and the constants (Hansen's defaults: gl_gym_amd.planner.RuleSearch.cma_defaults).
 * Refused: N outside 1..GLGYM_CMA_NMAX; E outside 1..K; P < 1; P*K past INT32_MAX - 255; a constant or weight that is not finite; a
 * negative weight; c_sigma, c_c, c_1 or c_mu outside [0, 1]; c_1 + c_mu > 1; d_sigma, chi_n or mu_eff not > 0; min_sigma negative or
 * > max_sigma; t_index = 0; a NULL pointer (t_base may be NULL). */
typedef struct {
    int32_t struct_size;
    int32_t P, K, N, E;
    const float* theta;          /* [Ht][P*K][6]: the population the elites belong to */
    const int32_t* elite_k;      /* [P][E]: glgym_plan_elites */
    const int32_t* n_elite;      /* [P] */
    const double* w;             /* [E] HOST: the recombination weights, >= 0 */
    const double* w_dev;         /* [E] device: the same values */
    double mu_eff, c_sigma, d_sigma, c_c, c_1, c_mu, chi_n, min_sigma, max_sigma;
    uint64_t t_index;            /* >= 1: the generation count */
    const uint64_t* t_base;      /* device word added to t_index, or NULL */
    float* mean;                 /* [Ht][P][6] in / out */
    double* sigma;               /* [P] in / out */
    double* cov;                 /* [P][N][N] in / out */
    double* chol;                /* [P][N][N] in / out */
    double* p_sigma;             /* [P][N] in / out */
    double* p_c;                 /* [P][N] in / out */
    int32_t* status;             /* [P] out */
} glgym_plan_cma_update_args;

int glgym_plan_cma_sample(glgym_handle h, const glgym_plan_cma_sample_args* a, void* stream);
int glgym_plan_cma_update(glgym_handle h, const glgym_plan_cma_update_args* a, void* stream);

/* ---- robust planning: scenario rollouts under crop noise, risk-aware scores (csrc/gl_scen.hpp, csrc/glgym_plan.hip; scores: csrc/glgym_search.hip)
 * With uncertainty_scale > 0 the environment multiplies the 34 crop parameters p[128..161] by 1 + U(-scale/2, scale/2) at every
 * env-step (glgym_crop_noise).  Here every one of the P*K candidates is simulated under S sampled futures of that block -- children
 * c = (p*K + k)*S + s, C = P*K*S of them -- and scored by a risk measure over its S returns, which glgym_plan_select / _elites /
 * _refit then take as the candidate's return.  Same conventions as above: struct_size first, GLGYM_EINVAL before anything is
 * launched, asynchronous on `stream`, no allocation, no host synchronisation (capturable), plain vector stores, no atomics.  Opt-in:
 * no other entry point changes.
 *
 * Scenario crop block of child c at horizon step h.  D = draw_index + *draw_base, hh = hold ? 0 : h.  For blk = 0..8 the words
 * r[4*blk .. 4*blk+3] are Philox4x32-10 of the counter (p*S + s, lo32(D), hi32(D), 16*hh + blk) under the key (lo32(seed),
 * hi32(seed) ^ 0x5343454e).  The candidate k is NOT in the counter: scenario s of greenhouse p is the same future for all K
 * candidates (common random numbers), so that their scores differ by their actions alone.  For i < 34, with p_i the handle's
 * float32 p[128+i], in double with products and sums rounded separately: u = (r[i] + 0.5) * 2^-32, z = (u - 0.5) * scale,
 * t = z * p_i, v_i = (float)(p_i + t); then v[16] = v[13] / v[14] in float32 (cLeafMax = laiMax / sla, as glgym_crop_noise); stored as
 * T.  hold = 1: one parametric draw held over the horizon; hold = 0: a fresh draw at every step, the environment's own process. */
typedef struct {
    int32_t struct_size;
    int32_t P, K, S;             /* greenhouses, candidates per greenhouse, scenarios per candidate (S <= 256); P*K*S <= INT32_MAX */
    int32_t ld;                  /* leading dimension of crop (>= P*K*S) */
    int32_t h_step;              /* horizon step h, 0 .. 65 535 */
    int32_t hold;                /* 0 | 1 */
    double scale;                /* finite, >= 0 */
    uint64_t seed;
    uint64_t draw_index;         /* which set of scenarios this is: another value, other futures */
    const uint64_t* draw_base;   /* device word added to draw_index, or NULL */
    void* crop;                  /* SoA [34][ld] T out (required) */
    const float* actions_in;     /* [P*K][6] f32: the candidates' action plane of this step, or NULL */
    float* actions_out;          /* [P*K*S][6] f32 out: row c = actions_in row c / S; NULL exactly when actions_in is */
} glgym_plan_scenario_args;

/* H env-steps of the C = P*K*S children: for h = 0 .. H-1 glgym_plan_scenario(h) into rollout.step.crop_p and `staging`, glgym_step
 * with action = staging and metrics = NULL, glgym_plan_accumulate with the running-product weight -- glgym_plan_rollout's loop with
 * the prologue in front of every step.  rollout.step.B must be P*K*S and rollout.step.crop_p is required; rollout.actions is the
 * CANDIDATES' block [H][P*K][6] (one plane is expanded per step, never H of them); rollout.controls must be NULL.  What glgym_step
 * refuses with a crop block (GLGYM_ODE_PIPE) is refused here with glgym_step's own error, before anything is launched. */
typedef struct {
    int32_t struct_size;
    int32_t P, K, S;
    int32_t hold;
    double scale;
    uint64_t seed;
    uint64_t draw_index;
    const uint64_t* draw_base;
    float* staging;              /* [P*K*S][6] f32: caller-owned staging plane of the expanded actions */
    glgym_plan_rollout_args rollout;
} glgym_plan_rollout_scenarios_args;

/* One wavefront per candidate j over its S scenario returns r_s = ret[j*S + s].  If any failed[j*S + s] != 0 or any r_s is not
 * finite: ret_cand[j] = NaN, failed_cand[j] = 1.  Otherwise failed_cand[j] = 0 and, with a the returns in ascending order,
 * ret_cand[j] = (((0.0 + a_0) + a_1) + ... + a_{m-1}) / (double)m: m = S the mean, m = 1 the worst case, between them the mean of
 * the worst m (a CVaR-style tail mean).  viol_cand[i][j] = (sum over s in index order, from 0.0, of viol[i][j*S + s]) / (double)S;
 * steps_cand[j] = min over s of n_steps[j*S + s].  The returns are staged in LDS and ranked by counting (as glgym_plan_elites); one
 * lane then sums in rank order, so the result is the sequential sum above bit for bit.  Independent of the handle's dtype. */
typedef struct {
    int32_t struct_size;
    int32_t J, S, m;             /* candidates, scenarios per candidate (1 .. 256), tail length (1 .. S) */
    int32_t ld;                  /* leading dimension of viol (>= J*S) */
    int32_t ld_cand;             /* leading dimension of viol_cand (>= J) */
    const double* ret;           /* [J*S] */
    const uint8_t* failed;       /* [J*S] */
    const double* viol;          /* SoA [3][ld]; required with viol_cand */
    const int32_t* n_steps;      /* [J*S]; required with steps_cand */
    double* ret_cand;            /* [J] out */
    uint8_t* failed_cand;        /* [J] out */
    double* viol_cand;           /* SoA [3][ld_cand] out, or NULL */
    int32_t* steps_cand;         /* [J] out, or NULL */
} glgym_plan_aggregate_args;

int glgym_plan_scenario(glgym_handle h, const glgym_plan_scenario_args* a, void* stream);
int glgym_plan_rollout_scenarios(glgym_handle h, const glgym_plan_rollout_scenarios_args* a, void* stream);
int glgym_plan_aggregate(glgym_handle h, const glgym_plan_aggregate_args* a, void* stream);

/* ---- violation budgets and chance constraints in candidate ranking (csrc/gl_constr.hpp, csrc/glgym_search.hip) -----------------
 * A second scoring stage behind the rollout (and behind glgym_plan_aggregate, if there are scenarios): it turns the candidates'
 * returns and the accumulated violations of their runs (viol rows 0, 1, 2: CO2, temperature, humidity) into the scores that
 * glgym_plan_select / _elites / _es_utilities then rank.  Same conventions as above: struct_size first, GLGYM_EINVAL with a
 * glgym_last_error text before anything is launched, asynchronous on `stream`, no allocation, no host synchronisation (capturable),
 * plain vector stores, no atomics.  Independent of the handle's dtype.  Opt-in: no other entry point changes.
 *
 * Indexing.  P ranking groups, K candidates per group, R = O*S runs per candidate: candidate j = p*K + k owns the children
 * c = ((p*O + o)*K + k)*S + s, its run r = o*S + s (o-major, then s).  O = 1 is the layout of glgym_plan_rollout_scenarios (S = 1:
 * no scenarios); P = 1, O = B ranks K policies that each ran on all B greenhouses, at stride K*S.
 *
 * Everything is double; products, quotients and sums are rounded separately (no contraction).
 * Per run r, child c:  d = per_step ? (double)max(n_steps[c], 1) : 1.0;  for i = 0, 1, 2:  e_i = max(0.0, viol[i][c] / d -
 * budget[i]), except that e_i = +0.0 when budget[i] = +inf (the constraint is off, whatever viol holds: inf - inf never appears) and
 * when viol[i][c] is not finite under an active budget -- which marks the candidate failed instead;
 * g_r = ((0.0 + weight[0]*e_0) + weight[1]*e_1) + weight[2]*e_2.  The run violates when g_r > 0.
 * Per candidate j:  n_viol = the number of violating runs;  feasible = n_viol <= n_allow (n_allow = 0: every run within budget;
 * n_allow = floor(eps*R): a chance constraint over the sampled futures);  excess G = (sum of the g_r) / (double)R, where the sum has
 * a fixed, parallel order: lane l of 64 adds the runs with r = l, l + 64, l + 128, ... in ascending r, starting from 0.0 (a lane
 * without a run keeps 0.0), and the 64 lane sums are then added in lane order 0, 1, ..., 63, starting from 0.0;
 * failed_out = failed_cand | (a non-finite viol under an active budget) | (ret_cand is not finite), as 0 | 1.
 * Score.  mode = GLGYM_CONSTRAIN_PENALTY: score = ret_cand - rho*G.  mode = GLGYM_CONSTRAIN_FEASIBLE_FIRST (the constrained
 * cross-entropy ordering): call a candidate admissible when its failed_out is 0; floor_p = (the smallest ret_cand over group p's
 * admissible feasible candidates, or 0.0 when it has none) - 1.0; a feasible candidate scores ret_cand, an infeasible one
 * floor_p - G.  Every feasible candidate thus outranks every infeasible one of its group, feasible ones are ordered by return,
 * infeasible ones by ascending excess, and the gap between the two classes is at least 1 (up to the rounding of floor_p): argmax,
 * counting ranks, centred ranks and CMA weights produce the lexicographic order without knowing of it; only an exponentially
 * weighted mean sees the magnitudes.  In either mode a candidate with failed_out = 1 scores NaN.
 * n_feasible[p] = the number of admissible feasible candidates of group p. */
typedef enum { GLGYM_CONSTRAIN_PENALTY = 0, GLGYM_CONSTRAIN_FEASIBLE_FIRST = 1 } glgym_constrain_mode;

typedef struct {
    int32_t struct_size;
    int32_t P, O, K, S;          /* all >= 1; P*O*K*S <= INT32_MAX */
    int32_t ld;                  /* leading dimension of viol (>= P*O*K*S) */
    int32_t per_step;            /* 0 | 1: budgets per accumulated step, or on the run's totals */
    int32_t n_allow;             /* 0 .. R */
    int32_t mode;                /* glgym_constrain_mode */
    double budget[3];            /* >= 0, or +inf: off; NaN or a negative value is refused */
    double weight[3];            /* finite, >= 0 */
    double rho;                  /* finite, >= 0; read in penalty mode only */
    const double* ret_cand;      /* [P*K] */
    const uint8_t* failed_cand;  /* [P*K] */
    const double* viol;          /* SoA [3][ld] */
    const int32_t* n_steps;      /* [P*O*K*S]; required with per_step */
    double* score;               /* [P*K] out; must not overlap ret_cand */
    uint8_t* failed_out;         /* [P*K] out; may be failed_cand */
    uint8_t* feasible;           /* [P*K] out, or NULL */
    double* excess;              /* [P*K] out = G, or NULL */
    int32_t* n_viol;             /* [P*K] out, or NULL */
    int32_t* n_feasible;         /* [P] out, or NULL */
} glgym_plan_constrain_args;

int glgym_plan_constrain(glgym_handle h, const glgym_plan_constrain_args* a, void* stream);

/* ---- weather-forecast uncertainty in scenario rollouts (csrc/gl_wscen.hpp, csrc/glgym_plan.hip) ------------------------------
 * A rollout's children step on the true future rows of the weather table: perfect foresight.  glgym_plan_weather gives scenario s of
 * greenhouse p (ps = p*S + s) its own, wrong forecast instead: a private window of H rows -- row ps*H + h of `window`, the parent's
 * row at horizon step h with a forecast error on the seven columns the right-hand side reads (iGlob, tOut, vpOut, co2Out, wind,
 * tSky, tSoOut) -- and child offsets that point into it.  The step kernels read one row per env-step, clamp(w_off + timestep, 0,
 * weather_rows - 1): with step.weather = window, step.weather_rows = P*S*H and step.w_off = w_off_child a scenario rollout
 * (glgym_plan_rollout_scenarios, which is unchanged) integrates the children on their windows.  Same conventions as above:
 * struct_size first, GLGYM_EINVAL before anything is launched, asynchronous on `stream`, no allocation, no host synchronisation
 * (capturable), plain vector stores, no atomics.  Opt-in: no other entry point changes.
 *
 * Source row of (p, h): clamp(w_off_parent[p] + timestep_parent[p] + h, 0, weather_rows - 1), the row a plain child reads.
 * Innovation of (ps, h, column j < 7): r[0..3] = Philox4x32-10 of the counter (ps, lo32(D), hi32(D), 8*h + j) under the key
 * (lo32(seed), hi32(seed) ^ 0x5753434e), D = draw_index + *draw_base -- the scenario draw index of glgym_plan_scenario under another
 * key tag, so that one index moves both kinds of future.  In double, products and sums rounded separately: c_i = (r[i] + 0.5) * 2^-32
 * - 0.5; eps = (((c_0 + c_1) + c_2) + c_3) * 1.7320508075688772: four centred uniforms scaled to unit variance, |eps| < 3.47.
 * Error: e_0 = 0 (the row being integrated now is a measurement); e_h = phi*e_{h-1} + g_j*eps_h for h >= 1 (two products, one sum),
 * g_j = sqrt(1 - phi*phi) * sigma[j] with the root taken once on the host: lag-1 correlation phi, standard deviation sigma_j
 * sqrt(1 - phi^(2h)), saturating with the lead time.  The candidate k is not involved (common random numbers).
 * Value from the source value w (T): columns 1, 5, 6 (temperatures) v = (T)((double)w + e); columns 0, 2, 3, 4 t = e*(double)w,
 * v0 = (double)w + t, v = (T)(v0 < 0 ? 0 : v0).  sigma[j] = 0 gives the source value.  Columns 7 .. nd-1 are copied.
 * w_off_child[(p*K + k)*S + s] = ps*H - timestep_parent[p] (may be negative; only the clamped sum is used): the child keeps the
 * parent's timestep, hence its clock and its season end. */
typedef struct {
    int32_t struct_size;
    int32_t P, K, S, H;          /* greenhouses, candidates, scenarios (<= 256), horizon (<= 65 536); P*S*H and P*K*S <= INT32_MAX */
    int32_t weather_rows;        /* rows of `weather` (>= 1) */
    const void* weather;         /* [weather_rows][nd] T: the parents' table (nd: the handle's) */
    const int32_t* w_off_parent;      /* [P] */
    const int32_t* timestep_parent;   /* [P] */
    double sigma[7];             /* finite, >= 0: [K] for columns 1, 5, 6, relative for columns 0, 2, 3, 4 */
    double phi;                  /* 0 <= phi < 1 */
    uint64_t seed;
    uint64_t draw_index;
    const uint64_t* draw_base;   /* device word added to draw_index, or NULL */
    void* window;                /* [P*S*H][nd] T out */
    int32_t* w_off_child;        /* [P*K*S] out, or NULL */
} glgym_plan_weather_args;

int glgym_plan_weather(glgym_handle h, const glgym_plan_weather_args* a, void* stream);

/* ---- rule-based controller (BASELINE config 1 "fixed rule-based actions") ------------------------------
 * u[6] = RuleBasedController.predict(x, weather[w_off + timestep], env clocks) for every env of the shard, written in the
 * SoA layout glgym_step consumes as `control` (step_raw_control).  Constants: the constructor arguments of
 * baseline.py:22-66 in declaration order.  Computed in fp64 for either handle dtype (12 exp per env-step: free). */
typedef struct {
    double lamps_on, lamps_off, lamps_day_start, lamps_day_stop, lamps_off_sun, lamp_rad_sum_limit;
    double temp_setpoint_day, temp_setpoint_night, heat_correction, heat_deadzone, co2_day;
    double vent_heat_Pband, rh_max, mech_dehumid_Pband, vent_rh_Pband, t_vent_off, vent_cold_Pband;
    double thScrSpDay, thScrSpNight, thScrPband, thScrDeadZone, thScrRh, thScrRhPband, lampExtraHeat;
    double blScrExtraRh, rhMax, tHeatBand, co2Band, useBlScr;
} glgym_rule_cfg;

typedef struct {
    int32_t B, ld;
    const void* x;             /* SoA [28][ld] T */
    const void* weather;       /* [weather_rows][10] T; row used = w_off[b] + timestep[b] (the row about to be integrated) */
    int32_t weather_rows;
    const int32_t* w_off;      /* [B] */
    const int32_t* timestep;   /* [B] */
    const float* start_day;    /* [B] day of year at reset: day_of_year = start_day + timestep*((dt/86400) mod 365),
                                  hour_of_day = (timestep*dt/3600) mod 24   (tomato_env.py:126-128) */
    const double* hour;        /* optional [B] explicit clocks; NULL = derive as above.  The reference keeps hour_of_day as a RUNNING SUM
                                  (hour += dt/3600; hour %= 24 per step): exact for dt = 900 s, but for increments that are not multiples of
                                  1/8 h (dt = 300 s, experiments/run_time.py) the sum reads 17.999999999999996 where the product reads 18 and
                                  the rules compare the clock with whole hours -- pass the running sum here to switch the lamps on the
                                  reference's step (gl_gym_amd.TomatoVecEnv does; tests/test_gpu_holdout.py rule_based_controller_kernel) */
    const double* doy;
    void* control;             /* SoA [6][ld] T out */
} glgym_rule_args;

int glgym_rule_based(glgym_handle h, const glgym_rule_cfg* cfg, const glgym_rule_args* a, void* stream);

/* ---- closed-loop rule-based rollouts: per-row controller constants, controller tuning (csrc/gl_rule.hpp, csrc/glgym_plan.hip) ----
 * The planning section above simulates OPEN-LOOP candidates, given as action or control blocks.  Here a candidate is a FEEDBACK LAW:
 * the rule-based controller with constants of its own, evaluated on the child's present state before every env-step of the horizon.
 * This section belongs to the planning section (it stands here because it needs glgym_rule_cfg and glgym_rule_args) and keeps its
 * conventions: struct_size first, every refusal GLGYM_EINVAL with a message before anything is launched, asynchronous on `stream`,
 * no allocation, no host synchronisation (capturable), plain vector stores, no atomics.  Opt-in: no other entry point changes.
 *
 * Search space.  D of the 29 constants are tuned: component i < D is constant number field[i] of glgym_rule_cfg read as double[29]
 * in declaration order (all distinct), between lo[i] and hi[i]; the others come from `base`.  Candidate parameters are a float32
 * block theta [Ht][J][6], Ht = ceil(D / 6): component i of row j is theta[i / 6][j][i % 6]; the padding entries are ignored.  That is
 * the block glgym_plan_sample / _elites / _refit / _select draw, rank, refit and pick when they are called with H = Ht.
 * Decode, in double with products and sums rounded separately: t = fmin(fmax((double)theta_i, -1.0), 1.0); v = lo_i + (hi_i - lo_i) *
 * (0.5 * (t + 1.0)).  A NaN theta reads as -1, i.e. lo (fmax / fmin return the other operand): a NaN control never reaches a step.
 * Refused: D outside 1..29, a field index outside 0..28 or given twice, a non-finite lo or hi, lo > hi, a tuned proportional band
 * (vent_heat_Pband, vent_rh_Pband, vent_cold_Pband, thScrPband, thScrRhPband, tHeatBand, co2Band) whose interval contains 0
 * (lo <= 0 <= hi), and an untuned band that is 0 in base (as glgym_rule_based refuses it). */
typedef struct {
    glgym_rule_cfg base;
    int32_t D;                   /* 1 .. 29 */
    int32_t field[29];
    double lo[29];
    double hi[29];
} glgym_rule_space;

/* glgym_rule_based with per-row constants: row b < B takes the constants decoded from row b / max(S, 1) of theta (S = 0 or 1: its
 * own row; S >= 2: the S scenario children of a candidate share one).  Needs B <= J * max(S, 1).  One thread per row, blocks of 256;
 * rows B .. ld-1 of `control` are not written.  The rules are those of glgym_rule_based, in fp64 for either handle dtype; the
 * comparisons between lamps_on / lamps_off and lamps_day_start / lamps_day_stop are taken per row. */
typedef struct {
    int32_t struct_size;
    int32_t J;                   /* rows of theta (>= 1) */
    int32_t S;                   /* 0 .. 256 */
    glgym_rule_args rule;        /* as for glgym_rule_based: x, weather, clocks (hour / doy optional), control out */
    glgym_rule_space space;
    const float* theta;          /* [Ht][J][6] f32 */
} glgym_rule_rows_args;

/* H CLOSED-LOOP env-steps of the children.  For h = 0 .. H-1: with S >= 1 glgym_plan_scenario at step h (crop blocks only, no action
 * plane); the rows kernel above on the children's present x, timestep and w_off with rollout.step.weather / weather_rows (the row
 * about to be integrated; clocks derived from timestep and start_day), into plane (record ? h : 0) of rollout.controls; glgym_step
 * with control = that plane and metrics = NULL; glgym_plan_accumulate with the running-product weight.  rollout.actions must be NULL
 * and rollout.controls is the plane buffer, record ? H : 1 planes of SoA [6][ld] T, WRITTEN by this call (rows step.B .. ld-1 of a
 * plane are not).  S = 0: no scenarios, rollout.step.B <= J, child c reads theta row c (P, K, hold, scale, seed, draw_index, draw_base
 * are ignored).  1 <= S <= 256: rollout.step.B == P*K*S, J == P*K, rollout.step.crop_p is required and child c reads theta row
 * c / S.  H >= 1 (with S >= 1 also H <= 65 536) and gamma as for glgym_plan_rollout.  The handle's verify mode, scheme, n_sub and
 * integrator apply as they do to any raw-control step (under GLGYM_VERIFY_AUTO a raw-control step runs verified); what glgym_step
 * refuses without launching (GLGYM_ODE_PIPE with a crop block or another scheme than RK4, a BDF glgym_evalF setting on explicit
 * steps) is refused here in its words before the first launch. */
typedef struct {
    int32_t struct_size;
    int32_t record;              /* 0: one control plane, overwritten at every step; 1: H planes, plane h = the controls of step h */
    glgym_plan_rollout_args rollout;
    glgym_rule_space space;
    const float* theta;          /* [Ht][J][6] f32 */
    const float* start_day;      /* [step.B]: the children's (glgym_plan_fork writes it) */
    int32_t J;
    int32_t P, K, S;             /* as glgym_plan_rollout_scenarios_args; S = 0: no scenarios */
    int32_t hold;
    double scale;
    uint64_t seed;
    uint64_t draw_index;
    const uint64_t* draw_base;
} glgym_plan_rollout_rule_args;

int glgym_rule_rows(glgym_handle h, const glgym_rule_rows_args* a, void* stream);
int glgym_plan_rollout_rule(glgym_handle h, const glgym_plan_rollout_rule_args* a, void* stream);

/* ---- closed-loop neural-policy rollouts: per-row MLP weights, policy search (csrc/gl_mlp.hpp, csrc/glgym_plan.hip) ----
 * The feedback law of a candidate is a small MLP from the observation row glgym_obs writes to the six actions of glgym_step's action
 * path, with weights of its own.  The section keeps the planning section's conventions: struct_size first, every refusal GLGYM_EINVAL
 * with a message before anything is launched, asynchronous on `stream`, no allocation, no host synchronisation (capturable), plain
 * vector stores, no atomics.  Opt-in: no other entry point changes.
 *
 * The net.  in_dim inputs (1 .. 1024), n_hidden hidden layers (0 .. 3; 0 is a linear policy) of width[l] neurons (1 .. 64), six
 * outputs; one activation for all hidden layers, one squash on the outputs.
 * Flat parameter vector, D components: layer by layer, the layer's weight [out][in] row-major, then its bias [out] -- the order of
 * torch's parameters_to_vector on nn.Sequential(Linear, act, ..., Linear).  Candidate parameters are a float32 block theta [Ht][J][6],
 * Ht = ceil(D / 6) <= 65 535: component i of row j is theta[i / 6][j][i % 6]; the padding entries are never used.  That is the block
 * glgym_plan_sample / _elites / _refit / _select draw, rank, refit and pick when they are called with H = Ht.
 * Parameter value: w_i = scale[g] * theta_i, one float32 product; g = 2 l for the weights of layer l and 2 l + 1 for its biases
 * (2 (n_hidden + 1) groups; scale finite and > 0).  With scale 1 a trained net loads exactly; with theta sampled in [-1, 1] the scale
 * is the search bound.
 * Arithmetic: float32 throughout, products and sums rounded separately (no fused multiply-add).
 *   input       o_i = fminf(fmaxf((obs_i - mean_i) * inv_std_i, -clip_obs), clip_obs); with mean = inv_std = NULL o_i = obs_i
 *   layer       z_o = bias_o, then for i ascending z_o = z_o + w_oi * a_i
 *   activation  relu: fmaxf(z, 0), a NaN reads as 0 | tanh: tanhf(z) | silu: z / (1 + expf(-z)), expf and IEEE division
 *   output      a_j = fminf(fmaxf(s, -1), 1) with s = z_j (squash clip) or tanhf(z_j) (squash tanh); a NaN reads as -1, so that a NaN
 *               action never reaches a step
 * Refused: a size outside its range, another activation or squash, a scale that is not finite and > 0, exactly one of mean / inv_std
 * NULL, with mean / inv_std a clip_obs that is not finite and > 0 (without them clip_obs is not looked at), Ht > 65 535. */
enum { GLGYM_MLP_RELU = 0, GLGYM_MLP_TANH = 1, GLGYM_MLP_SILU = 2 };
enum { GLGYM_MLP_SQUASH_CLIP = 0, GLGYM_MLP_SQUASH_TANH = 1 };
typedef struct {
    int32_t in_dim;              /* 1 .. 1024 */
    int32_t n_hidden;            /* 0 .. 3 */
    int32_t width[3];            /* 1 .. 64 each; entries n_hidden .. 2 are ignored */
    int32_t activation;          /* GLGYM_MLP_RELU | _TANH | _SILU */
    int32_t squash;              /* GLGYM_MLP_SQUASH_CLIP | _TANH */
    float scale[8];              /* entries 2 (n_hidden + 1) .. 7 are ignored */
    float clip_obs;
    const float* mean;           /* device [in_dim] f32, or NULL with inv_std */
    const float* inv_std;        /* device [in_dim] f32: 1 / sqrt(var + epsilon) */
} glgym_mlp_net;

/* which row of theta child c reads.  CHILD: row c / max(S, 1) -- every candidate of every greenhouse has weights of its own; needs
 * B <= J * max(S, 1).  CANDIDATE: row (c / max(S, 1)) % J -- policy k is shared by all greenhouses (children ordered greenhouse,
 * candidate, scenario with J candidates per greenhouse); J = 1 runs one policy everywhere. */
enum { GLGYM_POLICY_ROW_CHILD = 0, GLGYM_POLICY_ROW_CANDIDATE = 1 };

/* The policy of B rows: action[b] = net(obs[b]; theta row of b).  One lane per row, one wavefront per block; the activations of a
 * lane pass through LDS laid out [neuron][lane] (two buffers of at most 64 x 64 floats), inputs wider than 64 in tiles of 64.  The
 * theta reads of a wavefront are 6 consecutive floats per lane with neighbouring rows adjacent; lanes that share a row read one
 * address.  Nothing outside action [B][6] is written. */
typedef struct {
    int32_t struct_size;
    int32_t B;                   /* rows (1 .. 2^31 - 64) */
    int32_t J;                   /* rows of theta (>= 1) */
    int32_t S;                   /* 0 .. 256 */
    int32_t row_mode;            /* GLGYM_POLICY_ROW_CHILD | _CANDIDATE */
    glgym_mlp_net net;
    const float* obs;            /* [B][in_dim] row-major f32: what glgym_obs writes */
    const float* theta;          /* [Ht][J][6] f32 */
    float* action;               /* [B][6] row-major f32 out, in [-1, 1] */
} glgym_policy_rows_args;

/* H CLOSED-LOOP env-steps of the children.  For h = 0 .. H-1: with S >= 1 glgym_plan_scenario at step h (crop blocks only, no action
 * plane); glgym_obs in full mode on the children's present x, u, timestep, w_off and start_day with rollout.step.weather /
 * weather_rows and Np, into `obs` [step.B][in_dim]; the policy kernel above into plane (record ? h : 0) of `actions`; glgym_step
 * with action = that plane and metrics = NULL; glgym_plan_accumulate with the running-product weight.  rollout.actions and
 * rollout.controls must be NULL; `actions` is record ? H : 1 planes of [step.B][6] f32, WRITTEN by this call.  The handle's
 * observation modules apply: net.in_dim must equal glgym_obs_dim(h, Np).  S = 0: no scenarios (P, K, hold, scale, seed, draw_index,
 * draw_base are ignored); CHILD mode needs step.B <= J.  1 <= S <= 256: step.B == P*K*S, rollout.step.crop_p is required, J == P*K
 * in CHILD mode and J == K in CANDIDATE mode.  H >= 1 (with S >= 1 also H <= 65 536) and gamma as for glgym_plan_rollout.  The
 * handle's verify mode, scheme, n_sub and integrator apply as to any action step; what glgym_step refuses without launching is
 * refused here in its words before the first launch. */
typedef struct {
    int32_t struct_size;
    int32_t record;              /* 0: one action plane, overwritten at every step; 1: H planes, plane h = the actions of step h */
    glgym_plan_rollout_args rollout;
    glgym_mlp_net net;
    const float* theta;          /* [Ht][J][6] f32 */
    const float* start_day;      /* [step.B]: the children's (glgym_plan_fork writes it) */
    float* obs;                  /* [step.B][in_dim] f32 workspace: the observations of the last step afterwards */
    float* actions;              /* [record ? H : 1][step.B][6] f32 out */
    int32_t Np;                  /* forecast rows of the observation (glgym_obs_args.Np) */
    int32_t row_mode;
    int32_t J;
    int32_t P, K, S;             /* as glgym_plan_rollout_scenarios_args; S = 0: no scenarios */
    int32_t hold;
    double scale;
    uint64_t seed;
    uint64_t draw_index;
    const uint64_t* draw_base;
} glgym_plan_rollout_policy_args;

int glgym_policy_rows(glgym_handle h, const glgym_policy_rows_args* a, void* stream);
int glgym_plan_rollout_policy(glgym_handle h, const glgym_plan_rollout_policy_args* a, void* stream);

/* ---- rollout collection: Gaussian sampling stage and GAE (csrc/gl_actor.hpp, csrc/glgym_collect.hip) ----
 * What an on-policy learner does between two env-steps once its heads have been evaluated -- noise, sample, clip, log-probability,
 * buffer writes -- and after the last one, the generalised advantage estimate, as two entry points.  The planning section's
 * conventions hold: struct_size first, every refusal GLGYM_EINVAL with a message of its own before the handle is looked at and before
 * anything is launched, asynchronous on `stream`, no allocation, no host synchronisation (capturable), plain vector stores, no
 * atomics.  Opt-in: no other entry point changes.
 *
 * Heads.  The six raw means mean_in [B][6] and the value value_in [B] are the caller's: what torch modules of any size produced.
 * (Heads evaluated inside this call are not part of the library yet.)
 * Noise.  D = draw_index + *draw_base (draw_base NULL: 0).  Row b at step `step`: Philox4x32-10 with counter (b, 2 step + blk, lo32(D),
 * hi32(D)), blk = 0 | 1, key (lo32(seed), hi32(seed) ^ 0x41435431); with the eight words r0..r7, u = (r + 0.5) * 2^-32 and three
 * Box-Muller pairs in double from r0..r5 as glgym_plan_sample's: sqrt(-2 log u0) * cos(2 pi u1), ... * sin(2 pi u1); e_j = (float) of
 * them.  Row b's noise does not depend on B.  deterministic = 1: e_j = 0, no draw.
 * Sample, float32, every operation rounded on its own:
 *   a_j    = mean_j + std_j * e_j                                            -> action
 *   env_j  = fminf(fmaxf(a_j, -1), 1), a NaN reads as -1                     -> action_env, what glgym_step's action path takes
 *   logp   = s after s = 0 and, j ascending, s = s + (((-0.5f * e_j) * e_j - log_std_j) - 0.9189385f)
 * log_std [6] and std [6] are both the caller's device vectors (std = exp(log_std)): the kernel has no transcendental but the normals'.
 * value = value_in, copied into the buffer slot; obs_out, if given, is a copy of obs [B][in_dim] (the slot of the observation).
 * value_only = 1: only `value` is written (the bootstrap value after the last step); nothing else is looked at but value_in.
 * Kernel: one lane per row, 256 per block, no LDS, no barrier; the observation copy is a block's own 256 rows, one contiguous span.
 * Nothing outside the named outputs is written.
 * Refused: B < 1 or > 2^31 - 256, step < 0, a flag that is not 0 | 1, a NULL value_in or value; without value_only a NULL mean_in,
 * log_std, std, action, action_env or logp, and with obs_out an in_dim outside 1 .. 1024, a NULL obs, obs_out == obs or overlapping it. */
typedef struct {
    int32_t struct_size;
    int32_t B;                   /* rows */
    int32_t in_dim;              /* columns of obs / obs_out; looked at only with obs_out */
    int32_t step;                /* >= 0: the step of the rollout, second word of the counter */
    int32_t deterministic;       /* 0 | 1 */
    int32_t value_only;          /* 0 | 1 */
    const float* mean_in;        /* [B][6] f32 */
    const float* value_in;       /* [B] f32 */
    const float* log_std;        /* [6] f32 */
    const float* std;            /* [6] f32: exp(log_std) */
    uint64_t seed;
    uint64_t draw_index;
    const uint64_t* draw_base;   /* device word added to draw_index, or NULL */
    const float* obs;            /* [B][in_dim] f32, or NULL without obs_out */
    float* obs_out;              /* [B][in_dim] f32 out, or NULL */
    float* action;               /* [B][6] f32 out: a */
    float* action_env;           /* [B][6] f32 out: a clipped to [-1, 1] */
    float* eps;                  /* [B][6] f32 out: e, or NULL */
    float* logp;                 /* [B] f32 out */
    float* value;                /* [B] f32 out */
} glgym_ac_rows_args;

/* GAE(lambda) over a rollout of T steps of B environments, float32, gamma and lambda cast to float once and gl = gamma * lambda one
 * float32 product; per environment, adv = 0, then for t = T-1 .. 0:
 *   nnt    = 1 - (done[t] != 0);  nv = t == T-1 ? last_value : value[t+1]
 *   delta  = (reward[t] + (gamma * nv) * nnt) - value[t]
 *   adv    = delta + (gl * nnt) * adv                      -> advantage[t]
 *   returns[t] = adv + value[t]
 * every product and sum rounded on its own, left to right inside the brackets -- stable_baselines3's compute_returns_and_advantage with
 * episode_starts[t+1] == done[t].  One lane per environment, 256 per block, every access coalesced along b.
 * Refused: T < 1, B < 1, gamma or lambda outside [0, 1] or not finite, a NULL pointer, an output that overlaps an input or the other
 * output. */
typedef struct {
    int32_t struct_size;
    int32_t T;
    int32_t B;
    const float* reward;         /* [T][B] f32 */
    const uint8_t* done;         /* [T][B] */
    const float* value;          /* [T][B] f32 */
    const float* last_value;     /* [B] f32: the value of the observation after step T-1 */
    double gamma;
    double lambda;
    float* advantage;            /* [T][B] f32 out */
    float* returns;              /* [T][B] f32 out */
} glgym_gae_args;

int glgym_ac_rows(glgym_handle h, const glgym_ac_rows_args* a, void* stream);
int glgym_gae(glgym_handle h, const glgym_gae_args* a, void* stream);

/* ---- PPO update: seeded minibatches and the clipped-surrogate loss (csrc/gl_ppo.hpp, csrc/glgym_ppo.hip) ----
 * The other half of the on-policy loop: what stable_baselines3's PPO.train does around the two heads -- the shuffle, the minibatch
 * gathers, the advantage normalisation, the loss with its gradients with respect to the heads' outputs -- as two entry points.  The heads
 * themselves, their backward pass and the optimiser stay the caller's, in torch.  The planning section's conventions hold: struct_size
 * first, every refusal GLGYM_EINVAL with a message of its own before the handle is looked at and before anything is launched,
 * asynchronous on `stream`, no allocation, no host synchronisation (capturable), plain vector stores, no atomics.  Opt-in: no other
 * entry point changes.
 *
 * Permutation.  D = draw_index + *draw_base (draw_base NULL: 0).  Position p in [0, N) -> transition perm(p) in [0, N), computed per
 * index, never stored: w = the smallest even bit count >= 2 with 2^w >= N, half = w / 2, mask = 2^half - 1.  P(x) on [0, 2^w): L = x >> half,
 * R = x & mask; four rounds r = 0..3 of (L, R) = (R, L ^ (F(r, R) & mask)); P = (L << half) | R, where F(r, R) is word 0 of Philox4x32-10
 * with counter (R, r, lo32(D), hi32(D)) and key (lo32(seed), hi32(seed) ^ 0x50524d31).  perm(p): y = P(p); while y >= N: y = P(y).  It
 * depends on (seed, D, N) only -- not on M, offset or the launch.
 * Reductions (both entry points).  Rows are cut into chunks of 256; nb = min(ceil(M / 256), 1024) blocks of 256 lanes; block b takes
 * chunks b, b + nb, ...; lane t takes row 256 chunk + t of each, ascending, and adds its terms in double from 0.  The 64 lanes of a
 * wavefront combine by butterfly (xor 32, 16, .. 1), the four wavefronts of a block in index order, the blocks' partials go to
 * `workspace` and a finishing launch of the same call adds them in block order.  A function of M alone.
 *
 * glgym_ppo_batch: minibatch positions [offset, offset + M) of the permutation, gathered from flat [N] sources (a collector's buffer
 * viewed as [T*B]).  Row m of every output is row perm(offset + m) of its source, bit for bit; mb_index, if given, is perm(offset + m).
 * A block's output rows are one contiguous span written with lane stride 1; a row's permutation is computed once and shared.
 * adv_stats, if given: [0] = S1 / M and [1] = sqrt(max(0, (S2 - (S1 * S1) / M) / (M - 1))) of the minibatch's advantages, S1 = sum a,
 * S2 = sum a * a in double by the reduction above, every operation rounded on its own.  workspace: [1024][2] doubles = 16 384 bytes,
 * needed with adv_stats only.
 * Refused: N or M < 1, N > 2^31 - 256, offset < 0 or offset + M > N, in_dim outside 1 .. 1024, a NULL source or output other than
 * mb_index / adv_stats, adv_stats with M < 2 or with a NULL or undersized workspace, an output that overlaps a source or another output. */
typedef struct {
    int32_t struct_size;
    int32_t N;                   /* transitions in the sources */
    int32_t M;                   /* rows of this minibatch */
    int32_t offset;              /* first position of the permutation */
    int32_t in_dim;              /* columns of obs */
    uint64_t seed;
    uint64_t draw_index;
    const uint64_t* draw_base;   /* device word added to draw_index, or NULL */
    const float* obs;            /* [N][in_dim] f32 */
    const float* action;         /* [N][6] f32 */
    const float* logp;           /* [N] f32 */
    const float* advantage;      /* [N] f32 */
    const float* returns;        /* [N] f32 */
    const float* value;          /* [N] f32 */
    float* mb_obs;               /* [M][in_dim] f32 out */
    float* mb_action;            /* [M][6] f32 out */
    float* mb_logp;              /* [M] f32 out */
    float* mb_adv;               /* [M] f32 out */
    float* mb_ret;               /* [M] f32 out */
    float* mb_value;             /* [M] f32 out */
    int32_t* mb_index;           /* [M] i32 out, or NULL */
    double* adv_stats;           /* [2] out: mean, unbiased standard deviation of mb_adv, or NULL */
    double* workspace;           /* [1024][2] doubles, or NULL without adv_stats */
    int64_t workspace_bytes;
} glgym_ppo_batch_args;

/* glgym_ppo_loss: the clipped-surrogate loss of stable_baselines3's PPO.train on the heads' outputs of one minibatch, forward and
 * backward in one call.  float32, every operation rounded on its own, in this order (c = clip_range, cv = clip_range_vf,
 * w = (float)(1.0 / M), the coefficients cast to float once); per row:
 *   z_j    = (a_j - mean_j) * inv_std_j                          inv_std = exp(-log_std) is the caller's, as std is glgym_ac_rows'
 *   logp   = s after s = 0 and, j ascending, s = s + (((-0.5f * z_j) * z_j - log_std_j) - 0.9189385f)          -> logp_out
 *   d      = logp - old_logp;  ratio = (float) exp((double) d)                                                   -> ratio_out
 *   A      = adv, or with adv_stats (adv - (float) adv_stats[0]) / ((float) adv_stats[1] + 1e-8f)
 *   s1     = ratio * A;  rc = fminf(fmaxf(ratio, 1 - c), 1 + c);  s2 = rc * A;  surrogate = fminf(s1, s2)
 *   q      = s1 <= s2 ? (-w) * s1 : 0          (what the backward passes of min and clamp add up to, the tie inside the clip range included)
 *   grad_mean_j = q * (z_j * inv_std_j);  the row's term for log_std_j = q * (z_j * z_j - 1)
 *   vp     = value, or with cv > 0 old_v + fminf(fmaxf(value - old_v, -cv), cv);  value term = (ret - vp) * (ret - vp)
 *   grad_value  = ((vf_coef * 2) * w) * (vp - ret), or 0 where value - old_v lies outside [-cv, cv]
 *   kl term = (ratio - 1) - d;  clip term = |ratio - 1| > c
 * The rows' terms are added in double by the reduction above (the largest ratio with max in place of +, a NaN winning), then
 *   policy_loss = -(sum surrogate / M);  value_loss = sum value term / M
 *   entropy_loss = -e after e = 0 and, j ascending, e = e + ((0.5f + 0.9189385f) + log_std_j)      (float32)
 *   stats = { (policy_loss + ent_coef * entropy_loss) + vf_coef * value_loss, policy_loss, value_loss, entropy_loss, sum kl / M,
 *             sum clip / M, max ratio, M }                                                          (double)
 *   grad_log_std_j = (float)(sum of the rows' terms) - ent_coef                                     (float32)
 * A NaN stays in its row: its gradients, logp, ratio and kl are NaN and so are the sums they enter; fminf / fmaxf hand on their other
 * operand, so the surrogate of a row whose ratio is NaN reads (1 - c) * A.  Nothing traps; nothing outside the named outputs is written.
 * Kernel: one lane per row, 256 per block, LDS for combining the wavefronts only.  workspace: [1024][11] doubles = 90 112 bytes.
 * Refused: M < 1 or > 2^31 - 256, clip_range not > 0 or not finite, a coefficient or clip_range_vf that is not finite, clip_range_vf > 0
 * without mb_value, a NULL pointer other than adv_stats / mb_value / ratio_out / logp_out, an undersized workspace, an output that
 * overlaps an input or another output. */
typedef struct {
    int32_t struct_size;
    int32_t M;
    const float* mean;           /* [M][6] f32: the policy head's output */
    const float* value;          /* [M] f32: the value head's output */
    const float* log_std;        /* [6] f32 */
    const float* inv_std;        /* [6] f32: exp(-log_std) */
    const float* mb_action;      /* [M][6] f32 */
    const float* mb_logp;        /* [M] f32: old_logp */
    const float* mb_adv;         /* [M] f32 */
    const float* mb_ret;         /* [M] f32 */
    const float* mb_value;       /* [M] f32: old_v, or NULL with clip_range_vf <= 0 */
    const double* adv_stats;     /* [2]: glgym_ppo_batch's, or NULL: no normalisation */
    double clip_range;           /* > 0 */
    double clip_range_vf;        /* <= 0: off */
    double vf_coef;
    double ent_coef;
    float* grad_mean;            /* [M][6] f32 out */
    float* grad_value;           /* [M] f32 out */
    float* grad_log_std;         /* [6] f32 out */
    double* stats;               /* [8] out */
    float* ratio_out;            /* [M] f32 out, or NULL */
    float* logp_out;             /* [M] f32 out, or NULL */
    double* workspace;           /* [1024][11] doubles */
    int64_t workspace_bytes;
} glgym_ppo_loss_args;

int glgym_ppo_batch(glgym_handle h, const glgym_ppo_batch_args* a, void* stream);
int glgym_ppo_loss(glgym_handle h, const glgym_ppo_loss_args* a, void* stream);

/* ---- soft actor-critic: replay ring, squashed actor, loss stage, Polyak update (csrc/gl_sac.hpp, csrc/glgym_sac.hip) ----
 * The off-policy twin of the two sections above: what stable_baselines3's SAC does between the networks' outputs and their gradients, as
 * five entry points.  The actor, the two critics, the two target critics, autograd through them and the optimisers stay the caller's, in
 * torch.  The planning section's conventions hold: struct_size first, every refusal GLGYM_EINVAL with a message of its own before the
 * handle is looked at and before anything is launched, asynchronous on `stream`, no allocation, no host synchronisation (capturable),
 * plain vector stores, no atomics.  Opt-in: no other entry point changes.  Reductions are those of the PPO section: chunks of 256 rows,
 * nb = min(ceil(M / 256), 1024) blocks, lane / butterfly / wavefronts in index order / blocks in block order, in double, through
 * `workspace` and a finishing launch -- a function of M alone.
 *
 * glgym_sac_rows: the tanh-squashed Gaussian with a state-dependent deviation, forward.  mean_in [M][6] and log_std_in [M][6] are the
 * actor's two outputs.
 * Noise.  D = draw_index + *draw_base (draw_base NULL: 0).  Row r has the key k = (uint32)(row0 + r): Philox4x32-10 with counter
 * (k, 4 step + blk, lo32(D), hi32(D)), key (lo32(seed), hi32(seed) ^ 0x53414331 "SAC1").  blk = 0 | 1 give eight words and e_0..e_5 by
 * three Box-Muller pairs in double from words 0..5, each rounded once to float32, as glgym_ac_rows; blk = 2 | 3 give e2_0..e2_5 the same
 * way.  A row's noise depends on neither M nor any other row.
 * Per actuator j, float32, every operation rounded on its own, in this order:
 *   ls   = fminf(fmaxf(log_std_j, -20), 2)
 *   std  = (float) exp((double) ls)                                                     -> std
 *   u    = mean_j + std * e_j                                                           (e -> eps, e2 -> eps2)
 *   a    = (float) tanh((double) u)                                                     -> action, tanh
 *   c    = (1 - a * a) + 1e-6f
 *   l    = (float) log((double) c)                                                      -> corr
 *   logp = s after s = 0; j ascending: s = s + (((-0.5f * e_j) * e_j - ls_j) - 0.9189385f); then j ascending: s = s - l_j     -> logp
 *   env  = fminf(fmaxf(a, -1), 1); with action_noise_sigma > 0: fminf(fmaxf(a + sigma * e2_j, -1), 1)      -> action_env, action_slot
 * A NaN reads as -1 in env, whatever its source.  deterministic = 1: e_j = 0 (e2 is still drawn with sigma > 0).  uniform = 1 (the
 * learning_starts warm-up): a_j = (float)(2.0 * (((double) r_j + 0.5) * 2^-32) - 1.0) from words r_0..r_5 of blk 0 | 1, env_j its clip;
 * mean_in and log_std_in are not looked at and only action, action_env, action_slot and obs_out are written.
 * Every output is optional; at least one must be given.  eps2 and corr are diagnostic outputs: they exist so that a test can hand the
 * device's own noise and log term to a host build, nothing in the library reads them and callers should not depend on them.  obs_out is a copy of obs [M][in_dim].  Kernel: one lane per row, 256 per block,
 * no LDS, no barrier.  Nothing outside the named outputs is written.
 * Refused: M < 1 or > 2^31 - 256, step outside 0 .. 2^30 - 1, row0 < 0 or row0 + M > 2^32, a flag that is not 0 | 1, both flags set,
 * action_noise_sigma negative or not finite, no output at all, without uniform a NULL mean_in or log_std_in, with uniform a logp, eps,
 * eps2, std, tanh or corr output, with obs_out an in_dim outside 1 .. 1024, a NULL obs, obs_out overlapping obs. */
typedef struct {
    int32_t struct_size;
    int32_t M;                   /* rows */
    int32_t in_dim;              /* columns of obs / obs_out; looked at only with obs_out */
    int32_t step;                /* 0 .. 2^30 - 1: second word of the counter is 4 step + blk */
    int32_t deterministic;       /* 0 | 1 */
    int32_t uniform;             /* 0 | 1 */
    int64_t row0;                /* the noise of row r is keyed by row0 + r */
    const float* mean_in;        /* [M][6] f32 */
    const float* log_std_in;     /* [M][6] f32 */
    uint64_t seed;
    uint64_t draw_index;
    const uint64_t* draw_base;   /* device word added to draw_index, or NULL */
    double action_noise_sigma;   /* 0: off */
    const float* obs;            /* [M][in_dim] f32, or NULL without obs_out */
    float* obs_out;              /* [M][in_dim] f32 out, or NULL */
    float* action;               /* [M][6] f32 out: a, or NULL */
    float* action_env;           /* [M][6] f32 out: env, or NULL */
    float* action_slot;          /* [M][6] f32 out: env once more (a replay slot), or NULL */
    float* logp;                 /* [M] f32 out, or NULL */
    float* eps;                  /* [M][6] f32 out: e, or NULL */
    float* eps2;                 /* [M][6] f32 out, DIAGNOSTIC (tests; may change): e2 (0 without action_noise_sigma > 0), or NULL */
    float* std;                  /* [M][6] f32 out, or NULL */
    float* tanh;                 /* [M][6] f32 out: a, or NULL */
    float* corr;                 /* [M][6] f32 out, DIAGNOSTIC (tests; may change): l, or NULL */
} glgym_sac_rows_args;

/* glgym_sac_rows_grad: the reparameterised backward pass of glgym_sac_rows from what it saved.  Per element, float32, every operation
 * rounded on its own, in this order (ga = grad_action_j, gl = grad_logp of the row, a = tanh_j, e = eps_j):
 *   g  = 1 - a * a
 *   gu = (ga * g) + (gl * (((2 * a) * g) / (g + 1e-6f)))                               -> grad_mean
 *   grad_log_std = ((gu * (std * e)) - gl) where -20 <= log_std_in_j <= 2, else 0 (a NaN log_std_in: 0)
 * One lane per row.  Refused: M < 1 or > 2^31 - 256, a NULL pointer, an output that overlaps an input or the other output. */
typedef struct {
    int32_t struct_size;
    int32_t M;
    const float* grad_action;    /* [M][6] f32 */
    const float* grad_logp;      /* [M] f32 */
    const float* eps;            /* [M][6] f32 */
    const float* std;            /* [M][6] f32 */
    const float* tanh;           /* [M][6] f32 */
    const float* log_std_in;     /* [M][6] f32 */
    float* grad_mean;            /* [M][6] f32 out */
    float* grad_log_std;         /* [M][6] f32 out */
} glgym_sac_rows_grad_args;

/* glgym_sac_batch: M transitions drawn with replacement from a replay ring of S slots of B environments, slot-major: obs [S][B][in_dim],
 * action [S][B][6], reward [S][B], done [S][B] (uint8).  An observation is stored once: the next observation of slot s is the observation
 * of slot (s + 1) mod S.  head is the oldest valid slot and n_valid the number of slots, counted from head, whose successor observation
 * has been written (1 <= n_valid <= S - 1).
 * Position p in [0, M) of draw D = draw_index + *draw_base: Philox4x32-10 with counter (p, 0, lo32(D), hi32(D)) and key (lo32(seed),
 * hi32(seed) ^ 0x534d5031 "SMP1"); w = word0 * 2^32 + word1; idx = floor(w * n / 2^64) with n = n_valid * B (its bias is at most
 * n / 2^64); slot = (head + idx / B) mod S, b = idx mod B.  Row p of mb_obs, mb_action, mb_reward, mb_done is row (slot, b) of its source,
 * row p of mb_next_obs is row ((slot + 1) mod S, b) of obs, bit for bit; index_out, if given, is slot * B + b.  It depends on (seed, D, S,
 * B, head, n_valid) and p only.  A block's output rows are one contiguous span written with lane stride 1; the row indices are staged in LDS.
 * Refused: S < 2, B < 1, S * B > 2^31 - 1, M < 1 or > 2^31 - 256, in_dim outside 1 .. 1024, head outside 0 .. S - 1, n_valid < 1,
 * n_valid > S - 1 (a slot without a successor), a NULL pointer other than index_out / draw_base, an output that overlaps a source or
 * another output. */
typedef struct {
    int32_t struct_size;
    int32_t S;                   /* slots of the ring */
    int32_t B;                   /* environments per slot */
    int32_t in_dim;              /* columns of obs */
    int32_t M;                   /* rows of the minibatch */
    int32_t head;                /* oldest valid slot */
    int32_t n_valid;             /* slots with a written successor observation */
    int32_t reserved;            /* 0 */
    uint64_t seed;
    uint64_t draw_index;
    const uint64_t* draw_base;   /* device word added to draw_index, or NULL */
    const float* obs;            /* [S][B][in_dim] f32 */
    const float* action;         /* [S][B][6] f32 */
    const float* reward;         /* [S][B] f32 */
    const uint8_t* done;         /* [S][B] */
    float* mb_obs;               /* [M][in_dim] f32 out */
    float* mb_next_obs;          /* [M][in_dim] f32 out */
    float* mb_action;            /* [M][6] f32 out */
    float* mb_reward;            /* [M] f32 out */
    uint8_t* mb_done;            /* [M] out */
    int64_t* index_out;          /* [M] i64 out, or NULL */
} glgym_sac_batch_args;

/* glgym_sac_loss: the critic stage (stage = 0) or the actor stage (stage = 1) of stable_baselines3's SAC.train, forward and backward in
 * one call.  alpha [1] is a device float the caller forms as exp(log_alpha) (as std is the caller's in glgym_ac_rows); w = (float)(1.0 / M);
 * gamma and target_entropy are cast to float once.  float32, every operation rounded on its own, in this order; per row:
 * Critic stage (q1, q2: the critics on (obs, action); q1_next, q2_next: the target critics on (next_obs, next action); logp: the next
 * action's log-probability):
 *   m  = fminf(q1_next, q2_next)
 *   y  = reward + (((1 - done) * gamma) * (m - (alpha * logp)))                        -> target_out      (done != 0 reads as 1)
 *   grad_q1 = w * (q1 - y);  grad_q2 = w * (q2 - y)
 *   sums in double of (q1 - y) * (q1 - y), (q2 - y) * (q2 - y), q1, q2, y  =: S1, S2, Q1, Q2, Y
 *   stats = { (0.5 * (S1 + S2)) / M, S1 / M, S2 / M, Q1 / M, Q2 / M, Y / M, alpha, M }
 * Actor stage (q1, q2: the critics on (obs, the policy's action); logp: that action's log-probability):
 *   grad_logp = w * alpha;  grad_q1 = q1 <= q2 ? -w : 0;  grad_q2 = q1 <= q2 ? 0 : -w
 *   sums in double of (alpha * logp) - fminf(q1, q2), logp + target_entropy, logp  =: A, E, P
 *   stats = { A / M, -(log_alpha * (E / M)), -(E / M), P / M, alpha, log_alpha, 0, M };  grad_log_alpha = (float)(-(E / M))
 * stats[1] is the entropy coefficient's loss -(log_alpha) * mean(logp + target_entropy) and stats[2] its gradient.
 * NaN: fminf hands on its other operand, so a NaN q1_next alone leaves the target finite; a NaN in both, in logp, reward or alpha gives a NaN
 * y, NaN gradients of that row and NaN sums they enter.  In the actor stage a NaN q1 fails q1 <= q2: the row's gradient goes to q2, and
 * the loss term is alpha logp - q2.  Nothing traps; nothing outside the named outputs is written.
 * Kernel: one lane per row, 256 per block, LDS for combining the wavefronts only.  workspace: [1024][5] doubles = 40 960 bytes.
 * Refused: M < 1 or > 2^31 - 256, a stage other than 0 | 1, gamma outside [0, 1] or target_entropy not finite, a NULL q1, q2, logp,
 * alpha, grad_q1, grad_q2, stats or workspace, in the critic stage a NULL q1_next, q2_next, reward or done, in the actor stage a NULL
 * log_alpha or grad_logp, an undersized workspace, an output that overlaps an input or another output. */
typedef struct {
    int32_t struct_size;
    int32_t M;
    int32_t stage;               /* 0: critic, 1: actor */
    int32_t reserved;            /* 0 */
    const float* q1;             /* [M] f32 */
    const float* q2;             /* [M] f32 */
    const float* logp;           /* [M] f32 */
    const float* q1_next;        /* [M] f32, critic stage */
    const float* q2_next;        /* [M] f32, critic stage */
    const float* reward;         /* [M] f32, critic stage */
    const uint8_t* done;         /* [M], critic stage */
    const float* alpha;          /* [1] f32 device: exp(log_alpha) */
    const float* log_alpha;      /* [1] f32 device, actor stage */
    double gamma;                /* critic stage */
    double target_entropy;       /* actor stage */
    float* grad_q1;              /* [M] f32 out */
    float* grad_q2;              /* [M] f32 out */
    float* grad_logp;            /* [M] f32 out, actor stage */
    float* target_out;           /* [M] f32 out, critic stage, or NULL */
    float* grad_log_alpha;       /* [1] f32 out, actor stage, or NULL */
    double* stats;               /* [8] out */
    double* workspace;           /* [1024][5] doubles */
    int64_t workspace_bytes;
} glgym_sac_loss_args;

/* glgym_polyak: t = ((1 - tau) * t) + (tau * s) over a table of n <= 64 tensors in one launch, float32, 1 - tau one float32 difference of
 * (float) tau formed once, the two products rounded separately.  dst [n], src [n] (device arrays of device pointers) and count [n] (device
 * int64 element counts) are uploaded once by the caller; max_count, the largest count, only sizes the grid (the kernel strides over it:
 * a smaller value is slower, never wrong).  Every element is a dword access, so a tensor needs 4-byte alignment only; a tensor of 0
 * elements is skipped.  Refused: n outside 1 .. 64, a NULL table, tau outside [0, 1] or not finite, max_count < 0. */
typedef struct {
    int32_t struct_size;
    int32_t n;
    float* const* dst;           /* [n] device: the target tensors t */
    const float* const* src;     /* [n] device: the source tensors s */
    const int64_t* count;        /* [n] device: elements of each */
    int64_t max_count;
    double tau;
} glgym_polyak_args;

int glgym_sac_rows(glgym_handle h, const glgym_sac_rows_args* a, void* stream);
int glgym_sac_rows_grad(glgym_handle h, const glgym_sac_rows_grad_args* a, void* stream);
int glgym_sac_batch(glgym_handle h, const glgym_sac_batch_args* a, void* stream);
int glgym_sac_loss(glgym_handle h, const glgym_sac_loss_args* a, void* stream);
int glgym_polyak(glgym_handle h, const glgym_polyak_args* a, void* stream);

/* ---- recurrent PPO: fused LSTM cell and sequence minibatches (csrc/gl_lstm.hpp, csrc/glgym_rppo.hip) ----
 * What a recurrent policy (sb3-contrib's RecurrentPPO with MlpLstmPolicy) adds to the two on-policy sections above: the part of an LSTM
 * step that lies between torch's two gate products and the new state, its backward pass, and minibatches of whole sequences for truncated
 * back-propagation through time.  The products x W_ih^T + b and h W_hh^T, autograd through them, the heads and the optimiser stay the
 * caller's, in torch.  The planning section's conventions hold: struct_size first, every refusal GLGYM_EINVAL with a message of its own
 * before the handle is looked at and before anything is launched, asynchronous on `stream`, no allocation, no host synchronisation
 * (capturable), plain vector stores, no atomics, an output that overlaps an input or another output is refused.  Opt-in: no other entry
 * point changes.
 *
 * glgym_lstm_cell: one LSTM step on the gate pre-activations of M rows with hidden size H, gates in torch's order i, f, g, o:
 * gx [M][4H] is the input product with whatever bias the caller's addmm folded in (b_ih + b_hh), gh [M][4H] is h_prev W_hh^T without a
 * bias.  float32, every operation rounded on its own, in this order, per (row, unit j) (x_k = x[row][k H + j]):
 *   keep = start == NULL || start[row] == 0
 *   a_k  = keep ? gx_k + gh_k : gx_k                 k = i, f, g, o
 *   c0   = keep ? c_prev : 0
 *   i = (float)(1 / (1 + exp(-(double) a_i))), likewise f and o;  g = (float) tanh((double) a_g)
 *   c = f * c0 + i * g          (two products and one sum, not contracted)
 *   tc = (float) tanh((double) c);  h = o * tc
 * act, if given, is [M][5H] holding i, f, g, o, tc: what glgym_lstm_cell_grad reads (NULL while collecting).
 * The reset is a SELECT, not sb3-contrib's multiplication of the state by 1 - episode_start.  For finite states the two give the same
 * numbers; with the select a NaN or an infinity in the state of an episode that has ended cannot enter the next one (0 * NaN is NaN).
 * The mask commutes with the product -- (m h) W = m (h W) for a row scalar m in {0, 1} -- so gh may be computed from the unmasked h_prev
 * and no masking launch is needed in front of it.
 * Kernel: one lane per (row, unit), consecutive lanes on consecutive units of each gate plane; where H % 4 == 0 and every buffer is
 * 16-byte aligned a lane takes four units with one 16-byte access per plane.  No LDS, no barrier, no scratch; at most 2048 blocks of 256,
 * striding.  44 bytes per (row, unit) without act, 64 with it.
 * Refused: M < 1, H outside 1 .. 1024, M * 4 H above 2^31 - 1, a NULL pointer other than start / act, an overlap. */
typedef struct {
    int32_t struct_size;
    int32_t M;                   /* rows */
    int32_t H;                   /* hidden size */
    const float* gx;             /* [M][4H] f32: x W_ih^T + b_ih + b_hh */
    const float* gh;             /* [M][4H] f32: h_prev W_hh^T */
    const float* c_prev;         /* [M][H] f32 */
    const uint8_t* start;        /* [M]: non-zero = the row begins an episode, or NULL: none does */
    float* h;                    /* [M][H] f32 out */
    float* c;                    /* [M][H] f32 out */
    float* act;                  /* [M][5H] f32 out: i, f, g, o, tc, or NULL */
} glgym_lstm_cell_args;

/* glgym_lstm_cell_grad: the backward pass of glgym_lstm_cell from what it saved.  dh [M][H] is the gradient arriving at h, dc [M][H] the
 * one arriving at c from the step after (NULL: 0).  float32, every operation rounded on its own, in this order, per (row, unit), with keep
 * and c0 as above:
 *   do   = dh * tc
 *   dct  = dc + (dh * o) * (1 - tc * tc)
 *   da_i = (dct * g) * (i * (1 - i));  da_f = (dct * c0) * (f * (1 - f));  da_g = (dct * i) * (1 - g * g);  da_o = do * (o * (1 - o))
 *   d_gx = da;  d_gh = keep ? da : 0;  d_c_prev = keep ? dct * f : 0
 * No transcendental, no reduction (the bias gradients are the addmm's own).  The kernel is shaped as glgym_lstm_cell's.
 * Refused: as glgym_lstm_cell, the optional pointers being start and dc. */
typedef struct {
    int32_t struct_size;
    int32_t M;
    int32_t H;
    const float* dh;             /* [M][H] f32 */
    const float* dc;             /* [M][H] f32, or NULL: 0 */
    const float* act;            /* [M][5H] f32: glgym_lstm_cell's */
    const float* c_prev;         /* [M][H] f32 */
    const uint8_t* start;        /* [M], or NULL */
    float* d_gx;                 /* [M][4H] f32 out */
    float* d_gh;                 /* [M][4H] f32 out */
    float* d_c_prev;             /* [M][H] f32 out */
} glgym_lstm_cell_grad_args;

/* glgym_seq_batch: a minibatch of S whole sequences of L steps from a collector's [T][B] buffer, T % L == 0.  Sequence q in
 * [0, (T / L) B) is chunk q / B of environment q % B, i.e. buffer rows ((q / B) L + l) B + q % B for l = 0 .. L - 1.  The minibatch is
 * positions [offset, offset + S) of glgym_ppo_batch's permutation with N = (T / L) B (the same function, key tag and draw word): with L = 1
 * the call gathers what glgym_ppo_batch gathers.  The outputs are time-major: row (l, s) = l S + s of each is the source row of step l of
 * sequence perm(offset + s), bit for bit; mb_start is gathered from episode_starts (uint8); mb_index [S], if given, is perm(offset + s).
 * For i < n_state <= 4, state_src[i] is [T / L][B][state_dim[i]] (a recurrent state stored at the first step of every chunk) and
 * state_out[i] [S][state_dim[i]] its row perm(offset + s).
 * No padding: a sequence is not split where an episode starts inside it, glgym_lstm_cell's start select does there what a per-step loop
 * over the episode starts does.
 * adv_stats, if given: mean and unbiased standard deviation of the L S gathered advantages in flattened (l, s) order, by the reduction
 * and the formula stated for glgym_ppo_batch with M = L S.  workspace: [1024][2] doubles = 16 384 bytes, needed with adv_stats only.
 * Refused: T, B, S or L < 1, T % L != 0, T B > 2^31 - 256, offset < 0 or offset + S > (T / L) B, in_dim outside 1 .. 1024, n_state outside
 * 0 .. 4, a state dimension outside 1 .. 1024, a NULL source or output other than mb_index / adv_stats, adv_stats with L S < 2 or with a
 * NULL or undersized workspace, an output that overlaps a source or another output. */
typedef struct {
    int32_t struct_size;
    int32_t T;                   /* steps of the buffer */
    int32_t B;                   /* environments */
    int32_t L;                   /* steps of a sequence */
    int32_t S;                   /* sequences of this minibatch */
    int32_t offset;              /* first position of the permutation */
    int32_t in_dim;              /* columns of obs */
    int32_t n_state;             /* 0 .. 4 */
    int32_t state_dim[4];
    uint64_t seed;
    uint64_t draw_index;
    const uint64_t* draw_base;   /* device word added to draw_index, or NULL */
    const float* obs;            /* [T][B][in_dim] f32 */
    const float* action;         /* [T][B][6] f32 */
    const float* logp;           /* [T][B] f32 */
    const float* advantage;      /* [T][B] f32 */
    const float* returns;        /* [T][B] f32 */
    const float* value;          /* [T][B] f32 */
    const uint8_t* episode_starts; /* [T][B] */
    const float* state_src[4];   /* [T/L][B][state_dim[i]] f32 */
    float* mb_obs;               /* [L][S][in_dim] f32 out */
    float* mb_action;            /* [L][S][6] f32 out */
    float* mb_logp;              /* [L][S] f32 out */
    float* mb_adv;               /* [L][S] f32 out */
    float* mb_ret;               /* [L][S] f32 out */
    float* mb_value;             /* [L][S] f32 out */
    uint8_t* mb_start;           /* [L][S] out */
    float* state_out[4];         /* [S][state_dim[i]] f32 out */
    int32_t* mb_index;           /* [S] i32 out, or NULL */
    double* adv_stats;           /* [2] out: mean, unbiased standard deviation of mb_adv, or NULL */
    double* workspace;           /* [1024][2] doubles, or NULL without adv_stats */
    int64_t workspace_bytes;
} glgym_seq_batch_args;

int glgym_lstm_cell(glgym_handle h, const glgym_lstm_cell_args* a, void* stream);
int glgym_lstm_cell_grad(glgym_handle h, const glgym_lstm_cell_grad_args* a, void* stream);
int glgym_seq_batch(glgym_handle h, const glgym_seq_batch_args* a, void* stream);

/* ---- on-device VecNormalize ---------------------------------------------------------------------
 * Replaces stable_baselines3.common.vec_env.VecNormalize (3rd party, pinned ==2.6.0 in the reference's requirements.txt)
 * as the reference configures it: norm_obs, norm_reward, clip_obs = 10, gamma (gl_gym/RL/experiment_manager.py:142-147,
 * gl_gym/RL/utils.py:62-66).  Algorithm: batch mean/var -> RunningMeanStd.update_from_moments -> clip((x-mean)/sqrt(var+eps));
 * rewards: returns = returns*gamma + r; ret_rms.update(returns); clip(r/sqrt(ret_var+eps)); returns[done] = 0.
 * All statistics are caller-owned device doubles so they can be saved / restored like VecNormalize.save(). */
typedef struct {
    int32_t B, dim;
    const float* obs;          /* [B][dim] raw observations (glgym_obs output) */
    float* obs_out;            /* [B][dim] normalised + clipped (may alias obs) */
    const void* reward;        /* [B] T raw rewards, or NULL (reset: observations only) */
    float* reward_out;         /* [B] f32 normalised + clipped */
    const uint8_t* done;       /* [B] or NULL */
    double* obs_mean;          /* [dim] running mean   (init 0) */
    double* obs_var;           /* [dim] running var    (init 1) */
    double* obs_count;         /* [1]   running count  (init 1e-4) */
    double* ret_stats;         /* [3]   mean, var, count of the discounted returns (init 0, 1, 1e-4) */
    double* returns;           /* [B]   discounted return accumulators (init 0) */
    double* workspace;         /* [32*dim + 2] scratch, zeroed by the call */
    double gamma, epsilon;     /* 0.99, 1e-8 in SB3 */
    float clip_obs, clip_reward;
    int32_t training, norm_obs, norm_reward;
} glgym_vecnorm_args;

int glgym_vecnorm(glgym_handle h, const glgym_vecnorm_args* a, void* stream);

/* ---- weather pipeline on the device -----------------------------------------------------------------------
 * Replaces the array part of load_weather_data (gl_gym/environments/utils.py:48-125; called per reset at
 * tomato_env.py:249-259): raw samples (the CSV columns, already sliced to the season window) -> vpOut / co2Out / tSoOut
 * unit conversions (:281-444, :262-279), daily light sum (:216-250), daylight flags with their one-hour ramps (:177-214),
 * PCHIP resample (scipy PchipInterpolator, Fritsch-Carlson slopes) onto linspace(time[0], time[n_raw-1], n_out), and the
 * iGlob < 1e-10 -> 0 clean-up.  fp64 arithmetic, output in the handle's dtype, row-major [n_out][nd] -- the table
 * glgym_step / glgym_obs / glgym_reset read.  Parsing the CSV stays with the caller. */
typedef struct {
    int32_t n_raw;             /* raw samples (>= 3), uniformly spaced in time */
    const double* time;        /* [n_raw] device: seconds */
    const double* i_glob;      /* [n_raw] device: global radiation [W m-2]      ("global radiation") */
    const double* t_out;       /* [n_raw] device: outdoor temperature [C]       ("air temperature") */
    const double* rh;          /* [n_raw] device: relative humidity [%]         ("RH") */
    const double* wind;        /* [n_raw] device: wind speed [m s-1]            ("wind speed") */
    const double* t_sky;       /* [n_raw] device: sky temperature [C]           ("sky temperature") */
    double co2_ppm;            /* outdoor CO2 (the reference uses 400) */
    int32_t n_out;             /* rows of the resampled table: int(dt_raw / dt_env * n_raw) */
    int32_t nd;                /* row stride of out (>= 10; columns 10.. are zeroed) */
    void* out;                 /* [n_out][nd] T device */
    double* workspace;         /* [20 * n_raw] device scratch */
} glgym_weather_args;

int glgym_weather(glgym_handle h, const glgym_weather_args* a, void* stream);

/* Kernel timing on the stream the kernels are launched on (bench.py's roofline leg). */
int glgym_timer_start(glgym_handle h, void* stream);
int glgym_timer_stop(glgym_handle h, void* stream, float* elapsed_ms);   /* synchronises the stop event */

#ifdef __cplusplus
}
#endif
#endif /* GLGYM_H */
