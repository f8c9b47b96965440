// TESTS ONLY.  Host (g++) instantiation of greenlight-gym2_amd/csrc/gl_bdf_env.hpp's bdf_env_row -- controls, the BDF step, the reward
// epilogue -- with bdfhost.cpp's team of one, for one environment in fp64 (SoA arrays with ld = 1).  The product library never links
// or loads this file.
#include "bdfhost.cpp"

#include "gl_bdf_env.hpp"

// One env-step of one environment.  x[28] and u[6] in/out (previous control in, applied control out), exactly one of action[6] /
// control[6], weather[weather_rows][nd], *timestep in/out, p[208] (the handle's block, default reward settings of TomatoEnv.yml).
// Outputs reward, info[11], done, step_flags and the solver statistics stats[5].
extern "C" void envstep_host(double* x, double* u, const float* action, const double* control, const double* weather, int weather_rows,
                             int nd, int w_off, int* timestep, int N, const double* p, double dt, double rtol, double atol, int max_steps,
                             double* reward, double* info, unsigned char* done, int* step_flags, int* stats)
{
    ModelConst<double> m;
    std::memset(&m, 0, sizeof m);
    make_model_const<double>(p, m);
    glgym_reward_cfg c;
    c.elec_price = 0.3; c.heating_price = 0.09; c.co2_price = 0.3; c.fruit_price = 1.6; c.dmfm = 0.065;
    c.fixed_greenhouse_cost = 15.0; c.fixed_co2_cost = 0.015; c.fixed_lamp_cost = 0.07; c.fixed_screen_cost = 2.0;
    c.pen_lamp = 0.1;
    c.co2_min = 300; c.co2_max = 1600; c.temp_min = 15; c.temp_max = 34; c.rh_min = 50; c.rh_max = 85;
    RewardConstBase<double> rw;
    make_reward_const<double>(p, dt, c, rw, nullptr, nullptr, nullptr);
    glbdf::BdfEnvArgs<double> a;
    a.ld = 1;
    a.x = x; a.u = u; a.action = action; a.control = control;
    a.weather = weather; a.weather_rows = weather_rows; a.nd = nd;
    a.w_off = &w_off; a.timestep = timestep; a.crop_p = nullptr; a.N = N;
    a.reward = reward; a.info = info; a.done = done; a.step_flags = step_flags;
    a.dt = dt; a.rtol = rtol; a.atol = atol; a.max_steps = max_steps;
    a.gasR = p[39]; a.tCanMin = p[162];
    a.du = 0.1f;
    for (int j = 0; j < NU; ++j) { a.u_min[j] = 0.f; a.u_max[j] = 1.f; }
    static thread_local glbdf::BdfEnvScratch sh;
    CropConst<double> cr;
    StepCoef<double> s;
    HostTeam tm{m, cr, s};
    const glbdf::BdfEnvResult<double> r = glbdf::bdf_env_row<double>(tm, sh, m, cr, s, rw, a, 0);
    for (int i = 0; i < glbdf::NSTAT; ++i) stats[i] = r.stats[i];
}
