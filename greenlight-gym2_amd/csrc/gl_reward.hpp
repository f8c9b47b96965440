// gl_reward.hpp -- the reward epilogue's constants (rewards.py:96-124,156-231; TomatoEnv.yml:38-67) and the exact saturation vapour
// pressure of the indoor humidity observation (observations.py:70-77), shared by the env-step kernels of glgym.hip, the BDF env-step
// of glgym_bdf.hip and its host instantiation in tests/.  Compiles with a plain host compiler like gl_model.hpp.
#pragma once
#include "gl_model.hpp"
#include "glgym.h"

namespace glm {

template <class T> struct RewardConstBase {
    T heatK, elecK, co2K;       // cost per unit of u0 / u4 / u1 per env-step
    T gainK;                    // EUR per mg m-2 of fruit dry matter
    T minProfit, invRange;      // scale_reward(profit, min, max)
    T fixedCosts;
    T lo[3], hi[3], invMaxViol[3];
    T kPpm;
};

template <class T> inline void make_reward_const(const double* p, double dt, const glgym_reward_cfg& c, RewardConstBase<T>& r,
                                                 double* max_profit, double* min_profit, double* fixed_costs)
{
    const double heat = p[108] / p[46] * dt / 3600 * 1e-3 * c.heating_price;
    const double elec = p[172] * dt / 3600 * 1e-3 * c.elec_price;
    const double co2 = p[109] / p[46] * dt * 1e-6 * c.co2_price;
    const double maxP = p[154] * dt * 1e-6 / c.dmfm * c.fruit_price;
    const double minP = -(heat + elec + co2);
    const double yearly = c.fixed_greenhouse_cost + c.fixed_co2_cost + c.fixed_lamp_cost * 116 + c.fixed_screen_cost;
    const double fixed = yearly / 365 / (double)(86400 / (long)dt);       // rewards.py:155 uses floor division
    r.heatK = T(heat); r.elecK = T(elec); r.co2K = T(co2);
    r.gainK = T(1e-6 / c.dmfm * c.fruit_price);
    r.minProfit = T(minP); r.invRange = T(1.0 / (maxP - minP)); r.fixedCosts = T(fixed);
    r.lo[0] = T(c.co2_min); r.lo[1] = T(c.temp_min); r.lo[2] = T(c.rh_min);
    r.hi[0] = T(c.co2_max); r.hi[1] = T(c.temp_max); r.hi[2] = T(c.rh_max);
    r.invMaxViol[0] = T(1.0 / 2500.0); r.invMaxViol[1] = T(1.0 / 15.0); r.invMaxViol[2] = T(1.0 / 15.0);   // :89-93
    r.kPpm = T(8.3144598 / (101325.0 * 44.01e-3));
    if (max_profit) *max_profit = maxP;
    if (min_profit) *min_profit = minP;
    if (fixed_costs) *fixed_costs = fixed;
}

template <class T> GL_HD T sat_vp_exact(T t)
{
    return T(610.78) * Math<T>::exp(T(17.2694) * t / (t + T(238.3)));
}

}  // namespace glm
