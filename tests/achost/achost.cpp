// Host (g++) instantiation of the product's csrc/gl_actor.hpp -- tests only (tests/test_collect_host.py, and the reference the GPU tests
// of tests/test_gpu_collect.py compare the kernels with).  A lane of ac_rows_kernel is one pass of achost_rows' loop over row b, a lane
// of gae_kernel one call of gae_env.
// With -DACHOST_MAIN the file is a stand-alone program (the one the sanitizers run on): it drives the entries below over small and
// awkward shapes with exactly sized heap buffers and prints "achost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "glgym.h"
#include "gl_actor.hpp"

extern "C" {

int achost_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(glgym_ac_rows_args);
        case 1: return (int)sizeof(glgym_gae_args);
    }
    return -1;
}

unsigned achost_key_tag(void) { return glactor::KEY_TAG; }

// e [B][6] of rows 0 .. B-1
void achost_noise(int B, int step, unsigned long long D, unsigned long long seed, float* e)
{
    for (int b = 0; b < B; ++b) glactor::noise((uint32_t)b, (uint32_t)step, D, seed, e + (size_t)b * glactor::NU);
}

// glgym_ac_rows on the host: every pointer of the block is a host pointer, the arguments are taken as checked
void achost_rows(const glgym_ac_rows_args* a)
{
    constexpr int NU = glactor::NU;
    const uint64_t D = a->draw_index + (a->draw_base ? *a->draw_base : 0ull);
    for (int b = 0; b < a->B; ++b) {
        if (!a->value_only) {
            if (a->obs_out)
                for (int k = 0; k < a->in_dim; ++k) a->obs_out[(size_t)b * a->in_dim + k] = a->obs[(size_t)b * a->in_dim + k];
            float e[NU], act[NU], env[NU], logp;
            if (a->deterministic)
                for (int j = 0; j < NU; ++j) e[j] = 0.0f;
            else
                glactor::noise((uint32_t)b, (uint32_t)a->step, D, a->seed, e);
            glactor::sample(a->mean_in + (size_t)b * NU, a->std, a->log_std, e, act, env, &logp);
            for (int j = 0; j < NU; ++j) {
                a->action[(size_t)b * NU + j] = act[j];
                a->action_env[(size_t)b * NU + j] = env[j];
                if (a->eps) a->eps[(size_t)b * NU + j] = e[j];
            }
            a->logp[b] = logp;
        }
        a->value[b] = a->value_in[b];
    }
}

void achost_gae(const glgym_gae_args* a)
{
    for (int b = 0; b < a->B; ++b)
        glactor::gae_env(a->T, (size_t)a->B, a->reward + b, a->done + b, a->value + b, a->last_value[b], (float)a->gamma, (float)a->lambda,
                         a->advantage + b, a->returns + b);
}

}  // extern "C"

#ifdef ACHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

void drive(int in_dim, int B, int mode)
{
    std::vector<float> obs((size_t)B * in_dim), obs_out((size_t)B * in_dim), action((size_t)B * 6), env((size_t)B * 6), eps((size_t)B * 6),
        logp((size_t)B), value((size_t)B), mean_in((size_t)B * 6, 0.25f), value_in((size_t)B, 1.5f);
    for (size_t i = 0; i < obs.size(); ++i) obs[i] = (float)((int)(i % 7) - 3) * 0.5f;
    mean_in[0] = std::numeric_limits<float>::quiet_NaN();
    const float log_std[6] = {0.0f, -0.5f, 0.25f, -1.0f, 0.0f, 0.5f}, sd[6] = {1.0f, 0.6065307f, 1.2840254f, 0.36787945f, 1.0f, 1.6487212f};
    const uint64_t base = 3;
    glgym_ac_rows_args a;
    std::memset(&a, 0, sizeof a);
    a.struct_size = (int32_t)sizeof a; a.B = B; a.in_dim = in_dim; a.step = 5; a.deterministic = mode == 1; a.value_only = mode == 2;
    a.mean_in = mean_in.data(); a.value_in = value_in.data();
    a.log_std = log_std; a.std = sd; a.seed = 0x123456789abcdefull; a.draw_index = 7; a.draw_base = &base;
    a.obs = obs.data(); a.obs_out = mode == 2 ? nullptr : obs_out.data(); a.action = action.data(); a.action_env = env.data();
    a.eps = mode == 0 ? eps.data() : nullptr; a.logp = logp.data(); a.value = value.data();
    achost_rows(&a);
    if (mode != 2)
        for (size_t i = 0; i < env.size(); ++i) EXPECT(env[i] >= -1.0f && env[i] <= 1.0f);            // false for a NaN
    for (size_t i = 0; i < value.size(); ++i) EXPECT(value[i] == 1.5f);
}

void drive_gae(int T, int B)
{
    std::vector<float> r((size_t)T * B), v((size_t)T * B), last((size_t)B), adv((size_t)T * B), ret((size_t)T * B);
    std::vector<uint8_t> d((size_t)T * B);
    for (size_t i = 0; i < r.size(); ++i) { r[i] = 0.1f * (float)(i % 5); v[i] = 0.3f * (float)(i % 3); d[i] = (uint8_t)(i % 4 == 0); }
    for (int b = 0; b < B; ++b) last[(size_t)b] = 1.0f;
    glgym_gae_args g;
    std::memset(&g, 0, sizeof g);
    g.struct_size = (int32_t)sizeof g; g.T = T; g.B = B; g.reward = r.data(); g.done = d.data(); g.value = v.data(); g.last_value = last.data();
    g.gamma = 0.99; g.lambda = 0.95; g.advantage = adv.data(); g.returns = ret.data();
    achost_gae(&g);
    for (size_t i = 0; i < adv.size(); ++i) EXPECT(std::isfinite(adv[i]) && std::isfinite(ret[i]));
}

}  // namespace

int main()
{
    EXPECT(achost_sizeof(0) > 0 && achost_sizeof(1) > 0);
    for (int mode = 0; mode < 3; ++mode) {
        drive(1, 1, mode);
        drive(23, 3, mode);
        drive(130, 65, mode);
    }
    for (int T = 1; T <= 5; T += 2) { drive_gae(T, 1); drive_gae(T, 65); }
    std::printf(failures ? "achost FAILED (%d)\n" : "achost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
