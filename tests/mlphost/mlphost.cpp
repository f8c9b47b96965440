// Host (g++) instantiation of the product's csrc/gl_mlp.hpp -- tests only (tests/test_plan_policy_host.py).  A lane of
// policy_rows_kernel is one call of forward on row b with the weights of theta row policy_row(b, S, J, mode); the two activation
// buffers the kernel keeps in LDS are two exactly sized heap arrays here.
// With -DMLPHOST_MAIN the file is a stand-alone program (the one the sanitizers run on): it drives the entries below over small and
// awkward shapes with exactly sized heap buffers and prints "mlphost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "glgym.h"
#include "gl_mlp.hpp"

extern "C" {

int mlphost_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(glgym_mlp_net);
        case 1: return (int)sizeof(glgym_policy_rows_args);
        case 2: return (int)sizeof(glgym_plan_rollout_policy_args);
    }
    return -1;
}

// 0: the net is accepted; 1: refused, the reason copied to msg (at most n bytes)
int mlphost_net_error(const glgym_mlp_net* net, char* msg, int n)
{
    const char* why = glmlp::net_error(net);
    if (why && msg && n > 0) { std::strncpy(msg, why, (size_t)n - 1); msg[n - 1] = 0; }
    return why ? 1 : 0;
}

long long mlphost_n_params(const glgym_mlp_net* net) { return (long long)glmlp::n_params(*net); }
int mlphost_buffer_rows(const glgym_mlp_net* net) { return glmlp::buffer_rows(*net); }
int mlphost_policy_row(int c, int S, int J, int mode) { return glmlp::policy_row(c, S, J, mode); }

// glgym_policy_rows on the host: obs [B][in_dim], theta [Ht][J][6], action [B][6] out (net->mean / inv_std are host pointers here)
void mlphost_rows(const glgym_mlp_net* net, const float* obs, const float* theta, int J, int S, int mode, int B, float* action)
{
    const int rows = glmlp::buffer_rows(*net);
    std::vector<float> a((size_t)rows), b((size_t)rows);         // exactly sized: an index past a buffer is the sanitizer's to report
    float* two[2] = {a.data(), b.data()};
    auto buf = [&](int which, int k) -> float& { return two[which][k]; };
    for (int r = 0; r < B; ++r) {
        const int j = glmlp::policy_row(r, S, J, mode);
        glmlp::forward(*net, obs + (size_t)r * net->in_dim, theta + (size_t)j * glmlp::NU, (size_t)J * glmlp::NU, buf,
                       action + (size_t)r * glmlp::NU);
    }
}

}  // extern "C"

#ifdef MLPHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

glgym_mlp_net net_of(int in_dim, int n_hidden, const int* width, int act, int squash)
{
    glgym_mlp_net n;
    std::memset(&n, 0, sizeof n);
    n.in_dim = in_dim; n.n_hidden = n_hidden;
    for (int l = 0; l < n_hidden; ++l) n.width[l] = width[l];
    n.activation = act; n.squash = squash;
    for (int g = 0; g < 8; ++g) n.scale[g] = 0.25f + 0.125f * g;
    n.clip_obs = 10.0f;
    return n;
}

void drive(int in_dim, int n_hidden, const int* width, int act, int squash, bool norm, int J, int S, int mode)
{
    glgym_mlp_net n = net_of(in_dim, n_hidden, width, act, squash);
    EXPECT(mlphost_net_error(&n, nullptr, 0) == 0);
    const long long D = mlphost_n_params(&n);
    const int Ht = (int)((D + 5) / 6);
    const int B = mode == GLGYM_POLICY_ROW_CHILD ? J * (S > 1 ? S : 1) : 3 * J * (S > 1 ? S : 1) + 1;
    std::vector<float> mean((size_t)in_dim, 0.5f), inv_std((size_t)in_dim, 2.0f);       // exactly in_dim entries
    if (norm) { n.mean = mean.data(); n.inv_std = inv_std.data(); }
    std::vector<float> theta((size_t)Ht * J * 6), obs((size_t)B * in_dim), act_out((size_t)B * 6);
    for (size_t i = 0; i < theta.size(); ++i) theta[i] = (float)((int)(i % 9) - 4) * 0.2f;
    for (size_t i = 0; i < obs.size(); ++i) obs[i] = (float)((int)(i % 7) - 3) * 0.5f;
    theta[0] = std::numeric_limits<float>::quiet_NaN();
    obs[obs.size() - 1] = std::numeric_limits<float>::quiet_NaN();
    mlphost_rows(&n, obs.data(), theta.data(), J, S, mode, B, act_out.data());
    for (size_t i = 0; i < act_out.size(); ++i) EXPECT(act_out[i] >= -1.0f && act_out[i] <= 1.0f);      // false for a NaN
}

}  // namespace

int main()
{
    EXPECT(mlphost_sizeof(0) > 0 && mlphost_sizeof(1) > 0 && mlphost_sizeof(2) > 0);
    const int none[3] = {0, 0, 0}, one[3] = {1, 0, 0}, five[3] = {5, 0, 0}, three[3] = {8, 7, 64};
    for (int act = 0; act < 3; ++act)
        for (int squash = 0; squash < 2; ++squash) {
            drive(1, 0, none, act, squash, false, 1, 0, GLGYM_POLICY_ROW_CHILD);
            drive(23, 1, one, act, squash, true, 3, 1, GLGYM_POLICY_ROW_CANDIDATE);
            drive(33, 1, five, act, squash, false, 5, 3, GLGYM_POLICY_ROW_CHILD);
            drive(23, 3, three, act, squash, true, 2, 3, GLGYM_POLICY_ROW_CANDIDATE);
            drive(130, 1, five, act, squash, true, 2, 0, GLGYM_POLICY_ROW_CHILD);       // three tiles of inputs, the last of 2
            drive(1024, 0, none, act, squash, false, 1, 0, GLGYM_POLICY_ROW_CHILD);
        }
    glgym_mlp_net bad = net_of(23, 1, five, 0, 0);
    char msg[64];
    bad.width[0] = 65;
    EXPECT(mlphost_net_error(&bad, msg, (int)sizeof msg) == 1 && msg[0]);
    std::printf(failures ? "mlphost FAILED (%d)\n" : "mlphost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
