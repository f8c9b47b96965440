// Host (g++) instantiation of the product's csrc/gl_sac.hpp -- tests only (tests/test_sac_host.py, and the reference the GPU tests of
// tests/test_gpu_sac.py compare the kernels with).  A lane of a kernel of glgym_sac.hip is one pass of a loop, a block one pass of the loop
// over b, a butterfly a loop over an array of 64, the finishing launch the loop over the workspace at the end.  The three transcendentals
// of the squashed Gaussian (exp, tanh, log in double) are the one thing a device and a host do not share: sachost_rows takes their results
// as optional inputs.  With -DSACHOST_MAIN the file is a stand-alone program (the one the sanitizers run on): it drives the entries below
// over small and awkward shapes with exactly sized heap buffers and prints "sachost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "glgym.h"
#include "gl_sac.hpp"

namespace {

using glsac::BLOCK;
using glsac::N_SUM;
using glsac::N_WAVE;
using glsac::NU;
using glsac::WAVE;

// lane[256][N_SUM] -> the block's partial [N_SUM]: wavefronts by butterfly (xor 32 .. 1), then in index order
void block_combine(const double* lane, double* out)
{
    for (int q = 0; q < N_SUM; ++q) {
        double part[N_WAVE];
        for (int w = 0; w < N_WAVE; ++w) {
            double v[WAVE];
            for (int l = 0; l < WAVE; ++l) v[l] = lane[(size_t)(w * WAVE + l) * N_SUM + q];
            for (int m = WAVE / 2; m > 0; m >>= 1) {
                double o[WAVE];
                for (int l = 0; l < WAVE; ++l) o[l] = v[l] + v[l ^ m];
                for (int l = 0; l < WAVE; ++l) v[l] = o[l];
            }
            part[w] = v[0];
        }
        double t = part[0];
        for (int w = 1; w < N_WAVE; ++w) t = t + part[w];
        out[q] = t;
    }
}

}  // namespace

extern "C" {

int sachost_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(glgym_sac_rows_args);
        case 1: return (int)sizeof(glgym_sac_rows_grad_args);
        case 2: return (int)sizeof(glgym_sac_batch_args);
        case 3: return (int)sizeof(glgym_sac_loss_args);
        case 4: return (int)sizeof(glgym_polyak_args);
    }
    return -1;
}

unsigned sachost_key_tag(int which) { return which ? glsac::SAMPLE_TAG : glsac::KEY_TAG; }
long long sachost_ws_bytes(void) { return (long long)glsac::LOSS_WS_BYTES; }

// e (blk0 = 0) or e2 (blk0 = 2) of rows row0 .. row0 + M - 1 -> out [M][6]
void sachost_noise(long long row0, int M, int step, int blk0, unsigned long long D, unsigned long long seed, float* out)
{
    for (int r = 0; r < M; ++r) glsac::noise((uint32_t)((uint64_t)row0 + (uint64_t)r), (uint32_t)step, (uint32_t)blk0, D, seed, out + (size_t)r * NU);
}

// glgym_sac_rows on the host.  eps_in / eps2_in [M][6], if given, replace the noise (Box-Muller goes through libm too), std_in / tanh_in /
// corr_in [M][6] the results of exp, tanh and log, element by element.
void sachost_rows(const glgym_sac_rows_args* a, const float* eps_in, const float* eps2_in, const float* std_in, const float* tanh_in,
                  const float* corr_in)
{
    const uint64_t D = a->draw_index + (a->draw_base ? *a->draw_base : 0ull);
    const float sigma = (float)a->action_noise_sigma;
    if (a->obs_out)
        for (size_t i = 0; i < (size_t)a->M * (size_t)a->in_dim; ++i) a->obs_out[i] = a->obs[i];
    for (int64_t r = 0; r < a->M; ++r) {
        const uint32_t key = (uint32_t)((uint64_t)a->row0 + (uint64_t)r);
        float act[NU], e2[NU] = {0, 0, 0, 0, 0, 0};
        if (sigma > 0.0f && !a->uniform) glsac::noise(key, (uint32_t)a->step, 2u, D, a->seed, e2);
        if (eps2_in)
            for (int j = 0; j < NU; ++j) e2[j] = eps2_in[(size_t)r * NU + j];
        if (a->uniform) {
            glsac::uniform(key, (uint32_t)a->step, D, a->seed, act);
        } else {
            float e[NU] = {0, 0, 0, 0, 0, 0}, ls[NU], sd[NU], l[NU];
            if (!a->deterministic) glsac::noise(key, (uint32_t)a->step, 0u, D, a->seed, e);
            if (eps_in)
                for (int j = 0; j < NU; ++j) e[j] = eps_in[(size_t)r * NU + j];
            for (int j = 0; j < NU; ++j) {
                const size_t i = (size_t)r * NU + j;
                ls[j] = glsac::clamp_ls(a->log_std_in[i]);
                sd[j] = std_in ? std_in[i] : glsac::std_of(ls[j]);
                const float u = glsac::u_of(a->mean_in[i], sd[j], e[j]);
                act[j] = tanh_in ? tanh_in[i] : glsac::tanh_of(u);
                const float c = glsac::c_of(act[j]);
                l[j] = corr_in ? corr_in[i] : glsac::log_of(c);
            }
            if (a->logp) a->logp[r] = glsac::logp_of(e, ls, l);
            for (int j = 0; j < NU; ++j) {
                const size_t i = (size_t)r * NU + j;
                if (a->eps) a->eps[i] = e[j];
                if (a->eps2) a->eps2[i] = e2[j];
                if (a->std) a->std[i] = sd[j];
                if (a->tanh) a->tanh[i] = act[j];
                if (a->corr) a->corr[i] = l[j];
            }
        }
        for (int j = 0; j < NU; ++j) {
            const size_t i = (size_t)r * NU + j;
            const float env = glsac::env_of(act[j], a->uniform ? 0.0f : sigma, e2[j]);
            if (a->action) a->action[i] = act[j];
            if (a->action_env) a->action_env[i] = env;
            if (a->action_slot) a->action_slot[i] = env;
        }
    }
}

// u [M][6] of a call (what tanh is taken of), given the deviations: for the test of tanh
void sachost_u(const glgym_sac_rows_args* a, const float* eps_in, const float* std_in, float* u_out, float* c_out, const float* tanh_in)
{
    const uint64_t D = a->draw_index + (a->draw_base ? *a->draw_base : 0ull);
    for (int64_t r = 0; r < a->M; ++r) {
        float e[NU] = {0, 0, 0, 0, 0, 0};
        if (!a->deterministic) glsac::noise((uint32_t)((uint64_t)a->row0 + (uint64_t)r), (uint32_t)a->step, 0u, D, a->seed, e);
        for (int j = 0; j < NU; ++j) {
            const size_t i = (size_t)r * NU + j;
            u_out[i] = glsac::u_of(a->mean_in[i], std_in[i], eps_in ? eps_in[i] : e[j]);
            if (c_out) c_out[i] = glsac::c_of(tanh_in[i]);
        }
    }
}

void sachost_rows_grad(const glgym_sac_rows_grad_args* a)
{
    for (int64_t r = 0; r < a->M; ++r)
        for (int j = 0; j < NU; ++j) {
            const size_t i = (size_t)r * NU + j;
            glsac::squash_grad(a->grad_action[i], a->grad_logp[r], a->eps[i], a->std[i], a->tanh[i], a->log_std_in[i], a->grad_mean + i,
                               a->grad_log_std + i);
        }
}

void sachost_batch(const glgym_sac_batch_args* a)
{
    const uint64_t D = a->draw_index + (a->draw_base ? *a->draw_base : 0ull);
    const uint64_t n = (uint64_t)a->n_valid * (uint64_t)a->B;
    const size_t d = (size_t)a->in_dim;
    for (int64_t m = 0; m < a->M; ++m) {
        uint32_t row, nxt;
        glsac::ring_rows(glsac::sample_index((uint32_t)m, n, D, a->seed), a->S, a->B, a->head, &row, &nxt);
        for (size_t c = 0; c < d; ++c) {
            a->mb_obs[(size_t)m * d + c] = a->obs[(size_t)row * d + c];
            a->mb_next_obs[(size_t)m * d + c] = a->obs[(size_t)nxt * d + c];
        }
        for (int j = 0; j < NU; ++j) a->mb_action[(size_t)m * NU + j] = a->action[(size_t)row * NU + j];
        a->mb_reward[m] = a->reward[row];
        a->mb_done[m] = a->done[row];
        if (a->index_out) a->index_out[m] = (int64_t)row;
    }
}

void sachost_loss(const glgym_sac_loss_args* a)
{
    const int nb = glsac::n_blocks(a->M);
    const int64_t M = a->M;
    const glsac::Hyper hy = glsac::hyper(a->M, a->gamma, a->target_entropy);
    const float alpha = *a->alpha;
    for (int b = 0; b < nb; ++b) {
        std::vector<glsac::Sums> acc(BLOCK);
        for (auto& s : acc) glsac::sums_init(s);
        for (int64_t k = b; k * BLOCK < M; k += nb)
            for (int t = 0; t < BLOCK; ++t) {
                const int64_t r = k * BLOCK + t;
                if (r >= M) continue;
                if (a->stage == 0) {
                    glsac::CriticRow o;
                    glsac::critic_row(hy, alpha, a->q1[r], a->q2[r], a->q1_next[r], a->q2_next[r], a->logp[r], a->reward[r], a->done[r], o,
                                      acc[(size_t)t]);
                    a->grad_q1[r] = o.g1;
                    a->grad_q2[r] = o.g2;
                    if (a->target_out) a->target_out[r] = o.y;
                } else {
                    glsac::ActorRow o;
                    glsac::actor_row(hy, alpha, a->q1[r], a->q2[r], a->logp[r], o, acc[(size_t)t]);
                    a->grad_q1[r] = o.g1;
                    a->grad_q2[r] = o.g2;
                    a->grad_logp[r] = hy.w * alpha;
                }
            }
        std::vector<double> lane((size_t)BLOCK * N_SUM);
        for (int t = 0; t < BLOCK; ++t)
            for (int q = 0; q < N_SUM; ++q) lane[(size_t)t * N_SUM + q] = acc[(size_t)t].s[q];
        block_combine(lane.data(), a->workspace + (size_t)b * N_SUM);
    }
    double S[N_SUM];
    for (int q = 0; q < N_SUM; ++q) {
        S[q] = a->workspace[q];
        for (int b = 1; b < nb; ++b) S[q] = S[q] + a->workspace[(size_t)b * N_SUM + q];
    }
    if (a->stage == 0) {
        glsac::critic_stats(S, a->M, alpha, a->stats);
    } else {
        float g;
        glsac::actor_stats(S, a->M, alpha, *a->log_alpha, a->stats, &g);
        if (a->grad_log_alpha) *a->grad_log_alpha = g;
    }
}

// glgym_polyak on the host: the tables are host arrays of host pointers
void sachost_polyak(const glgym_polyak_args* a)
{
    const float tau = (float)a->tau, omt = 1.0f - tau;
    for (int k = 0; k < a->n; ++k)
        for (int64_t i = 0; i < a->count[k]; ++i) a->dst[k][i] = glsac::polyak(a->dst[k][i], a->src[k][i], tau, omt);
}

}  // extern "C"

#ifdef SACHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

void drive_rows(int M, int in_dim, int uniform, double sigma)
{
    std::vector<float> mean((size_t)M * 6), ls((size_t)M * 6), obs((size_t)M * in_dim), obs_out((size_t)M * in_dim);
    for (size_t i = 0; i < mean.size(); ++i) { mean[i] = 0.3f * (float)((int)(i % 7) - 3); ls[i] = (float)((int)(i % 27) - 22); }
    for (size_t i = 0; i < obs.size(); ++i) obs[i] = (float)i;
    if (M > 2) { mean[7] = std::numeric_limits<float>::quiet_NaN(); ls[13] = std::numeric_limits<float>::infinity(); }
    std::vector<float> act((size_t)M * 6), env((size_t)M * 6), slot((size_t)M * 6), logp((size_t)M), eps((size_t)M * 6), sd((size_t)M * 6),
        th((size_t)M * 6), corr((size_t)M * 6), gm((size_t)M * 6), gs((size_t)M * 6), ga((size_t)M * 6, 0.5f), gl((size_t)M, -0.25f);
    const uint64_t base = 3;
    glgym_sac_rows_args a;
    std::memset(&a, 0, sizeof a);
    a.struct_size = (int32_t)sizeof a; a.M = M; a.in_dim = in_dim; a.step = 5; a.uniform = uniform; a.row0 = 4294967296ll - M; a.seed = 99;
    a.draw_index = 1; a.draw_base = &base; a.action_noise_sigma = sigma; a.mean_in = mean.data(); a.log_std_in = ls.data();
    a.obs = obs.data(); a.obs_out = obs_out.data(); a.action = act.data(); a.action_env = env.data(); a.action_slot = slot.data();
    if (!uniform) { a.logp = logp.data(); a.eps = eps.data(); a.std = sd.data(); a.tanh = th.data(); a.corr = corr.data(); }
    sachost_rows(&a, nullptr, nullptr, nullptr, nullptr, nullptr);
    for (size_t i = 0; i < env.size(); ++i) EXPECT(env[i] >= -1.0f && env[i] <= 1.0f && env[i] == slot[i]);
    EXPECT(obs_out == obs);
    if (uniform) return;
    sachost_rows(&a, eps.data(), nullptr, sd.data(), th.data(), corr.data());
    glgym_sac_rows_grad_args g;
    std::memset(&g, 0, sizeof g);
    g.struct_size = (int32_t)sizeof g; g.M = M; g.grad_action = ga.data(); g.grad_logp = gl.data(); g.eps = eps.data(); g.std = sd.data();
    g.tanh = th.data(); g.log_std_in = ls.data(); g.grad_mean = gm.data(); g.grad_log_std = gs.data();
    sachost_rows_grad(&g);
    EXPECT(std::isfinite(gm[0]));
}

void drive_batch(int S, int B, int head, int n_valid, int M, int in_dim)
{
    const size_t N = (size_t)S * B;
    std::vector<float> obs(N * in_dim), action(N * 6), reward(N);
    std::vector<uint8_t> done(N);
    for (size_t i = 0; i < N; ++i) { reward[i] = (float)i; done[i] = (uint8_t)(i % 3 == 0); for (int c = 0; c < in_dim; ++c) obs[i * in_dim + c] = (float)i; }
    std::vector<float> mo((size_t)M * in_dim), mn((size_t)M * in_dim), ma((size_t)M * 6), mr((size_t)M);
    std::vector<uint8_t> md((size_t)M);
    std::vector<int64_t> idx((size_t)M);
    glgym_sac_batch_args a;
    std::memset(&a, 0, sizeof a);
    a.struct_size = (int32_t)sizeof a; a.S = S; a.B = B; a.in_dim = in_dim; a.M = M; a.head = head; a.n_valid = n_valid; a.seed = 5; a.draw_index = 2;
    a.obs = obs.data(); a.action = action.data(); a.reward = reward.data(); a.done = done.data(); a.mb_obs = mo.data(); a.mb_next_obs = mn.data();
    a.mb_action = ma.data(); a.mb_reward = mr.data(); a.mb_done = md.data(); a.index_out = idx.data();
    sachost_batch(&a);
    for (int m = 0; m < M; ++m) {
        const int64_t row = idx[(size_t)m], slot = row / B, b = row % B;
        EXPECT((slot - head + S) % S < n_valid);
        EXPECT(mr[(size_t)m] == (float)row && mn[(size_t)m * in_dim] == (float)(((slot + 1) % S) * B + b));
    }
}

void drive_loss(int M, int stage)
{
    std::vector<float> q1((size_t)M), q2((size_t)M), lp((size_t)M), q1n((size_t)M), q2n((size_t)M), r((size_t)M), g1((size_t)M), g2((size_t)M),
        gl((size_t)M), y((size_t)M);
    std::vector<uint8_t> done((size_t)M);
    for (int i = 0; i < M; ++i) { q1[(size_t)i] = 0.1f * (float)(i % 11); q2[(size_t)i] = 0.5f; lp[(size_t)i] = -3.0f; q1n[(size_t)i] = 1.0f; q2n[(size_t)i] = 0.5f; r[(size_t)i] = 0.25f; done[(size_t)i] = (uint8_t)(i % 5 == 0); }
    std::vector<double> ws(glsac::LOSS_WS_BYTES / sizeof(double)), stats(8);
    const float alpha = 0.2f, log_alpha = -1.609438f;
    float gla = 0;
    glgym_sac_loss_args a;
    std::memset(&a, 0, sizeof a);
    a.struct_size = (int32_t)sizeof a; a.M = M; a.stage = stage; a.q1 = q1.data(); a.q2 = q2.data(); a.logp = lp.data(); a.alpha = &alpha;
    a.gamma = 0.96; a.target_entropy = -6.0; a.grad_q1 = g1.data(); a.grad_q2 = g2.data(); a.stats = stats.data(); a.workspace = ws.data();
    a.workspace_bytes = (int64_t)glsac::LOSS_WS_BYTES;
    if (stage == 0) { a.q1_next = q1n.data(); a.q2_next = q2n.data(); a.reward = r.data(); a.done = done.data(); a.target_out = y.data(); }
    else { a.log_alpha = &log_alpha; a.grad_logp = gl.data(); a.grad_log_alpha = &gla; }
    sachost_loss(&a);
    EXPECT(stats[7] == (double)M && std::isfinite(stats[0]));
}

void drive_polyak()
{
    std::vector<float> t0(1), t1(63), t2(258), s0(1, 1.0f), s1(63, 2.0f), s2(258, 3.0f), none;
    float* dst[4] = {t0.data(), none.data(), t1.data(), t2.data() + 1};
    const float* src[4] = {s0.data(), none.data(), s1.data(), s2.data() + 1};
    const int64_t count[4] = {1, 0, 63, 257};
    glgym_polyak_args a;
    std::memset(&a, 0, sizeof a);
    a.struct_size = (int32_t)sizeof a; a.n = 4; a.dst = dst; a.src = src; a.count = count; a.max_count = 257; a.tau = 0.25;
    sachost_polyak(&a);
    EXPECT(t0[0] == 0.25f && t1[62] == 0.5f && t2[0] == 0.0f && t2[257] == 0.75f);
}

}  // namespace

int main()
{
    for (int i = 0; i < 5; ++i) EXPECT(sachost_sizeof(i) > 0);
    for (int in_dim : {1, 23, 24})
        for (int M : {1, 65, 257}) {
            drive_rows(M, in_dim, 0, 0.0);
            drive_rows(M, in_dim, 0, 0.05);
            drive_rows(M, in_dim, 1, 0.0);
        }
    drive_batch(3, 5, 0, 1, 300, 3);
    drive_batch(3, 5, 2, 2, 300, 23);
    drive_batch(4, 1, 3, 3, 65, 1);
    drive_batch(2, 65537, 0, 1, 257, 2);
    for (int M : {1, 2, 65, 257, glsac::MAX_BLOCKS * BLOCK + 5}) {
        drive_loss(M, 0);
        drive_loss(M, 1);
    }
    drive_polyak();
    std::printf(failures ? "sachost FAILED (%d)\n" : "sachost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
