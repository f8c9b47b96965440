// Host (g++) instantiation of the product's csrc/gl_ppo.hpp -- tests only (tests/test_ppo_host.py, and the reference the GPU tests of
// tests/test_gpu_ppo.py compare the kernels with).  A lane of ppo_batch_kernel / ppo_loss_kernel is one pass of the loop over t, a block
// one pass of the loop over b, a butterfly a loop over an array of 64, the finishing launch the loop over the workspace at the end.
// With -DPPOHOST_MAIN the file is a stand-alone program (the one the sanitizers run on): it drives the entries below over small and
// awkward shapes with exactly sized heap buffers and prints "ppohost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "glgym.h"
#include "gl_ppo.hpp"

namespace {

using glppo::BLOCK;
using glppo::N_ADV;
using glppo::N_SUM;
using glppo::N_WAVE;
using glppo::NU;
using glppo::WAVE;

// the 64 lanes of a wavefront by butterfly: every lane ends with the same value, lane 0's is returned
template <class Op> double butterfly(double v[WAVE], Op op)
{
    for (int m = WAVE / 2; m > 0; m >>= 1) {
        double o[WAVE];
        for (int l = 0; l < WAVE; ++l) o[l] = op(v[l], v[l ^ m]);
        for (int l = 0; l < WAVE; ++l) v[l] = o[l];
    }
    return v[0];
}

// lane[256][n] -> the block's partial [n]: wavefronts by butterfly, then in index order
template <class Op> void block_combine(const double* lane, int n, double* out, Op op)
{
    for (int q = 0; q < n; ++q) {
        double part[N_WAVE];
        for (int w = 0; w < N_WAVE; ++w) {
            double v[WAVE];
            for (int l = 0; l < WAVE; ++l) v[l] = lane[(size_t)(w * WAVE + l) * n + q];
            part[w] = butterfly(v, [&](double x, double y) { return op(q, x, y); });
        }
        double t = part[0];
        for (int w = 1; w < N_WAVE; ++w) t = op(q, t, part[w]);
        out[q] = t;
    }
}

}  // namespace

extern "C" {

int ppohost_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(glgym_ppo_batch_args);
        case 1: return (int)sizeof(glgym_ppo_loss_args);
    }
    return -1;
}

unsigned ppohost_key_tag(void) { return glppo::KEY_TAG; }
int ppohost_n_blocks(long long M) { return glppo::n_blocks(M); }
long long ppohost_ws_bytes(int which) { return which ? (long long)glppo::LOSS_WS_BYTES : (long long)glppo::BATCH_WS_BYTES; }

// perm(p) for p = p0 .. p0 + n - 1 of the permutation of [0, N)
void ppohost_perm(int N, int p0, int n, unsigned long long D, unsigned long long seed, unsigned tag, int32_t* out)
{
    const int half = glppo::half_bits((uint32_t)N);
    for (int i = 0; i < n; ++i) out[i] = (int32_t)glppo::perm((uint32_t)(p0 + i), (uint32_t)N, half, D, seed, tag);
}

// glgym_ppo_batch on the host: every pointer of the block is a host pointer, the arguments are taken as checked
void ppohost_batch(const glgym_ppo_batch_args* a)
{
    const uint64_t D = a->draw_index + (a->draw_base ? *a->draw_base : 0ull);
    const int half = glppo::half_bits((uint32_t)a->N), nb = glppo::n_blocks(a->M);
    const int64_t M = a->M;
    for (int b = 0; b < nb; ++b) {
        std::vector<double> lane((size_t)BLOCK * N_ADV, 0.0);
        for (int64_t k = b; k * BLOCK < M; k += nb) {
            for (int t = 0; t < BLOCK; ++t) {
                const int64_t m = k * BLOCK + t;
                if (m >= M) continue;
                const size_t i = glppo::perm((uint32_t)(a->offset + m), (uint32_t)a->N, half, D, a->seed);
                for (int c = 0; c < a->in_dim; ++c) a->mb_obs[(size_t)m * a->in_dim + c] = a->obs[i * a->in_dim + c];
                for (int j = 0; j < NU; ++j) a->mb_action[(size_t)m * NU + j] = a->action[i * NU + j];
                a->mb_logp[m] = a->logp[i];
                a->mb_adv[m] = a->advantage[i];
                a->mb_ret[m] = a->returns[i];
                a->mb_value[m] = a->value[i];
                if (a->mb_index) a->mb_index[m] = (int32_t)i;
                double term[N_ADV];
                glppo::adv_terms(a->advantage[i], term);
                for (int q = 0; q < N_ADV; ++q) lane[(size_t)t * N_ADV + q] = lane[(size_t)t * N_ADV + q] + term[q];
            }
        }
        if (a->adv_stats) block_combine(lane.data(), N_ADV, a->workspace + (size_t)b * N_ADV, [](int, double x, double y) { return x + y; });
    }
    if (!a->adv_stats) return;
    double S[N_ADV];
    for (int q = 0; q < N_ADV; ++q) {
        S[q] = a->workspace[q];
        for (int b = 1; b < nb; ++b) S[q] = S[q] + a->workspace[(size_t)b * N_ADV + q];
    }
    glppo::adv_stats_of(S[0], S[1], a->M, a->adv_stats);
}

// glgym_ppo_loss on the host.  ratio_in, if given, replaces (float) exp((double) d) row by row: the libm behind the exponential is the
// one thing a device and a host do not share.
void ppohost_loss(const glgym_ppo_loss_args* a, const float* ratio_in)
{
    const int nb = glppo::n_blocks(a->M);
    const int64_t M = a->M;
    const glppo::Hyper hy = glppo::hyper(a->M, a->clip_range, a->clip_range_vf, a->vf_coef, a->ent_coef);
    const glppo::Norm nrm = glppo::norm_of(a->adv_stats);
    for (int b = 0; b < nb; ++b) {
        std::vector<glppo::Sums> acc(BLOCK);
        for (auto& s : acc) glppo::sums_init(s);
        for (int64_t k = b; k * BLOCK < M; k += nb) {
            for (int t = 0; t < BLOCK; ++t) {
                const int64_t r = k * BLOCK + t;
                if (r >= M) continue;
                float z[NU];
                const float old_logp = a->mb_logp[r];
                const float logp = glppo::logp_of(a->mean + (size_t)r * NU, a->mb_action + (size_t)r * NU, a->inv_std, a->log_std, z);
                const float ratio = ratio_in ? ratio_in[r] : glppo::ratio_of(logp, old_logp);
                glppo::Row o;
                glppo::finish_row(hy, nrm, z, a->inv_std, logp, old_logp, ratio, a->mb_adv[r], a->value[r], hy.vclip ? a->mb_value[r] : 0.0f,
                                  a->mb_ret[r], o);
                for (int j = 0; j < NU; ++j) a->grad_mean[(size_t)r * NU + j] = o.grad_mean[j];
                a->grad_value[r] = o.grad_value;
                if (a->ratio_out) a->ratio_out[r] = ratio;
                if (a->logp_out) a->logp_out[r] = logp;
                glppo::sums_add(acc[(size_t)t], o, ratio);
            }
        }
        std::vector<double> lane((size_t)BLOCK * N_SUM);
        for (int t = 0; t < BLOCK; ++t)
            for (int q = 0; q < N_SUM; ++q) lane[(size_t)t * N_SUM + q] = acc[(size_t)t].s[q];
        block_combine(lane.data(), N_SUM, a->workspace + (size_t)b * N_SUM, glppo::combine);
    }
    double S[N_SUM];
    for (int q = 0; q < N_SUM; ++q) {
        S[q] = a->workspace[q];
        for (int b = 1; b < nb; ++b) S[q] = glppo::combine(q, S[q], a->workspace[(size_t)b * N_SUM + q]);
    }
    glppo::loss_stats(S, a->M, hy, a->log_std, a->stats, a->grad_log_std);
}

}  // extern "C"

#ifdef PPOHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

void drive_perm(int N)
{
    std::vector<int32_t> p((size_t)N);
    std::vector<uint8_t> seen((size_t)N, 0);
    ppohost_perm(N, 0, N, 5, 0x123456789abcdefull, glppo::KEY_TAG, p.data());
    for (int i = 0; i < N; ++i) {
        EXPECT(p[(size_t)i] >= 0 && p[(size_t)i] < N);
        if (p[(size_t)i] >= 0 && p[(size_t)i] < N) seen[(size_t)p[(size_t)i]] += 1;
    }
    for (int i = 0; i < N; ++i) EXPECT(seen[(size_t)i] == 1);
}

void drive_batch(int N, int M, int offset, int in_dim, bool stats)
{
    std::vector<float> obs((size_t)N * in_dim), action((size_t)N * 6), logp((size_t)N), adv((size_t)N), ret((size_t)N), value((size_t)N);
    for (size_t i = 0; i < obs.size(); ++i) obs[i] = (float)((int)(i % 11) - 5) * 0.25f;
    for (size_t i = 0; i < action.size(); ++i) action[i] = (float)((int)(i % 7) - 3) * 0.5f;
    for (int i = 0; i < N; ++i) { logp[(size_t)i] = -0.1f * (float)i; adv[(size_t)i] = (float)((i % 9) - 4); ret[(size_t)i] = 1.0f; value[(size_t)i] = (float)i; }
    std::vector<float> mb_obs((size_t)M * in_dim), mb_action((size_t)M * 6), mb_logp((size_t)M), mb_adv((size_t)M), mb_ret((size_t)M), mb_value((size_t)M);
    std::vector<int32_t> index((size_t)M);
    std::vector<double> ws(glppo::BATCH_WS_BYTES / sizeof(double)), st(2);
    const uint64_t base = 2;
    glgym_ppo_batch_args a;
    std::memset(&a, 0, sizeof a);
    a.struct_size = (int32_t)sizeof a; a.N = N; a.M = M; a.offset = offset; a.in_dim = in_dim; a.seed = 77; a.draw_index = 1; a.draw_base = &base;
    a.obs = obs.data(); a.action = action.data(); a.logp = logp.data(); a.advantage = adv.data(); a.returns = ret.data(); a.value = value.data();
    a.mb_obs = mb_obs.data(); a.mb_action = mb_action.data(); a.mb_logp = mb_logp.data(); a.mb_adv = mb_adv.data(); a.mb_ret = mb_ret.data();
    a.mb_value = mb_value.data(); a.mb_index = index.data();
    if (stats) { a.adv_stats = st.data(); a.workspace = ws.data(); a.workspace_bytes = (int64_t)glppo::BATCH_WS_BYTES; }
    ppohost_batch(&a);
    for (int m = 0; m < M; ++m) EXPECT(mb_value[(size_t)m] == (float)index[(size_t)m]);
    if (stats) EXPECT(std::isfinite(st[0]) && st[1] >= 0.0);
}

void drive_loss(int M, bool norm, double cv)
{
    std::vector<float> mean((size_t)M * 6), value((size_t)M), action((size_t)M * 6), logp((size_t)M), adv((size_t)M), ret((size_t)M), old_v((size_t)M);
    for (size_t i = 0; i < mean.size(); ++i) { mean[i] = 0.1f * (float)((int)(i % 5) - 2); action[i] = 0.3f * (float)((int)(i % 7) - 3); }
    for (int i = 0; i < M; ++i) { value[(size_t)i] = 0.5f; logp[(size_t)i] = -6.0f; adv[(size_t)i] = (float)((i % 3) - 1); ret[(size_t)i] = 1.0f; old_v[(size_t)i] = 0.25f; }
    if (M > 2) mean[6] = std::numeric_limits<float>::quiet_NaN();
    const float log_std[6] = {0.0f, -0.5f, 0.25f, -1.0f, 0.0f, 0.5f}, inv_std[6] = {1.0f, 1.6487212f, 0.7788008f, 2.7182817f, 1.0f, 0.60653067f};
    std::vector<float> gm((size_t)M * 6), gv((size_t)M), gl(6), ratio((size_t)M), lp((size_t)M);
    std::vector<double> ws(glppo::LOSS_WS_BYTES / sizeof(double)), stats(8);
    const double st[2] = {0.1, 0.8};
    glgym_ppo_loss_args a;
    std::memset(&a, 0, sizeof a);
    a.struct_size = (int32_t)sizeof a; a.M = M; a.mean = mean.data(); a.value = value.data(); a.log_std = log_std; a.inv_std = inv_std;
    a.mb_action = action.data(); a.mb_logp = logp.data(); a.mb_adv = adv.data(); a.mb_ret = ret.data(); a.mb_value = cv > 0 ? old_v.data() : nullptr;
    a.adv_stats = norm ? st : nullptr; a.clip_range = 0.2; a.clip_range_vf = cv; a.vf_coef = 0.5; a.ent_coef = 0.01;
    a.grad_mean = gm.data(); a.grad_value = gv.data(); a.grad_log_std = gl.data(); a.stats = stats.data(); a.ratio_out = ratio.data();
    a.logp_out = lp.data(); a.workspace = ws.data(); a.workspace_bytes = (int64_t)glppo::LOSS_WS_BYTES;
    ppohost_loss(&a, nullptr);
    EXPECT(stats[7] == (double)M);
    EXPECT(std::isfinite(gm[0]) && std::isfinite(gv[0]));
    if (M > 2) EXPECT(std::isnan(gm[6]) && std::isnan(stats[4]) && std::isfinite(gm[12]));
    ppohost_loss(&a, ratio.data());
}

}  // namespace

int main()
{
    EXPECT(ppohost_sizeof(0) > 0 && ppohost_sizeof(1) > 0);
    for (int N : {1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1000, 4097}) drive_perm(N);
    for (int in_dim : {1, 23, 24}) {
        drive_batch(1, 1, 0, in_dim, false);
        drive_batch(1000, 257, 300, in_dim, true);
        drive_batch(1000, 232, 768, in_dim, true);
    }
    drive_batch(glppo::MAX_BLOCKS * BLOCK + 300, glppo::MAX_BLOCKS * BLOCK + 5, 295, 3, true);
    for (int M : {1, 2, 65, 257}) {
        drive_loss(M, false, 0.0);
        drive_loss(M, M > 1, 0.1);
    }
    drive_loss(glppo::MAX_BLOCKS * BLOCK + 5, true, 0.0);
    std::printf(failures ? "ppohost FAILED (%d)\n" : "ppohost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
