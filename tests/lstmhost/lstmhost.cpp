// Host (g++) instantiation of the product's csrc/gl_lstm.hpp -- tests only (tests/test_rppo_host.py, and the reference the GPU tests of
// tests/test_gpu_rppo.py compare the kernels with).  A lane of lstm_cell_kernel / lstm_cell_grad_kernel is one pass of the loop over
// (row, unit), a lane of seq_batch_kernel one pass of the loop over the minibatch's sequences; the advantage statistics are summed as
// tests/ppohost/ppohost.cpp sums them.  With -DLSTMHOST_MAIN the file is a stand-alone program (the one the sanitizers run on): it drives
// the entries below over small and awkward shapes with exactly sized heap buffers and prints "lstmhost ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "glgym.h"
#include "gl_lstm.hpp"

namespace {

using glppo::BLOCK;
using glppo::N_ADV;
using glppo::N_WAVE;
using glppo::WAVE;
using glstm::N_ACT;
constexpr int NU = GLGYM_NU;

// glgym_ppo_batch's reduction over M flat rows: lanes, butterfly, wavefronts in index order, blocks in block order
void adv_stats_host(const float* adv, int64_t M, double* ws, double out[2])
{
    const int nb = glppo::n_blocks(M);
    for (int b = 0; b < nb; ++b) {
        std::vector<double> lane((size_t)BLOCK * N_ADV, 0.0);
        for (int64_t k = b; k * BLOCK < M; k += nb)
            for (int t = 0; t < BLOCK; ++t) {
                const int64_t m = k * BLOCK + t;
                if (m >= M) continue;
                double term[N_ADV];
                glppo::adv_terms(adv[m], term);
                for (int q = 0; q < N_ADV; ++q) lane[(size_t)t * N_ADV + q] = lane[(size_t)t * N_ADV + q] + term[q];
            }
        for (int q = 0; q < N_ADV; ++q) {
            double part[N_WAVE];
            for (int w = 0; w < N_WAVE; ++w) {
                double v[WAVE];
                for (int l = 0; l < WAVE; ++l) v[l] = lane[(size_t)(w * WAVE + l) * N_ADV + q];
                for (int m = WAVE / 2; m > 0; m >>= 1) {
                    double o[WAVE];
                    for (int l = 0; l < WAVE; ++l) o[l] = v[l] + v[l ^ m];
                    for (int l = 0; l < WAVE; ++l) v[l] = o[l];
                }
                part[w] = v[0];
            }
            double t = part[0];
            for (int w = 1; w < N_WAVE; ++w) t = t + part[w];
            ws[(size_t)b * N_ADV + q] = t;
        }
    }
    double S[N_ADV];
    for (int q = 0; q < N_ADV; ++q) {
        S[q] = ws[q];
        for (int b = 1; b < nb; ++b) S[q] = S[q] + ws[(size_t)b * N_ADV + q];
    }
    glppo::adv_stats_of(S[0], S[1], (int)M, out);
}

}  // namespace

extern "C" {

int lstmhost_sizeof(int which)
{
    switch (which) {
        case 0: return (int)sizeof(glgym_lstm_cell_args);
        case 1: return (int)sizeof(glgym_lstm_cell_grad_args);
        case 2: return (int)sizeof(glgym_seq_batch_args);
    }
    return -1;
}

int lstmhost_n_blocks(long long n_lane) { return glstm::n_blocks(n_lane); }

// glgym_lstm_cell on the host: every pointer of the block is a host pointer, the arguments are taken as checked.  act_in [M][5H], if given,
// replaces the five activations unit by unit: the libm behind exp and tanh is the one thing a device and a host do not share.
void lstmhost_cell(const glgym_lstm_cell_args* a, const float* act_in)
{
    const size_t H = (size_t)a->H;
    for (size_t row = 0; row < (size_t)a->M; ++row) {
        const bool keep = !a->start || a->start[row] == 0;
        for (size_t j = 0; j < H; ++j) {
            float gx[4], gh[4], act[N_ACT], c, h;
            for (size_t k = 0; k < 4; ++k) { gx[k] = a->gx[row * 4 * H + k * H + j]; gh[k] = a->gh[row * 4 * H + k * H + j]; }
            const float cp = a->c_prev[row * H + j];
            if (act_in) {
                float pre[4], c0;
                glstm::preact(keep, gx, gh, cp, pre, c0);
                for (size_t k = 0; k < (size_t)N_ACT; ++k) act[k] = act_in[row * N_ACT * H + k * H + j];
                c = glstm::cell_of(act[glstm::A_I], act[glstm::A_F], act[glstm::A_G], c0);
                h = glstm::hidden_of(act[glstm::A_O], act[glstm::A_TC]);
            } else {
                glstm::forward(keep, gx, gh, cp, act, c, h);
            }
            a->h[row * H + j] = h;
            a->c[row * H + j] = c;
            if (a->act)
                for (size_t k = 0; k < (size_t)N_ACT; ++k) a->act[row * N_ACT * H + k * H + j] = act[k];
        }
    }
}

void lstmhost_cell_grad(const glgym_lstm_cell_grad_args* a)
{
    const size_t H = (size_t)a->H;
    for (size_t row = 0; row < (size_t)a->M; ++row) {
        const bool keep = !a->start || a->start[row] == 0;
        for (size_t j = 0; j < H; ++j) {
            float act[N_ACT], da[4], dcp;
            for (size_t k = 0; k < (size_t)N_ACT; ++k) act[k] = a->act[row * N_ACT * H + k * H + j];
            glstm::backward(keep, a->dh[row * H + j], a->dc ? a->dc[row * H + j] : 0.0f, act, a->c_prev[row * H + j], da, dcp);
            for (size_t k = 0; k < 4; ++k) {
                a->d_gx[row * 4 * H + k * H + j] = da[k];
                a->d_gh[row * 4 * H + k * H + j] = keep ? da[k] : 0.0f;
            }
            a->d_c_prev[row * H + j] = dcp;
        }
    }
}

void lstmhost_seq_batch(const glgym_seq_batch_args* a)
{
    const uint64_t D = a->draw_index + (a->draw_base ? *a->draw_base : 0ull);
    const uint32_t N = (uint32_t)(a->T / a->L) * (uint32_t)a->B;
    const int half = glppo::half_bits(N);
    const size_t S = (size_t)a->S, B = (size_t)a->B, d = (size_t)a->in_dim;
    for (size_t s = 0; s < S; ++s) {
        const uint32_t q = glppo::perm((uint32_t)((size_t)a->offset + s), N, half, D, a->seed);
        const size_t r0 = glstm::first_row(q, (uint32_t)a->B, (uint32_t)a->L);
        if (a->mb_index) a->mb_index[s] = (int32_t)q;
        for (size_t l = 0; l < (size_t)a->L; ++l) {
            const size_t i = r0 + l * B, m = l * S + s;
            for (size_t c = 0; c < d; ++c) a->mb_obs[m * d + c] = a->obs[i * d + c];
            for (size_t j = 0; j < (size_t)NU; ++j) a->mb_action[m * NU + j] = a->action[i * NU + j];
            a->mb_logp[m] = a->logp[i];
            a->mb_adv[m] = a->advantage[i];
            a->mb_ret[m] = a->returns[i];
            a->mb_value[m] = a->value[i];
            a->mb_start[m] = a->episode_starts[i];
        }
        for (int k = 0; k < a->n_state; ++k) {
            const size_t w = (size_t)a->state_dim[k];
            for (size_t c = 0; c < w; ++c) a->state_out[k][s * w + c] = a->state_src[k][(size_t)q * w + c];
        }
    }
    if (a->adv_stats) adv_stats_host(a->mb_adv, (int64_t)a->L * (int64_t)a->S, a->workspace, a->adv_stats);
}

}  // extern "C"

#ifdef LSTMHOST_MAIN
namespace {

int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

void drive_cell(int M, int H, int start_kind, bool want_act, bool want_dc)
{
    const size_t MH = (size_t)M * H;
    std::vector<float> gx(4 * MH), gh(4 * MH), cp(MH), h(MH), c(MH), act(N_ACT * MH), dh(MH), dc(MH), dgx(4 * MH), dgh(4 * MH), dcp(MH);
    std::vector<uint8_t> start((size_t)M);
    for (size_t i = 0; i < 4 * MH; ++i) { gx[i] = 0.25f * (float)((int)(i % 13) - 6); gh[i] = 0.125f * (float)((int)(i % 7) - 3); }
    for (size_t i = 0; i < MH; ++i) { cp[i] = 0.5f * (float)((int)(i % 5) - 2); dh[i] = 0.1f * (float)((int)(i % 9) - 4); dc[i] = 0.05f * (float)(i % 3); }
    for (int r = 0; r < M; ++r) start[(size_t)r] = start_kind == 2 ? (uint8_t)(r % 3 == 1) : (uint8_t)(start_kind > 0);
    for (int r = 0; r < M; ++r)
        if (start[(size_t)r]) { cp[(size_t)r * H] = std::numeric_limits<float>::quiet_NaN(); gh[(size_t)r * 4 * H] = std::numeric_limits<float>::infinity(); }
    glgym_lstm_cell_args a;
    std::memset(&a, 0, sizeof a);
    a.struct_size = (int32_t)sizeof a; a.M = M; a.H = H; a.gx = gx.data(); a.gh = gh.data(); a.c_prev = cp.data();
    a.start = start_kind < 0 ? nullptr : start.data(); a.h = h.data(); a.c = c.data(); a.act = want_act ? act.data() : nullptr;
    lstmhost_cell(&a, nullptr);
    for (size_t i = 0; i < MH; ++i) EXPECT(std::isfinite(h[i]) && std::isfinite(c[i]) && std::fabs(h[i]) <= 1.0f);
    if (!want_act) return;
    std::vector<float> h2(MH), c2(MH);
    a.h = h2.data(); a.c = c2.data(); a.act = nullptr;
    lstmhost_cell(&a, act.data());
    EXPECT(std::memcmp(h.data(), h2.data(), MH * sizeof(float)) == 0 && std::memcmp(c.data(), c2.data(), MH * sizeof(float)) == 0);
    glgym_lstm_cell_grad_args g;
    std::memset(&g, 0, sizeof g);
    g.struct_size = (int32_t)sizeof g; g.M = M; g.H = H; g.dh = dh.data(); g.dc = want_dc ? dc.data() : nullptr; g.act = act.data();
    g.c_prev = cp.data(); g.start = a.start; g.d_gx = dgx.data(); g.d_gh = dgh.data(); g.d_c_prev = dcp.data();
    lstmhost_cell_grad(&g);
    for (int r = 0; r < M; ++r)
        for (int j = 0; j < H; ++j) {
            const bool keep = !a.start || !start[(size_t)r];
            EXPECT(std::isfinite(dgx[(size_t)r * 4 * H + j]) && std::isfinite(dcp[(size_t)r * H + j]));
            if (!keep) EXPECT(dgh[(size_t)r * 4 * H + j] == 0.0f && dcp[(size_t)r * H + j] == 0.0f);
        }
}

void drive_seq(int T, int B, int L, int S, int offset, int in_dim, int n_state, bool stats)
{
    const size_t R = (size_t)T * B, N = (size_t)(T / L) * B, M = (size_t)L * S;
    std::vector<float> obs(R * in_dim), action(R * 6), logp(R), adv(R), ret(R), value(R);
    std::vector<uint8_t> es(R);
    for (size_t i = 0; i < R; ++i) { logp[i] = -0.1f * (float)i; adv[i] = (float)((int)(i % 9) - 4); ret[i] = 1.0f; value[i] = (float)i; es[i] = (uint8_t)(i % 4 == 0); }
    for (size_t i = 0; i < obs.size(); ++i) obs[i] = (float)(i / (size_t)in_dim);
    const int dims[4] = {3, 1, 64, 5};
    std::vector<std::vector<float>> src((size_t)n_state), out((size_t)n_state);
    std::vector<float> mb_obs(M * in_dim), mb_action(M * 6), mb_logp(M), mb_adv(M), mb_ret(M), mb_value(M);
    std::vector<uint8_t> mb_start(M);
    std::vector<int32_t> index((size_t)S);
    std::vector<double> ws(glppo::BATCH_WS_BYTES / sizeof(double)), st(2);
    glgym_seq_batch_args a;
    std::memset(&a, 0, sizeof a);
    a.struct_size = (int32_t)sizeof a; a.T = T; a.B = B; a.L = L; a.S = S; a.offset = offset; a.in_dim = in_dim; a.n_state = n_state; a.seed = 77; a.draw_index = 1;
    for (int k = 0; k < n_state; ++k) {
        src[(size_t)k].resize(N * dims[k]);
        out[(size_t)k].resize((size_t)S * dims[k]);
        for (size_t i = 0; i < src[(size_t)k].size(); ++i) src[(size_t)k][i] = (float)(i / (size_t)dims[k]);
        a.state_dim[k] = dims[k]; a.state_src[k] = src[(size_t)k].data(); a.state_out[k] = out[(size_t)k].data();
    }
    a.obs = obs.data(); a.action = action.data(); a.logp = logp.data(); a.advantage = adv.data(); a.returns = ret.data(); a.value = value.data();
    a.episode_starts = es.data(); a.mb_obs = mb_obs.data(); a.mb_action = mb_action.data(); a.mb_logp = mb_logp.data(); a.mb_adv = mb_adv.data();
    a.mb_ret = mb_ret.data(); a.mb_value = mb_value.data(); a.mb_start = mb_start.data(); a.mb_index = index.data();
    if (stats) { a.adv_stats = st.data(); a.workspace = ws.data(); a.workspace_bytes = (int64_t)glppo::BATCH_WS_BYTES; }
    lstmhost_seq_batch(&a);
    for (int s = 0; s < S; ++s) {
        const int q = index[(size_t)s];
        EXPECT(q >= 0 && (size_t)q < N);
        for (int l = 0; l < L; ++l) {
            const size_t row = ((size_t)(q / B) * L + l) * B + q % B, m = (size_t)l * S + s;
            EXPECT(mb_value[m] == (float)row && mb_obs[m * in_dim] == (float)row && mb_start[m] == es[row]);
        }
        for (int k = 0; k < n_state; ++k) EXPECT(out[(size_t)k][(size_t)s * dims[k]] == (float)q);
    }
    if (stats) EXPECT(std::isfinite(st[0]) && st[1] >= 0.0);
}

}  // namespace

int main()
{
    EXPECT(lstmhost_sizeof(0) > 0 && lstmhost_sizeof(1) > 0 && lstmhost_sizeof(2) > 0);
    for (int M : {1, 63, 65, 257})
        for (int H : {1, 3, 64, 65})
            for (int kind : {-1, 0, 1, 2}) {
                drive_cell(M, H, kind, true, true);
                drive_cell(M, H, kind, M % 2 == 0, false);
            }
    for (int in_dim : {1, 23, 24})
        for (int L : {1, 2, 5}) {
            drive_seq(L, 1, L, 1, 0, in_dim, 0, false);
            drive_seq(3 * L, 3, L, 9, 0, in_dim, 2, true);
            drive_seq(3 * L, 8, L, 7, 17, in_dim, 4, true);
            drive_seq(L, 300, L, 257, 43, in_dim, 4, true);
        }
    std::printf(failures ? "lstmhost FAILED (%d)\n" : "lstmhost ok\n", failures);
    return failures ? 1 : 0;
}
#endif
