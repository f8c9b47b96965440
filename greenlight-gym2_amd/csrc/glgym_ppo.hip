// glgym_ppo.hip -- the PPO update on the device (include/glgym.h glgym_ppo_batch, glgym_ppo_loss), kernels and C entry points: one
// minibatch of a seeded permutation gathered from a collector's flat buffer, and the clipped-surrogate loss with its gradients with respect
// to the heads' outputs.  The scalar logic and the order of every sum are gl_ppo.hpp's (instantiated on the host by
// tests/ppohost/ppohost.cpp); the heads, their backward pass and the optimiser are the caller's, in torch.
//
// ppo_batch: block = 256 positions of the permutation per chunk, grid-stride over chunks.  A lane walks the permutation of its own position
// once, leaves the source row in LDS and copies the row's four scalars; the chunk's observation and action rows are then ONE contiguous
// output span, written with lane stride 1 (the read side follows the staged source rows, row segment by row segment).
// ppo_loss: lane = row, 256 per block, grid-stride over chunks; six means and six actions per lane as ac_rows_kernel reads them,
// everything else in registers; LDS only to combine the four wavefronts' partial sums.  Both reduce as gl_ppo.hpp states: lane, butterfly,
// wavefronts in index order, partials to the caller's workspace by plain stores, and a one-block finishing launch in block order (its
// loads of the partials are parallel, through LDS; its additions are not).
#include <cmath>
#include <string>

#include "glgym_internal.h"

#include "gl_ppo.hpp"

namespace {

using glppo::BLOCK;
using glppo::N_ADV;
using glppo::N_SUM;
using glppo::N_WAVE;
using glppo::WAVE;
constexpr int NU = GLGYM_NU;

// out[0 .. n_row * width) = rows src[0 .. n_row) of `in`, lane stride 1 on the output; (r, c) follow i without a division per element.
// COPY_DEPTH independent loads are in flight per lane before the first store: the gather is bound by latency, not by issue.
constexpr int COPY_DEPTH = 8;
__device__ __forceinline__ void copy_rows(float* out, const float* in, int width, int n_row, const uint32_t* src)
{
    const int n = n_row * width;                                       // <= 256 * 1024
    const int dq = BLOCK / width, dr = BLOCK - dq * width;             // dr < width
    int r = (int)threadIdx.x / width, c = (int)threadIdx.x - r * width;
    for (int i0 = threadIdx.x; i0 < n; i0 += BLOCK * COPY_DEPTH) {
        float v[COPY_DEPTH];
#pragma unroll
        for (int u = 0; u < COPY_DEPTH; ++u) {
            if (i0 + u * BLOCK < n) v[u] = in[(size_t)src[r] * (size_t)width + c];
            r += dq;
            c += dr;
            if (c >= width) { c -= width; ++r; }
        }
#pragma unroll
        for (int u = 0; u < COPY_DEPTH; ++u)
            if (i0 + u * BLOCK < n) out[i0 + u * BLOCK] = v[u];
    }
}

// The finishing launches: one block of FIN lanes.  The partials ws[block][NS] come in with one coalesced load per lane and slot into LDS,
// FIN blocks at a time; lane q < NS then adds slot q in block order from block 0 -- the order is the header's, only the loads are parallel.
constexpr int FIN = 512;
template <int NS, bool LOSS> __device__ __forceinline__ void sum_partials(const double* ws, int nb, double (*tile)[FIN], double* S)
{
    const int tid = threadIdx.x;
    double t = 0.0;
    for (int base = 0; base < nb; base += FIN) {
        const int cnt = nb - base < FIN ? nb - base : FIN;
        if (tid < cnt) {
#pragma unroll
            for (int q = 0; q < NS; ++q) tile[q][tid] = ws[(size_t)(base + tid) * NS + q];
        }
        __syncthreads();
        if (tid < NS) {
            int i = 0;
            if (base == 0) { t = tile[tid][0]; i = 1; }
            for (; i < cnt; ++i) t = LOSS ? glppo::combine(tid, t, tile[tid][i]) : t + tile[tid][i];
        }
        __syncthreads();
    }
    if (tid < NS) S[tid] = t;
    __syncthreads();
}

// grid = n_blocks(M), block b: chunks b, b + nb, ...
__global__ __launch_bounds__(BLOCK) void ppo_batch_kernel(glgym_ppo_batch_args a, int nb, int half)
{
    __shared__ uint32_t src[BLOCK];
    __shared__ double part[N_WAVE][N_ADV];
    const int tid = threadIdx.x;
    const uint64_t D = a.draw_index + (a.draw_base ? *a.draw_base : 0ull);
    const int64_t M = a.M;
    double s[N_ADV] = {0.0, 0.0};
    for (int64_t k = blockIdx.x; k * BLOCK < M; k += nb) {
        const int64_t m0 = k * BLOCK;
        const int n_row = (int)(M - m0 < BLOCK ? M - m0 : BLOCK);
        if (tid < n_row) {
            const size_t m = (size_t)(m0 + tid);
            const uint32_t i = glppo::perm((uint32_t)((int64_t)a.offset + m0 + tid), (uint32_t)a.N, half, D, a.seed);
            src[tid] = i;
            const float adv = a.advantage[i];
            a.mb_logp[m] = a.logp[i];
            a.mb_adv[m] = adv;
            a.mb_ret[m] = a.returns[i];
            a.mb_value[m] = a.value[i];
            if (a.mb_index) a.mb_index[m] = (int32_t)i;
            double t[N_ADV];
            glppo::adv_terms(adv, t);
            for (int q = 0; q < N_ADV; ++q) s[q] = s[q] + t[q];
        }
        __syncthreads();
        copy_rows(a.mb_obs + (size_t)m0 * (size_t)a.in_dim, a.obs, a.in_dim, n_row, src);
        copy_rows(a.mb_action + (size_t)m0 * NU, a.action, NU, n_row, src);
        __syncthreads();                                               // src is the next chunk's
    }
    if (!a.adv_stats) return;
    for (int q = 0; q < N_ADV; ++q) {
        double v = s[q];
        for (int m = WAVE / 2; m > 0; m >>= 1) v = v + __shfl_xor(v, m, WAVE);
        if ((tid & (WAVE - 1)) == 0) part[tid / WAVE][q] = v;
    }
    __syncthreads();
    if (tid < N_ADV) {
        double t = part[0][tid];
        for (int w = 1; w < N_WAVE; ++w) t = t + part[w][tid];
        a.workspace[(size_t)blockIdx.x * N_ADV + tid] = t;
    }
}

// one block: the partials in block order, then the statistics
__global__ __launch_bounds__(FIN) void ppo_batch_finish_kernel(const double* ws, int nb, int M, double* adv_stats)
{
    __shared__ double tile[N_ADV][FIN];
    __shared__ double S[N_ADV];
    sum_partials<N_ADV, false>(ws, nb, tile, S);
    if (threadIdx.x == 0) glppo::adv_stats_of(S[0], S[1], M, adv_stats);
}

// grid = n_blocks(M), lane = row
__global__ __launch_bounds__(BLOCK) void ppo_loss_kernel(glgym_ppo_loss_args a, glppo::Hyper hy, int nb)
{
    __shared__ double part[N_WAVE][N_SUM];
    const int tid = threadIdx.x;
    const int64_t M = a.M;
    float ls[NU], is[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) { ls[j] = a.log_std[j]; is[j] = a.inv_std[j]; }
    const glppo::Norm nrm = glppo::norm_of(a.adv_stats);
    glppo::Sums acc;
    glppo::sums_init(acc);
    for (int64_t k = blockIdx.x; k * BLOCK < M; k += nb) {
        const int64_t r64 = k * BLOCK + tid;
        if (r64 >= M) continue;
        const size_t r = (size_t)r64;
        float mean[NU], act[NU], z[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) { mean[j] = a.mean[r * NU + j]; act[j] = a.mb_action[r * NU + j]; }
        const float old_logp = a.mb_logp[r];
        const float logp = glppo::logp_of(mean, act, is, ls, z);
        const float ratio = glppo::ratio_of(logp, old_logp);
        glppo::Row o;
        glppo::finish_row(hy, nrm, z, is, logp, old_logp, ratio, a.mb_adv[r], a.value[r], hy.vclip ? a.mb_value[r] : 0.0f, a.mb_ret[r], o);
#pragma unroll
        for (int j = 0; j < NU; ++j) a.grad_mean[r * NU + j] = o.grad_mean[j];
        a.grad_value[r] = o.grad_value;
        if (a.ratio_out) a.ratio_out[r] = ratio;
        if (a.logp_out) a.logp_out[r] = logp;
        glppo::sums_add(acc, o, ratio);
    }
#pragma unroll
    for (int q = 0; q < N_SUM; ++q) {
        double v = acc.s[q];
        for (int m = WAVE / 2; m > 0; m >>= 1) v = glppo::combine(q, v, __shfl_xor(v, m, WAVE));
        if ((tid & (WAVE - 1)) == 0) part[tid / WAVE][q] = v;
    }
    __syncthreads();
    if (tid < N_SUM) {
        double t = part[0][tid];
        for (int w = 1; w < N_WAVE; ++w) t = glppo::combine(tid, t, part[w][tid]);
        a.workspace[(size_t)blockIdx.x * N_SUM + tid] = t;
    }
}

__global__ __launch_bounds__(FIN) void ppo_loss_finish_kernel(glgym_ppo_loss_args a, glppo::Hyper hy, int nb)
{
    __shared__ double tile[N_SUM][FIN];
    __shared__ double S[N_SUM];
    sum_partials<N_SUM, true>(a.workspace, nb, tile, S);
    if (threadIdx.x == 0) {
        float ls[NU], g[NU];
        double st[8];
        for (int j = 0; j < NU; ++j) ls[j] = a.log_std[j];
        glppo::loss_stats(S, a.M, hy, ls, st, g);
        for (int q = 0; q < 8; ++q) a.stats[q] = st[q];
        for (int j = 0; j < NU; ++j) a.grad_log_std[j] = g[j];
    }
}

struct Span {
    const void* p;
    size_t n;
};

// [p, p + n) and [q, q + m) share a byte
bool overlaps(const Span& x, const Span& y)
{
    if (!x.p || !y.p) return false;
    const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
    return a < b + y.n && b < a + x.n;
}

// an output overlaps an input, or another output
template <size_t NI, size_t NO> int overlap_kind(const Span (&in)[NI], const Span (&out)[NO])
{
    for (size_t o = 0; o < NO; ++o)
        for (size_t i = 0; i < NI; ++i)
            if (overlaps(out[o], in[i])) return 1;
    for (size_t o = 0; o < NO; ++o)
        for (size_t p = o + 1; p < NO; ++p)
            if (overlaps(out[o], out[p])) return 2;
    return 0;
}

}  // namespace

extern "C" {

int glgym_ppo_batch(glgym_handle h, const glgym_ppo_batch_args* a, void* stream)
{
    if (!a) return refuse("glgym_ppo_batch: null arguments");
    if (!plan_size_ok("glgym_ppo_batch", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->N < 1) return refuse("glgym_ppo_batch: N < 1");
    if (a->N > INT32_MAX - (BLOCK - 1)) return refuse("glgym_ppo_batch: more than 2^31 - 256 transitions");
    if (a->M < 1) return refuse("glgym_ppo_batch: M < 1");
    if (a->offset < 0) return refuse("glgym_ppo_batch: offset < 0");
    if ((int64_t)a->offset + (int64_t)a->M > (int64_t)a->N) return refuse("glgym_ppo_batch: offset + M > N");
    if (a->in_dim < 1 || a->in_dim > glppo::MAX_IN) return refuse("glgym_ppo_batch: in_dim outside 1..1024");
    if (!a->obs || !a->action || !a->logp || !a->advantage || !a->returns || !a->value)
        return refuse("glgym_ppo_batch: null obs, action, logp, advantage, returns or value");
    if (!a->mb_obs || !a->mb_action || !a->mb_logp || !a->mb_adv || !a->mb_ret || !a->mb_value)
        return refuse("glgym_ppo_batch: null mb_obs, mb_action, mb_logp, mb_adv, mb_ret or mb_value");
    if (a->adv_stats) {
        if (a->M < 2) return refuse("glgym_ppo_batch: adv_stats with M < 2 (the unbiased deviation divides by M - 1)");
        if (!a->workspace) return refuse("glgym_ppo_batch: adv_stats without a workspace");
        if (a->workspace_bytes < (int64_t)glppo::BATCH_WS_BYTES) return refuse("glgym_ppo_batch: workspace smaller than 16384 bytes");
    }
    const size_t N = (size_t)a->N, M = (size_t)a->M, f = sizeof(float), d = (size_t)a->in_dim;
    const Span in[] = {{a->obs, N * d * f}, {a->action, N * NU * f}, {a->logp, N * f}, {a->advantage, N * f}, {a->returns, N * f},
                       {a->value, N * f}, {a->draw_base, sizeof(uint64_t)}};
    const Span out[] = {{a->mb_obs, M * d * f}, {a->mb_action, M * NU * f}, {a->mb_logp, M * f}, {a->mb_adv, M * f}, {a->mb_ret, M * f},
                        {a->mb_value, M * f}, {a->mb_index, M * sizeof(int32_t)}, {a->adv_stats, 2 * sizeof(double)},
                        {a->adv_stats ? a->workspace : nullptr, glppo::BATCH_WS_BYTES}};
    switch (overlap_kind(in, out)) {
        case 1: return refuse("glgym_ppo_batch: an output overlaps a source");
        case 2: return refuse("glgym_ppo_batch: an output overlaps another output");
    }
    if (!h) return refuse("glgym_ppo_batch: null handle");
    DeviceGuard dev_guard(h);
    const int nb = glppo::n_blocks(a->M);
    hipLaunchKernelGGL(ppo_batch_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, *a, nb, glppo::half_bits((uint32_t)a->N));
    HIPCHK(hipGetLastError());
    if (a->adv_stats) {
        hipLaunchKernelGGL(ppo_batch_finish_kernel, dim3(1), dim3(FIN), 0, (hipStream_t)stream, a->workspace, nb, a->M, a->adv_stats);
        HIPCHK(hipGetLastError());
    }
    return GLGYM_OK;
}

int glgym_ppo_loss(glgym_handle h, const glgym_ppo_loss_args* a, void* stream)
{
    if (!a) return refuse("glgym_ppo_loss: null arguments");
    if (!plan_size_ok("glgym_ppo_loss", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->M < 1) return refuse("glgym_ppo_loss: M < 1");
    if (a->M > INT32_MAX - (BLOCK - 1)) return refuse("glgym_ppo_loss: more than 2^31 - 256 rows");
    if (!(a->clip_range > 0.0) || !std::isfinite(a->clip_range)) return refuse("glgym_ppo_loss: clip_range not > 0 or not finite");
    if (!std::isfinite(a->clip_range_vf)) return refuse("glgym_ppo_loss: clip_range_vf not finite");
    if (!std::isfinite(a->vf_coef)) return refuse("glgym_ppo_loss: vf_coef not finite");
    if (!std::isfinite(a->ent_coef)) return refuse("glgym_ppo_loss: ent_coef not finite");
    if (a->clip_range_vf > 0.0 && !a->mb_value) return refuse("glgym_ppo_loss: clip_range_vf > 0 without mb_value");
    if (!a->mean || !a->value || !a->log_std || !a->inv_std || !a->mb_action || !a->mb_logp || !a->mb_adv || !a->mb_ret)
        return refuse("glgym_ppo_loss: null mean, value, log_std, inv_std, mb_action, mb_logp, mb_adv or mb_ret");
    if (!a->grad_mean || !a->grad_value || !a->grad_log_std || !a->stats)
        return refuse("glgym_ppo_loss: null grad_mean, grad_value, grad_log_std or stats");
    if (!a->workspace) return refuse("glgym_ppo_loss: null workspace");
    if (a->workspace_bytes < (int64_t)glppo::LOSS_WS_BYTES) return refuse("glgym_ppo_loss: workspace smaller than 90112 bytes");
    const size_t M = (size_t)a->M, f = sizeof(float);
    const Span in[] = {{a->mean, M * NU * f}, {a->value, M * f}, {a->log_std, NU * f}, {a->inv_std, NU * f}, {a->mb_action, M * NU * f},
                       {a->mb_logp, M * f}, {a->mb_adv, M * f}, {a->mb_ret, M * f}, {a->mb_value, M * f}, {a->adv_stats, 2 * sizeof(double)}};
    const Span out[] = {{a->grad_mean, M * NU * f}, {a->grad_value, M * f}, {a->grad_log_std, NU * f}, {a->stats, 8 * sizeof(double)},
                        {a->ratio_out, M * f}, {a->logp_out, M * f}, {a->workspace, glppo::LOSS_WS_BYTES}};
    switch (overlap_kind(in, out)) {
        case 1: return refuse("glgym_ppo_loss: an output overlaps an input");
        case 2: return refuse("glgym_ppo_loss: an output overlaps another output");
    }
    if (!h) return refuse("glgym_ppo_loss: null handle");
    DeviceGuard dev_guard(h);
    const int nb = glppo::n_blocks(a->M);
    const glppo::Hyper hy = glppo::hyper(a->M, a->clip_range, a->clip_range_vf, a->vf_coef, a->ent_coef);
    hipLaunchKernelGGL(ppo_loss_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, *a, hy, nb);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(ppo_loss_finish_kernel, dim3(1), dim3(FIN), 0, (hipStream_t)stream, *a, hy, nb);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

}  // extern "C"
