// glgym_sac.hip -- soft actor-critic on the device (include/glgym.h glgym_sac_rows, glgym_sac_rows_grad, glgym_sac_batch, glgym_sac_loss,
// glgym_polyak), kernels and C entry points: the tanh-squashed Gaussian between the actor's outputs and the env-step or the critics, its
// reparameterised backward pass, seeded sampling with replacement from a slot-major replay ring, the critic and actor loss stages with
// their gradients, and the Polyak update of the target critics.  The scalar logic and the order of every sum are gl_sac.hpp's
// (instantiated on the host by tests/sachost/sachost.cpp); the networks, autograd through them and the optimisers are the caller's, in torch.
//
// sac_rows / sac_rows_grad: lane = row, 256 per block, everything in registers, no LDS, no barrier; the observation copy is the block's
// own 256 rows, one contiguous span.  sac_batch: block = 256 positions per chunk, grid-stride over chunks; a lane draws its own position
// once, leaves the two source rows in LDS and copies the row's scalars; the chunk's observation, next-observation and action rows are then
// contiguous output spans written with lane stride 1 (glgym_ppo.hip's copy).  sac_loss: lane = row, grid-stride over chunks, LDS only to
// combine the four wavefronts; partials to the caller's workspace by plain stores and a one-block finishing launch in block order.
// polyak: blockIdx.y = tensor, grid-stride over its elements, one dword per access.
#include <cmath>
#include <string>

#include "glgym_internal.h"

#include "gl_sac.hpp"

namespace {

using glsac::BLOCK;
using glsac::N_SUM;
using glsac::N_WAVE;
using glsac::WAVE;
constexpr int NU = GLGYM_NU;

// grid = ceil(M / 256), lane = row
__global__ __launch_bounds__(BLOCK) void sac_rows_kernel(glgym_sac_rows_args a, float sigma)
{
    const int64_t r0 = (int64_t)blockIdx.x * BLOCK;
    const int64_t r64 = r0 + threadIdx.x;
    if (a.obs_out) {
        const int64_t n_row = a.M - r0 < BLOCK ? a.M - r0 : BLOCK;
        const size_t base = (size_t)r0 * (size_t)a.in_dim;
        const int n = (int)n_row * a.in_dim;                           // <= 256 * 1024
        for (int i = threadIdx.x; i < n; i += BLOCK) a.obs_out[base + i] = a.obs[base + i];
    }
    if (r64 >= a.M) return;
    const size_t r = (size_t)r64;
    const uint32_t key = (uint32_t)((uint64_t)a.row0 + (uint64_t)r64);
    const uint64_t D = a.draw_index + (a.draw_base ? *a.draw_base : 0ull);
    float act[NU], e2[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) e2[j] = 0.0f;
    if (sigma > 0.0f && !a.uniform) glsac::noise(key, (uint32_t)a.step, 2u, D, a.seed, e2);
    if (a.uniform) {
        glsac::uniform(key, (uint32_t)a.step, D, a.seed, act);
    } else {
        float e[NU], ls[NU], sd[NU], l[NU];
        if (a.deterministic) {
#pragma unroll
            for (int j = 0; j < NU; ++j) e[j] = 0.0f;
        } else {
            glsac::noise(key, (uint32_t)a.step, 0u, D, a.seed, e);
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            ls[j] = glsac::clamp_ls(a.log_std_in[r * NU + j]);
            sd[j] = glsac::std_of(ls[j]);
            act[j] = glsac::tanh_of(glsac::u_of(a.mean_in[r * NU + j], sd[j], e[j]));
            l[j] = glsac::log_of(glsac::c_of(act[j]));
        }
        if (a.logp) a.logp[r] = glsac::logp_of(e, ls, l);
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            if (a.eps) a.eps[r * NU + j] = e[j];
            if (a.eps2) a.eps2[r * NU + j] = e2[j];
            if (a.std) a.std[r * NU + j] = sd[j];
            if (a.tanh) a.tanh[r * NU + j] = act[j];
            if (a.corr) a.corr[r * NU + j] = l[j];
        }
    }
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        const float env = glsac::env_of(act[j], a.uniform ? 0.0f : sigma, e2[j]);
        if (a.action) a.action[r * NU + j] = act[j];
        if (a.action_env) a.action_env[r * NU + j] = env;
        if (a.action_slot) a.action_slot[r * NU + j] = env;
    }
}

// grid = ceil(M / 256), lane = row
__global__ __launch_bounds__(BLOCK) void sac_rows_grad_kernel(glgym_sac_rows_grad_args a)
{
    const int64_t r64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (r64 >= a.M) return;
    const size_t r = (size_t)r64;
    const float gl = a.grad_logp[r];
#pragma unroll
    for (int j = 0; j < NU; ++j) {
        const size_t i = r * NU + j;
        float gm, gs;
        glsac::squash_grad(a.grad_action[i], gl, a.eps[i], a.std[i], a.tanh[i], a.log_std_in[i], &gm, &gs);
        a.grad_mean[i] = gm;
        a.grad_log_std[i] = gs;
    }
}

// out[0 .. n_row * width) = rows src[0 .. n_row) of `in`, lane stride 1 on the output (glgym_ppo.hip's copy_rows)
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

// grid = n_blocks(M), block b: chunks b, b + nb, ...
__global__ __launch_bounds__(BLOCK) void sac_batch_kernel(glgym_sac_batch_args a, int nb)
{
    __shared__ uint32_t src[BLOCK], nxt[BLOCK];
    const int tid = threadIdx.x;
    const uint64_t D = a.draw_index + (a.draw_base ? *a.draw_base : 0ull);
    const uint64_t n = (uint64_t)a.n_valid * (uint64_t)a.B;
    const int64_t M = a.M;
    for (int64_t k = blockIdx.x; k * BLOCK < M; k += nb) {
        const int64_t m0 = k * BLOCK;
        const int n_row = (int)(M - m0 < BLOCK ? M - m0 : BLOCK);
        if (tid < n_row) {
            const size_t m = (size_t)(m0 + tid);
            uint32_t row, next_row;
            glsac::ring_rows(glsac::sample_index((uint32_t)m, n, D, a.seed), a.S, a.B, a.head, &row, &next_row);
            src[tid] = row;
            nxt[tid] = next_row;
            a.mb_reward[m] = a.reward[row];
            a.mb_done[m] = a.done[row];
            if (a.index_out) a.index_out[m] = (int64_t)row;
        }
        __syncthreads();
        copy_rows(a.mb_obs + (size_t)m0 * (size_t)a.in_dim, a.obs, a.in_dim, n_row, src);
        copy_rows(a.mb_next_obs + (size_t)m0 * (size_t)a.in_dim, a.obs, a.in_dim, n_row, nxt);
        copy_rows(a.mb_action + (size_t)m0 * NU, a.action, NU, n_row, src);
        __syncthreads();                                               // src and nxt are the next chunk's
    }
}

// grid = n_blocks(M), lane = row
__global__ __launch_bounds__(BLOCK) void sac_loss_kernel(glgym_sac_loss_args a, glsac::Hyper hy, int nb)
{
    __shared__ double part[N_WAVE][N_SUM];
    const int tid = threadIdx.x;
    const int64_t M = a.M;
    const float alpha = *a.alpha;
    glsac::Sums acc;
    glsac::sums_init(acc);
    for (int64_t k = blockIdx.x; k * BLOCK < M; k += nb) {
        const int64_t r64 = k * BLOCK + tid;
        if (r64 >= M) continue;
        const size_t r = (size_t)r64;
        if (a.stage == 0) {
            glsac::CriticRow o;
            glsac::critic_row(hy, alpha, a.q1[r], a.q2[r], a.q1_next[r], a.q2_next[r], a.logp[r], a.reward[r], a.done[r], o, acc);
            a.grad_q1[r] = o.g1;
            a.grad_q2[r] = o.g2;
            if (a.target_out) a.target_out[r] = o.y;
        } else {
            glsac::ActorRow o;
            glsac::actor_row(hy, alpha, a.q1[r], a.q2[r], a.logp[r], o, acc);
            a.grad_q1[r] = o.g1;
            a.grad_q2[r] = o.g2;
            a.grad_logp[r] = hy.w * alpha;
        }
    }
#pragma unroll
    for (int q = 0; q < N_SUM; ++q) {
        double v = acc.s[q];
        for (int m = WAVE / 2; m > 0; m >>= 1) v = v + __shfl_xor(v, m, WAVE);
        if ((tid & (WAVE - 1)) == 0) part[tid / WAVE][q] = v;
    }
    __syncthreads();
    if (tid < N_SUM) {
        double t = part[0][tid];
        for (int w = 1; w < N_WAVE; ++w) t = t + part[w][tid];
        a.workspace[(size_t)blockIdx.x * N_SUM + tid] = t;
    }
}

// one block: the partials in block order (their loads parallel through LDS, their additions not), then the statistics
constexpr int FIN = 512;
__global__ __launch_bounds__(FIN) void sac_loss_finish_kernel(glgym_sac_loss_args a, int nb)
{
    __shared__ double tile[N_SUM][FIN];
    __shared__ double S[N_SUM];
    const int tid = threadIdx.x;
    double t = 0.0;
    for (int base = 0; base < nb; base += FIN) {
        const int cnt = nb - base < FIN ? nb - base : FIN;
        if (tid < cnt) {
#pragma unroll
            for (int q = 0; q < N_SUM; ++q) tile[q][tid] = a.workspace[(size_t)(base + tid) * N_SUM + q];
        }
        __syncthreads();
        if (tid < N_SUM) {
            int i = 0;
            if (base == 0) { t = tile[tid][0]; i = 1; }
            for (; i < cnt; ++i) t = t + tile[tid][i];
        }
        __syncthreads();
    }
    if (tid < N_SUM) S[tid] = t;
    __syncthreads();
    if (tid == 0) {
        double st[8];
        const float alpha = *a.alpha;
        if (a.stage == 0) {
            glsac::critic_stats(S, a.M, alpha, st);
        } else {
            float g;
            glsac::actor_stats(S, a.M, alpha, *a.log_alpha, st, &g);
            if (a.grad_log_alpha) *a.grad_log_alpha = g;
        }
        for (int q = 0; q < 8; ++q) a.stats[q] = st[q];
    }
}

// grid = (blocks over the largest tensor, n), blockIdx.y = tensor
__global__ __launch_bounds__(BLOCK) void polyak_kernel(glgym_polyak_args a, float tau, float omt)
{
    const int k = blockIdx.y;
    const int64_t cnt = a.count[k];
    float* t = a.dst[k];
    const float* s = a.src[k];
    const int64_t stride = (int64_t)gridDim.x * BLOCK;
    for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < cnt; i += stride) t[i] = glsac::polyak(t[i], s[i], tau, omt);
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

bool flag(int32_t v) { return v == 0 || v == 1; }

}  // namespace

extern "C" {

int glgym_sac_rows(glgym_handle h, const glgym_sac_rows_args* a, void* stream)
{
    if (!a) return refuse("glgym_sac_rows: null arguments");
    if (!plan_size_ok("glgym_sac_rows", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->M < 1) return refuse("glgym_sac_rows: M < 1");
    if (a->M > INT32_MAX - (BLOCK - 1)) return refuse("glgym_sac_rows: more than 2^31 - 256 rows");
    if (a->step < 0 || a->step >= (1 << 30)) return refuse("glgym_sac_rows: step outside 0 .. 2^30 - 1");
    if (a->row0 < 0 || a->row0 + (int64_t)a->M > ((int64_t)1 << 32)) return refuse("glgym_sac_rows: row0 < 0 or row0 + M > 2^32");
    if (!flag(a->deterministic) || !flag(a->uniform)) return refuse("glgym_sac_rows: deterministic and uniform must be 0 or 1");
    if (a->deterministic && a->uniform) return refuse("glgym_sac_rows: deterministic and uniform are both set");
    if (!(a->action_noise_sigma >= 0.0) || !std::isfinite(a->action_noise_sigma))
        return refuse("glgym_sac_rows: action_noise_sigma negative or not finite");
    if (!a->obs_out && !a->action && !a->action_env && !a->action_slot && !a->logp && !a->eps && !a->eps2 && !a->std && !a->tanh && !a->corr)
        return refuse("glgym_sac_rows: no output");
    if (a->uniform) {
        if (a->logp || a->eps || a->eps2 || a->std || a->tanh || a->corr)
            return refuse("glgym_sac_rows: uniform with a logp, eps, eps2, std, tanh or corr output");
    } else if (!a->mean_in || !a->log_std_in) {
        return refuse("glgym_sac_rows: null mean_in or log_std_in");
    }
    const size_t M = (size_t)a->M, f = sizeof(float);
    size_t obs_bytes = 0;
    if (a->obs_out) {
        if (a->in_dim < 1 || a->in_dim > glsac::MAX_IN) return refuse("glgym_sac_rows: in_dim outside 1..1024");
        if (!a->obs) return refuse("glgym_sac_rows: null obs (obs_out copies it)");
        obs_bytes = M * (size_t)a->in_dim * f;
    }
    const Span in[] = {{a->uniform ? nullptr : a->mean_in, M * NU * f}, {a->uniform ? nullptr : a->log_std_in, M * NU * f},
                       {a->obs_out ? a->obs : nullptr, obs_bytes}, {a->draw_base, sizeof(uint64_t)}};
    const Span out[] = {{a->obs_out, obs_bytes}, {a->action, M * NU * f}, {a->action_env, M * NU * f}, {a->action_slot, M * NU * f},
                        {a->logp, M * f}, {a->eps, M * NU * f}, {a->eps2, M * NU * f}, {a->std, M * NU * f}, {a->tanh, M * NU * f}, {a->corr, M * NU * f}};
    switch (overlap_kind(in, out)) {
        case 1: return refuse("glgym_sac_rows: an output overlaps an input");
        case 2: return refuse("glgym_sac_rows: an output overlaps another output");
    }
    if (!h) return refuse("glgym_sac_rows: null handle");
    DeviceGuard dev_guard(h);
    hipLaunchKernelGGL(sac_rows_kernel, dim3((unsigned)(((int64_t)a->M + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, *a,
                       (float)a->action_noise_sigma);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_sac_rows_grad(glgym_handle h, const glgym_sac_rows_grad_args* a, void* stream)
{
    if (!a) return refuse("glgym_sac_rows_grad: null arguments");
    if (!plan_size_ok("glgym_sac_rows_grad", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->M < 1) return refuse("glgym_sac_rows_grad: M < 1");
    if (a->M > INT32_MAX - (BLOCK - 1)) return refuse("glgym_sac_rows_grad: more than 2^31 - 256 rows");
    if (!a->grad_action || !a->grad_logp || !a->eps || !a->std || !a->tanh || !a->log_std_in)
        return refuse("glgym_sac_rows_grad: null grad_action, grad_logp, eps, std, tanh or log_std_in");
    if (!a->grad_mean || !a->grad_log_std) return refuse("glgym_sac_rows_grad: null grad_mean or grad_log_std");
    const size_t n6 = (size_t)a->M * NU * sizeof(float);
    const Span in[] = {{a->grad_action, n6}, {a->grad_logp, (size_t)a->M * sizeof(float)}, {a->eps, n6}, {a->std, n6}, {a->tanh, n6},
                       {a->log_std_in, n6}};
    const Span out[] = {{a->grad_mean, n6}, {a->grad_log_std, n6}};
    switch (overlap_kind(in, out)) {
        case 1: return refuse("glgym_sac_rows_grad: an output overlaps an input");
        case 2: return refuse("glgym_sac_rows_grad: an output overlaps another output");
    }
    if (!h) return refuse("glgym_sac_rows_grad: null handle");
    DeviceGuard dev_guard(h);
    hipLaunchKernelGGL(sac_rows_grad_kernel, dim3((unsigned)(((int64_t)a->M + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)stream, *a);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_sac_batch(glgym_handle h, const glgym_sac_batch_args* a, void* stream)
{
    if (!a) return refuse("glgym_sac_batch: null arguments");
    if (!plan_size_ok("glgym_sac_batch", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->S < 2) return refuse("glgym_sac_batch: S < 2");
    if (a->B < 1) return refuse("glgym_sac_batch: B < 1");
    if ((int64_t)a->S * (int64_t)a->B > (int64_t)INT32_MAX) return refuse("glgym_sac_batch: S * B > 2^31 - 1");
    if (a->M < 1) return refuse("glgym_sac_batch: M < 1");
    if (a->M > INT32_MAX - (BLOCK - 1)) return refuse("glgym_sac_batch: more than 2^31 - 256 rows");
    if (a->in_dim < 1 || a->in_dim > glsac::MAX_IN) return refuse("glgym_sac_batch: in_dim outside 1..1024");
    if (a->head < 0 || a->head >= a->S) return refuse("glgym_sac_batch: head outside 0 .. S - 1");
    if (a->n_valid < 1) return refuse("glgym_sac_batch: n_valid < 1");
    if (a->n_valid >= a->S) return refuse("glgym_sac_batch: n_valid > S - 1 (a slot without a successor)");
    if (!a->obs || !a->action || !a->reward || !a->done) return refuse("glgym_sac_batch: null obs, action, reward or done");
    if (!a->mb_obs || !a->mb_next_obs || !a->mb_action || !a->mb_reward || !a->mb_done)
        return refuse("glgym_sac_batch: null mb_obs, mb_next_obs, mb_action, mb_reward or mb_done");
    const size_t N = (size_t)a->S * (size_t)a->B, M = (size_t)a->M, f = sizeof(float), d = (size_t)a->in_dim;
    const Span in[] = {{a->obs, N * d * f}, {a->action, N * NU * f}, {a->reward, N * f}, {a->done, N}, {a->draw_base, sizeof(uint64_t)}};
    const Span out[] = {{a->mb_obs, M * d * f}, {a->mb_next_obs, M * d * f}, {a->mb_action, M * NU * f}, {a->mb_reward, M * f}, {a->mb_done, M},
                        {a->index_out, M * sizeof(int64_t)}};
    switch (overlap_kind(in, out)) {
        case 1: return refuse("glgym_sac_batch: an output overlaps a source");
        case 2: return refuse("glgym_sac_batch: an output overlaps another output");
    }
    if (!h) return refuse("glgym_sac_batch: null handle");
    DeviceGuard dev_guard(h);
    const int nb = glsac::n_blocks(a->M);
    hipLaunchKernelGGL(sac_batch_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, *a, nb);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_sac_loss(glgym_handle h, const glgym_sac_loss_args* a, void* stream)
{
    if (!a) return refuse("glgym_sac_loss: null arguments");
    if (!plan_size_ok("glgym_sac_loss", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->M < 1) return refuse("glgym_sac_loss: M < 1");
    if (a->M > INT32_MAX - (BLOCK - 1)) return refuse("glgym_sac_loss: more than 2^31 - 256 rows");
    if (a->stage != 0 && a->stage != 1) return refuse("glgym_sac_loss: stage must be 0 (critic) or 1 (actor)");
    if (!a->q1 || !a->q2 || !a->logp || !a->alpha) return refuse("glgym_sac_loss: null q1, q2, logp or alpha");
    if (!a->grad_q1 || !a->grad_q2 || !a->stats) return refuse("glgym_sac_loss: null grad_q1, grad_q2 or stats");
    const bool critic = a->stage == 0;
    if (critic) {
        if (!(a->gamma >= 0.0 && a->gamma <= 1.0)) return refuse("glgym_sac_loss: gamma outside [0, 1] or not finite");
        if (!a->q1_next || !a->q2_next || !a->reward || !a->done) return refuse("glgym_sac_loss: critic stage with a null q1_next, q2_next, reward or done");
    } else {
        if (!std::isfinite(a->target_entropy)) return refuse("glgym_sac_loss: target_entropy not finite");
        if (!a->log_alpha || !a->grad_logp) return refuse("glgym_sac_loss: actor stage with a null log_alpha or grad_logp");
    }
    if (!a->workspace) return refuse("glgym_sac_loss: null workspace");
    if (a->workspace_bytes < (int64_t)glsac::LOSS_WS_BYTES) return refuse("glgym_sac_loss: workspace smaller than 40960 bytes");
    const size_t M = (size_t)a->M, f = sizeof(float);
    const Span in[] = {{a->q1, M * f}, {a->q2, M * f}, {a->logp, M * f}, {critic ? a->q1_next : nullptr, M * f},
                       {critic ? a->q2_next : nullptr, M * f}, {critic ? a->reward : nullptr, M * f}, {critic ? a->done : nullptr, M},
                       {a->alpha, f}, {critic ? nullptr : a->log_alpha, f}};
    const Span out[] = {{a->grad_q1, M * f}, {a->grad_q2, M * f}, {critic ? nullptr : a->grad_logp, M * f},
                        {critic ? a->target_out : nullptr, M * f}, {critic ? nullptr : a->grad_log_alpha, f}, {a->stats, 8 * sizeof(double)},
                        {a->workspace, glsac::LOSS_WS_BYTES}};
    switch (overlap_kind(in, out)) {
        case 1: return refuse("glgym_sac_loss: an output overlaps an input");
        case 2: return refuse("glgym_sac_loss: an output overlaps another output");
    }
    if (!h) return refuse("glgym_sac_loss: null handle");
    DeviceGuard dev_guard(h);
    const int nb = glsac::n_blocks(a->M);
    const glsac::Hyper hy = glsac::hyper(a->M, a->gamma, a->target_entropy);
    hipLaunchKernelGGL(sac_loss_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, *a, hy, nb);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(sac_loss_finish_kernel, dim3(1), dim3(FIN), 0, (hipStream_t)stream, *a, nb);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_polyak(glgym_handle h, const glgym_polyak_args* a, void* stream)
{
    if (!a) return refuse("glgym_polyak: null arguments");
    if (!plan_size_ok("glgym_polyak", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->n < 1) return refuse("glgym_polyak: n < 1");
    if (a->n > glsac::MAX_TENSORS) return refuse("glgym_polyak: more than 64 tensors");
    if (!a->dst || !a->src || !a->count) return refuse("glgym_polyak: null dst, src or count");
    if (!(a->tau >= 0.0 && a->tau <= 1.0)) return refuse("glgym_polyak: tau outside [0, 1] or not finite");
    if (a->max_count < 0) return refuse("glgym_polyak: max_count < 0");
    if (!h) return refuse("glgym_polyak: null handle");
    DeviceGuard dev_guard(h);
    int64_t gx = (a->max_count + BLOCK - 1) / BLOCK;
    gx = gx < 1 ? 1 : gx > glsac::MAX_BLOCKS ? glsac::MAX_BLOCKS : gx;
    const float tau = (float)a->tau;
    hipLaunchKernelGGL(polyak_kernel, dim3((unsigned)gx, (unsigned)a->n), dim3(BLOCK), 0, (hipStream_t)stream, *a, tau, 1.0f - tau);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

}  // extern "C"
