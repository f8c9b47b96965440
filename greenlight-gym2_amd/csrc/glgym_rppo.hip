// glgym_rppo.hip -- recurrent PPO on the device (include/glgym.h glgym_lstm_cell, glgym_lstm_cell_grad, glgym_seq_batch), kernels and C
// entry points: what lies between torch's two gate products of an LSTM step and its new state, the backward pass of that, and one minibatch
// of whole sequences gathered time-major from a collector's [T][B] buffer.  The scalar logic is gl_lstm.hpp's (instantiated on the host by
// tests/lstmhost/lstmhost.cpp); the permutation and the advantage statistics are gl_ppo.hpp's.
//
// lstm_cell / lstm_cell_grad: streaming kernels, one lane per (row, V consecutive units), V = 4 (one 16-byte access per gate plane) where
// H % 4 == 0 and every buffer is 16-byte aligned, else 1.  Consecutive lanes take consecutive units of a gate plane.  No LDS, no barrier;
// the grid is capped at 2048 blocks and strides.
// seq_batch: block = 256 sequences per chunk, grid-stride over chunks.  A lane walks the permutation of its own sequence once, leaves the
// sequence's first buffer row in LDS and copies the L steps' scalars; for every step l the chunk's observation and action rows are one
// contiguous span of the time-major output, written with lane stride 1.  The advantage statistics are two further launches over the
// gathered mb_adv in glgym_ppo_batch's own order.
#include <string>

#include "glgym_internal.h"

#include "gl_lstm.hpp"

namespace {

using glppo::N_ADV;
using glppo::N_WAVE;
using glppo::WAVE;
using glstm::BLOCK;
using glstm::N_ACT;
constexpr int NU = GLGYM_NU;

template <int V> struct Vec;
template <> struct Vec<1> {
    float v[1];
};
template <> struct alignas(16) Vec<4> {
    float v[4];
};

template <int V> __device__ __forceinline__ Vec<V> load(const float* p) { return *reinterpret_cast<const Vec<V>*>(p); }
template <int V> __device__ __forceinline__ void store(float* p, const Vec<V>& x) { *reinterpret_cast<Vec<V>*>(p) = x; }

// grid = n_blocks(M * H / V); lane e -> row e / (H / V), units V * (e % (H / V)) ..
template <int V> __global__ __launch_bounds__(BLOCK) void lstm_cell_kernel(glgym_lstm_cell_args a, uint32_t n_lane, uint32_t step)
{
    const uint32_t H = (uint32_t)a.H, HV = H / V;
    for (uint32_t e = blockIdx.x * BLOCK + threadIdx.x; e < n_lane; e += step) {
        const uint32_t row = e / HV, j = (e - row * HV) * V;
        const bool keep = !a.start || a.start[row] == 0;
        const size_t g0 = (size_t)row * 4 * H + j, s0 = (size_t)row * H + j;
        Vec<V> gx[4], gh[4], act[N_ACT], c, h;
#pragma unroll
        for (int k = 0; k < 4; ++k) gx[k] = load<V>(a.gx + g0 + (size_t)k * H);
#pragma unroll
        for (int k = 0; k < 4; ++k) gh[k] = load<V>(a.gh + g0 + (size_t)k * H);
        const Vec<V> cp = load<V>(a.c_prev + s0);
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const float x[4] = {gx[0].v[u], gx[1].v[u], gx[2].v[u], gx[3].v[u]}, y[4] = {gh[0].v[u], gh[1].v[u], gh[2].v[u], gh[3].v[u]};
            float t[N_ACT];
            glstm::forward(keep, x, y, cp.v[u], t, c.v[u], h.v[u]);
#pragma unroll
            for (int k = 0; k < N_ACT; ++k) act[k].v[u] = t[k];
        }
        store<V>(a.h + s0, h);
        store<V>(a.c + s0, c);
        if (a.act) {
            const size_t a0 = (size_t)row * N_ACT * H + j;
#pragma unroll
            for (int k = 0; k < N_ACT; ++k) store<V>(a.act + a0 + (size_t)k * H, act[k]);
        }
    }
}

template <int V> __global__ __launch_bounds__(BLOCK) void lstm_cell_grad_kernel(glgym_lstm_cell_grad_args a, uint32_t n_lane, uint32_t step)
{
    const uint32_t H = (uint32_t)a.H, HV = H / V;
    for (uint32_t e = blockIdx.x * BLOCK + threadIdx.x; e < n_lane; e += step) {
        const uint32_t row = e / HV, j = (e - row * HV) * V;
        const bool keep = !a.start || a.start[row] == 0;
        const size_t g0 = (size_t)row * 4 * H + j, s0 = (size_t)row * H + j, a0 = (size_t)row * N_ACT * H + j;
        Vec<V> act[N_ACT], dc, da[4], dg[4], dcp;
#pragma unroll
        for (int k = 0; k < N_ACT; ++k) act[k] = load<V>(a.act + a0 + (size_t)k * H);
        const Vec<V> dh = load<V>(a.dh + s0), cp = load<V>(a.c_prev + s0);
        if (a.dc) dc = load<V>(a.dc + s0);
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const float t[N_ACT] = {act[0].v[u], act[1].v[u], act[2].v[u], act[3].v[u], act[4].v[u]};
            float d[4];
            glstm::backward(keep, dh.v[u], a.dc ? dc.v[u] : 0.0f, t, cp.v[u], d, dcp.v[u]);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                da[k].v[u] = d[k];
                dg[k].v[u] = keep ? d[k] : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            store<V>(a.d_gx + g0 + (size_t)k * H, da[k]);
            store<V>(a.d_gh + g0 + (size_t)k * H, dg[k]);
        }
        store<V>(a.d_c_prev + s0, dcp);
    }
}

// out[0 .. n_row * width) = rows src[0 .. n_row) + row_off of `in`, lane stride 1 on the output (glgym_ppo.hip copy_rows, with the step's
// row offset): COPY_DEPTH independent loads are in flight per lane before the first store.
constexpr int COPY_DEPTH = 8;
__device__ __forceinline__ void copy_rows(float* out, const float* in, int width, int n_row, const uint32_t* src, uint32_t row_off)
{
    const int n = n_row * width;                                       // <= 256 * 1024
    const int dq = BLOCK / width, dr = BLOCK - dq * width;             // dr < width
    int r = (int)threadIdx.x / width, c = (int)threadIdx.x - r * width;
    for (int i0 = threadIdx.x; i0 < n; i0 += BLOCK * COPY_DEPTH) {
        float v[COPY_DEPTH];
#pragma unroll
        for (int u = 0; u < COPY_DEPTH; ++u) {
            if (i0 + u * BLOCK < n) v[u] = in[(size_t)(src[r] + row_off) * (size_t)width + c];
            r += dq;
            c += dr;
            if (c >= width) { c -= width; ++r; }
        }
#pragma unroll
        for (int u = 0; u < COPY_DEPTH; ++u)
            if (i0 + u * BLOCK < n) out[i0 + u * BLOCK] = v[u];
    }
}

// grid = glppo::n_blocks(S), block b: chunks of 256 sequences b, b + nb, ...
__global__ __launch_bounds__(BLOCK) void seq_batch_kernel(glgym_seq_batch_args a, int nb, int half, uint32_t N)
{
    __shared__ uint32_t seq[BLOCK];                                    // the sequence: a row of the state sources
    __shared__ uint32_t row0[BLOCK];                                   // its first buffer row
    const int tid = threadIdx.x;
    const uint64_t D = a.draw_index + (a.draw_base ? *a.draw_base : 0ull);
    const int64_t S = a.S;
    const uint32_t B = (uint32_t)a.B, L = (uint32_t)a.L;
    for (int64_t k = blockIdx.x; k * BLOCK < S; k += nb) {
        const int64_t m0 = k * BLOCK;
        const int n_row = (int)(S - m0 < BLOCK ? S - m0 : BLOCK);
        if (tid < n_row) {
            const uint32_t q = glppo::perm((uint32_t)((int64_t)a.offset + m0 + tid), N, half, D, a.seed);
            const uint32_t r0 = glstm::first_row(q, B, L);
            seq[tid] = q;
            row0[tid] = r0;
            if (a.mb_index) a.mb_index[m0 + tid] = (int32_t)q;
            for (uint32_t l = 0; l < L; ++l) {
                const size_t i = (size_t)r0 + (size_t)l * B, m = (size_t)l * (size_t)S + (size_t)(m0 + tid);
                a.mb_logp[m] = a.logp[i];
                a.mb_adv[m] = a.advantage[i];
                a.mb_ret[m] = a.returns[i];
                a.mb_value[m] = a.value[i];
                a.mb_start[m] = a.episode_starts[i];
            }
        }
        __syncthreads();
        for (uint32_t l = 0; l < L; ++l) {
            const size_t m = (size_t)l * (size_t)S + (size_t)m0;
            copy_rows(a.mb_obs + m * (size_t)a.in_dim, a.obs, a.in_dim, n_row, row0, l * B);
            copy_rows(a.mb_action + m * NU, a.action, NU, n_row, row0, l * B);
        }
        for (int s = 0; s < a.n_state; ++s)
            copy_rows(a.state_out[s] + (size_t)m0 * (size_t)a.state_dim[s], a.state_src[s], a.state_dim[s], n_row, seq, 0u);
        __syncthreads();                                               // seq and row0 are the next chunk's
    }
}

// the advantage statistics of the gathered rows, glgym_ppo_batch's reduction over M = L * S flat rows: grid = glppo::n_blocks(M)
__global__ __launch_bounds__(BLOCK) void seq_adv_kernel(const float* mb_adv, int64_t M, int nb, double* ws)
{
    __shared__ double part[N_WAVE][N_ADV];
    const int tid = threadIdx.x;
    double s[N_ADV] = {0.0, 0.0};
    for (int64_t k = blockIdx.x; k * BLOCK < M; k += nb) {
        const int64_t m = k * BLOCK + tid;
        if (m < M) {
            double t[N_ADV];
            glppo::adv_terms(mb_adv[m], t);
            for (int q = 0; q < N_ADV; ++q) s[q] = s[q] + t[q];
        }
    }
    for (int q = 0; q < N_ADV; ++q) {
        double v = s[q];
        for (int m = WAVE / 2; m > 0; m >>= 1) v = v + __shfl_xor(v, m, WAVE);
        if ((tid & (WAVE - 1)) == 0) part[tid / WAVE][q] = v;
    }
    __syncthreads();
    if (tid < N_ADV) {
        double t = part[0][tid];
        for (int w = 1; w < N_WAVE; ++w) t = t + part[w][tid];
        ws[(size_t)blockIdx.x * N_ADV + tid] = t;
    }
}

// one wavefront: lane q < 2 adds slot q of the partials in block order from block 0
__global__ __launch_bounds__(WAVE) void seq_adv_finish_kernel(const double* ws, int nb, int M, double* adv_stats)
{
    __shared__ double S[N_ADV];
    const int tid = threadIdx.x;
    if (tid < N_ADV) {
        double t = ws[tid];
        for (int b = 1; b < nb; ++b) t = t + ws[(size_t)b * N_ADV + tid];
        S[tid] = t;
    }
    __syncthreads();
    if (tid == 0) glppo::adv_stats_of(S[0], S[1], M, adv_stats);
}

struct Span {
    const void* p;
    size_t n;
};

// [p, p + n) and [q, q + m) share a byte
bool overlaps(const Span& x, const Span& y)
{
    if (!x.p || !y.p || !x.n || !y.n) return false;
    const uintptr_t a = (uintptr_t)x.p, b = (uintptr_t)y.p;
    return a < b + y.n && b < a + x.n;
}

// an output overlaps an input, or another output
int overlap_kind(const Span* in, size_t ni, const Span* out, size_t no)
{
    for (size_t o = 0; o < no; ++o)
        for (size_t i = 0; i < ni; ++i)
            if (overlaps(out[o], in[i])) return 1;
    for (size_t o = 0; o < no; ++o)
        for (size_t p = o + 1; p < no; ++p)
            if (overlaps(out[o], out[p])) return 2;
    return 0;
}

bool aligned16(std::initializer_list<const void*> ps)
{
    for (const void* p : ps)
        if ((uintptr_t)p & 15u) return false;
    return true;
}

// what the two cell entry points refuse alike
int cell_shape_refusal(const std::string& who, int32_t M, int32_t H)
{
    if (M < 1) return refuse(who + ": M < 1");
    if (H < 1 || H > glstm::MAX_H) return refuse(who + ": H outside 1..1024");
    if ((int64_t)M * 4 * (int64_t)H > (int64_t)INT32_MAX) return refuse(who + ": M * 4 H above 2^31 - 1");
    return GLGYM_OK;
}

}  // namespace

extern "C" {

int glgym_lstm_cell(glgym_handle h, const glgym_lstm_cell_args* a, void* stream)
{
    if (!a) return refuse("glgym_lstm_cell: null arguments");
    if (!plan_size_ok("glgym_lstm_cell", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (int rc = cell_shape_refusal("glgym_lstm_cell", a->M, a->H)) return rc;
    if (!a->gx || !a->gh || !a->c_prev) return refuse("glgym_lstm_cell: null gx, gh or c_prev");
    if (!a->h || !a->c) return refuse("glgym_lstm_cell: null h or c");
    const size_t MH = (size_t)a->M * (size_t)a->H, f = sizeof(float);
    const Span in[] = {{a->gx, 4 * MH * f}, {a->gh, 4 * MH * f}, {a->c_prev, MH * f}, {a->start, (size_t)a->M}};
    const Span out[] = {{a->h, MH * f}, {a->c, MH * f}, {a->act, N_ACT * MH * f}};
    switch (overlap_kind(in, 4, out, 3)) {
        case 1: return refuse("glgym_lstm_cell: an output overlaps an input");
        case 2: return refuse("glgym_lstm_cell: an output overlaps another output");
    }
    if (!h) return refuse("glgym_lstm_cell: null handle");
    DeviceGuard dev_guard(h);
    const bool wide = a->H % 4 == 0 && aligned16({a->gx, a->gh, a->c_prev, a->h, a->c, a->act});
    const uint32_t n_lane = (uint32_t)(wide ? MH / 4 : MH);
    const int nb = glstm::n_blocks(n_lane);
    if (wide)
        hipLaunchKernelGGL(lstm_cell_kernel<4>, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, *a, n_lane, (uint32_t)nb * BLOCK);
    else
        hipLaunchKernelGGL(lstm_cell_kernel<1>, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, *a, n_lane, (uint32_t)nb * BLOCK);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_lstm_cell_grad(glgym_handle h, const glgym_lstm_cell_grad_args* a, void* stream)
{
    if (!a) return refuse("glgym_lstm_cell_grad: null arguments");
    if (!plan_size_ok("glgym_lstm_cell_grad", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (int rc = cell_shape_refusal("glgym_lstm_cell_grad", a->M, a->H)) return rc;
    if (!a->dh || !a->act || !a->c_prev) return refuse("glgym_lstm_cell_grad: null dh, act or c_prev");
    if (!a->d_gx || !a->d_gh || !a->d_c_prev) return refuse("glgym_lstm_cell_grad: null d_gx, d_gh or d_c_prev");
    const size_t MH = (size_t)a->M * (size_t)a->H, f = sizeof(float);
    const Span in[] = {{a->dh, MH * f}, {a->dc, MH * f}, {a->act, N_ACT * MH * f}, {a->c_prev, MH * f}, {a->start, (size_t)a->M}};
    const Span out[] = {{a->d_gx, 4 * MH * f}, {a->d_gh, 4 * MH * f}, {a->d_c_prev, MH * f}};
    switch (overlap_kind(in, 5, out, 3)) {
        case 1: return refuse("glgym_lstm_cell_grad: an output overlaps an input");
        case 2: return refuse("glgym_lstm_cell_grad: an output overlaps another output");
    }
    if (!h) return refuse("glgym_lstm_cell_grad: null handle");
    DeviceGuard dev_guard(h);
    const bool wide = a->H % 4 == 0 && aligned16({a->dh, a->dc, a->act, a->c_prev, a->d_gx, a->d_gh, a->d_c_prev});
    const uint32_t n_lane = (uint32_t)(wide ? MH / 4 : MH);
    const int nb = glstm::n_blocks(n_lane);
    if (wide)
        hipLaunchKernelGGL(lstm_cell_grad_kernel<4>, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, *a, n_lane, (uint32_t)nb * BLOCK);
    else
        hipLaunchKernelGGL(lstm_cell_grad_kernel<1>, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, *a, n_lane, (uint32_t)nb * BLOCK);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_seq_batch(glgym_handle h, const glgym_seq_batch_args* a, void* stream)
{
    if (!a) return refuse("glgym_seq_batch: null arguments");
    if (!plan_size_ok("glgym_seq_batch", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->T < 1 || a->B < 1) return refuse("glgym_seq_batch: T or B < 1");
    if (a->L < 1) return refuse("glgym_seq_batch: L < 1");
    if (a->T % a->L != 0) return refuse("glgym_seq_batch: T is no multiple of L");
    if ((int64_t)a->T * (int64_t)a->B > (int64_t)INT32_MAX - (BLOCK - 1)) return refuse("glgym_seq_batch: more than 2^31 - 256 transitions");
    const int64_t N64 = (int64_t)(a->T / a->L) * (int64_t)a->B;
    if (a->S < 1) return refuse("glgym_seq_batch: S < 1");
    if (a->offset < 0) return refuse("glgym_seq_batch: offset < 0");
    if ((int64_t)a->offset + (int64_t)a->S > N64) return refuse("glgym_seq_batch: offset + S > (T / L) B");
    if (a->in_dim < 1 || a->in_dim > glppo::MAX_IN) return refuse("glgym_seq_batch: in_dim outside 1..1024");
    if (a->n_state < 0 || a->n_state > glstm::MAX_STATE) return refuse("glgym_seq_batch: n_state outside 0..4");
    for (int s = 0; s < a->n_state; ++s) {
        if (a->state_dim[s] < 1 || a->state_dim[s] > glstm::MAX_H) return refuse("glgym_seq_batch: a state dimension outside 1..1024");
        if (!a->state_src[s] || !a->state_out[s]) return refuse("glgym_seq_batch: null state_src or state_out");
    }
    if (!a->obs || !a->action || !a->logp || !a->advantage || !a->returns || !a->value || !a->episode_starts)
        return refuse("glgym_seq_batch: null obs, action, logp, advantage, returns, value or episode_starts");
    if (!a->mb_obs || !a->mb_action || !a->mb_logp || !a->mb_adv || !a->mb_ret || !a->mb_value || !a->mb_start)
        return refuse("glgym_seq_batch: null mb_obs, mb_action, mb_logp, mb_adv, mb_ret, mb_value or mb_start");
    const int64_t M64 = (int64_t)a->L * (int64_t)a->S;
    if (a->adv_stats) {
        if (M64 < 2) return refuse("glgym_seq_batch: adv_stats with L * S < 2 (the unbiased deviation divides by L * S - 1)");
        if (!a->workspace) return refuse("glgym_seq_batch: adv_stats without a workspace");
        if (a->workspace_bytes < (int64_t)glppo::BATCH_WS_BYTES) return refuse("glgym_seq_batch: workspace smaller than 16384 bytes");
    }
    const size_t R = (size_t)a->T * (size_t)a->B, N = (size_t)N64, M = (size_t)M64, S = (size_t)a->S, f = sizeof(float), d = (size_t)a->in_dim;
    Span in[8 + glstm::MAX_STATE] = {{a->obs, R * d * f}, {a->action, R * NU * f}, {a->logp, R * f}, {a->advantage, R * f}, {a->returns, R * f},
                                     {a->value, R * f}, {a->episode_starts, R}, {a->draw_base, sizeof(uint64_t)}};
    Span out[10 + glstm::MAX_STATE] = {{a->mb_obs, M * d * f}, {a->mb_action, M * NU * f}, {a->mb_logp, M * f}, {a->mb_adv, M * f},
                                       {a->mb_ret, M * f}, {a->mb_value, M * f}, {a->mb_start, M}, {a->mb_index, S * sizeof(int32_t)},
                                       {a->adv_stats, 2 * sizeof(double)}, {a->adv_stats ? a->workspace : nullptr, glppo::BATCH_WS_BYTES}};
    for (int s = 0; s < a->n_state; ++s) {
        in[8 + s] = {a->state_src[s], N * (size_t)a->state_dim[s] * f};
        out[10 + s] = {a->state_out[s], S * (size_t)a->state_dim[s] * f};
    }
    switch (overlap_kind(in, 8 + (size_t)a->n_state, out, 10 + (size_t)a->n_state)) {
        case 1: return refuse("glgym_seq_batch: an output overlaps a source");
        case 2: return refuse("glgym_seq_batch: an output overlaps another output");
    }
    if (!h) return refuse("glgym_seq_batch: null handle");
    DeviceGuard dev_guard(h);
    const int nb = glppo::n_blocks(a->S);
    hipLaunchKernelGGL(seq_batch_kernel, dim3((unsigned)nb), dim3(BLOCK), 0, (hipStream_t)stream, *a, nb, glppo::half_bits((uint32_t)N),
                       (uint32_t)N);
    HIPCHK(hipGetLastError());
    if (a->adv_stats) {
        const int nba = glppo::n_blocks(M64);
        hipLaunchKernelGGL(seq_adv_kernel, dim3((unsigned)nba), dim3(BLOCK), 0, (hipStream_t)stream, a->mb_adv, M64, nba, a->workspace);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(seq_adv_finish_kernel, dim3(1), dim3(WAVE), 0, (hipStream_t)stream, a->workspace, nba, (int)M64, a->adv_stats);
        HIPCHK(hipGetLastError());
    }
    return GLGYM_OK;
}

}  // extern "C"
