// glgym_search.hip -- the part of device-side planning that ranks and searches over finished returns and never touches an env-step
// (include/glgym.h glgym_plan_select .. _cma_update), kernels and C entry points: pick the best of K candidates per parent and the
// MPPI-weighted mean, aggregate scenario returns, rank under constraints, and the stages of CEM, ES and CMA-ES.  What drives env-steps --
// fork, accumulate, the prologues, the rollouts -- is glgym_plan.hip.  The scalar logic is the gl_*.hpp headers' (each instantiated on
// the host by a tests/*host/*.cpp).  Each entry point checks its arguments and launches its kernels itself, at the bottom of this file.
//
// Layouts.  select: one wavefront per parent, lanes stride over the candidates k, partial (value, index) pairs and sums are combined
// with butterfly shuffles; the action block [H][P*K][6] f32 is read with lanes over k, 6 consecutive floats each, so a wavefront touches 1 536
// contiguous bytes per load round.  The MPPI mean runs one wavefront per (parent, horizon step): the K returns are re-read from L2 by
// each (9 bytes per candidate against the 24 bytes of its action row), which keeps the call free of workspace and allocation.
// These two use no LDS; no kernel here uses atomics, all stores are plain vector stores.
//
// The cross-entropy method's stages (glgym_plan_sample / _elites / _refit; scalar logic in gl_cem.hpp, instantiated on the host by
// tests/cemhost/cemhost.cpp).  sample: lane = child, four wavefronts per 64 children share the horizon's steps (the normals are the
// cost; the recurrence along h runs per lane over normals staged in LDS); 6 consecutive floats per lane, so a wavefront writes 1 536
// contiguous bytes per step; the mean / std rows of a parent are broadcast reads.  elites: lane = candidate, ceil(K / 64) blocks of
// four wavefronts per parent; the parent's K returns pass through LDS in tiles of 256 (every lane reads the same LDS address, a
// broadcast) and each thread counts the candidates that come before its own -- the rank IS the output slot, so there is no sort
// network and no atomic.  refit: one wavefront per (parent, horizon step), lanes stride over the elites, two passes over at most E
// gathered rows.
//
// The evolution strategy's stages (glgym_plan_es_sample / _es_utilities / _es_update; scalar logic in gl_es.hpp, instantiated on the host
// by tests/eshost/eshost.cpp).  sample: lane = mirrored pair, one wavefront per 64 pairs and plane, four to a block; no LDS (no recurrence along
// h), three 16-byte stores per lane and plane.  utilities: the elites' grid and counting, one utility stored per candidate.  update: one
// wavefront per (row, plane), lanes stride over the pairs, one pass over the plane's K rows, lane 0 steps mean, std and moments.
//
// The CMA-ES stages (glgym_plan_cma_sample / _cma_update; scalar logic in gl_cma.hpp, instantiated on the host by
// tests/cmahost/cmahost.cpp).  sample: lane = child, the children of a block from one row, whose Cholesky factor sits in LDS (broadcast
// reads); y = chol z is accumulated column by column in registers.  update: one block per row; the elites' y pass through LDS in tiles,
// every sum over the elites runs sequentially in the thread that owns its output, the Cholesky factorisation with lanes on rows; the
// new state waits in LDS until the row's status is known.
//
// Robust planning's aggregation (glgym_plan_aggregate; scalar logic in gl_scen.hpp, instantiated on the host by
// tests/scenhost/scenhost.cpp): one wavefront per candidate, its S <= 256 scenario returns ranked by counting in LDS and summed in
// rank order by one lane.
//
// Constrained ranking (glgym_plan_constrain; scalar logic in gl_constr.hpp, instantiated on the host by tests/constrhost/constrhost.cpp).
// candidates, more than 8 runs each: one wavefront per candidate, four to a block; the lanes stride over its R runs, the lane sums are
// added in lane order by reading lane after lane (the lane index is uniform: no LDS, no barrier).  Up to 8 runs (the planner's S <= 8):
// lane = candidate, the runs added in ascending r, which is the same sum bit for bit; a wavefront reads 64 x S consecutive doubles per
// violation row.  groups: one block of 256 per ranking group; the smallest admissible feasible return by a strided pass and a
// tree over LDS (a minimum has no order), then the scores.  Two launches, so that 8 192 candidates of ONE group do not run their
// 64*S runs each on one workgroup.
#include <cmath>
#include <string>

#include "glgym_internal.h"

#include "gl_cem.hpp"
#include "gl_cma.hpp"
#include "gl_constr.hpp"
#include "gl_es.hpp"
#include "gl_plan.hpp"
#include "gl_scen.hpp"

namespace {

constexpr int NU = GLGYM_NU;
constexpr int WAVE = glplan::WAVE;

__device__ __forceinline__ glplan::Cand wave_best(glplan::Cand c)
{
    for (int m = WAVE / 2; m > 0; m >>= 1) {
        glplan::Cand o;
        o.v = __shfl_xor(c.v, m, WAVE);
        o.k = __shfl_xor(c.k, m, WAVE);
        c = glplan::combine(c, o);
    }
    return c;
}

__device__ __forceinline__ double wave_sum(double v)
{
    for (int m = WAVE / 2; m > 0; m >>= 1) v = v + __shfl_xor(v, m, WAVE);
    return v;
}

// grid = P, one wavefront each
__global__ __launch_bounds__(WAVE) void plan_select_kernel(glgym_plan_select_args a)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const size_t first = (size_t)p * a.K;               // the parent's first child
    const glplan::Cand c = wave_best(glplan::lane_best(lane, a.K, a.ret + first, a.failed + first));
    const bool none = c.k == glplan::NONE;
    if (lane == 0) {
        a.best_k[p] = none ? -1 : c.k;
        a.best_ret[p] = none ? __builtin_nan("") : c.v;
    }
    if (!a.actions) return;
    const size_t n_child = (size_t)a.P * a.K;
    if (a.best_action && lane < NU) a.best_action[(size_t)p * NU + lane] = none ? 0.f : a.actions[(first + c.k) * NU + lane];
    if (a.best_sequence)
        for (int i = lane; i < a.H * NU; i += WAVE) {
            const int h = i / NU, j = i - h * NU;
            a.best_sequence[((size_t)h * a.P + p) * NU + j] = none ? 0.f : a.actions[((size_t)h * n_child + first + c.k) * NU + j];
        }
}

// grid = (P, H), one wavefront each
__global__ __launch_bounds__(WAVE) void plan_mean_kernel(glgym_plan_select_args a)
{
    const int p = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const size_t first = (size_t)p * a.K;
    const double* ret = a.ret + first;
    const uint8_t* failed = a.failed + first;
    const glplan::Cand c = wave_best(glplan::lane_best(lane, a.K, ret, failed));
    double acc[NU] = {0, 0, 0, 0, 0, 0};
    if (c.k != glplan::NONE) {                          // wave-uniform
        const double inv_t = 1.0 / a.temperature;
        const double z = wave_sum(glplan::lane_weight_sum(lane, a.K, ret, failed, c.v, inv_t));
        glplan::lane_mean(lane, a.K, ret, failed, c.v, inv_t, z, a.actions + ((size_t)h * a.P * a.K + first) * NU, acc);
        for (int j = 0; j < NU; ++j) acc[j] = wave_sum(acc[j]);
    }
    if (lane == 0) {
        float* out = a.mean_sequence + ((size_t)h * a.P + p) * NU;
        for (int j = 0; j < NU; ++j) out[j] = (float)acc[j];
    }
}

// grid = ceil(C / 64) blocks of SAMPLE_WAVES wavefronts: lane = child, wave w draws the normals of the steps h = g*SAMPLE_WAVES + w
// (the costly part: two Philox blocks, three ln / sqrt / sin / cos in double) and stages them in LDS; every lane then runs its child's
// recurrence n_h = beta n_{h-1} + sb e_h over the group's steps in step order -- 6 x SAMPLE_WAVES multiply-adds, repeated by each wave
// rather than exchanged -- keeps n at the group's end, and writes the row of its own step: 1 536 contiguous bytes per wave.
constexpr int SAMPLE_WAVES = 4;
__global__ __launch_bounds__(SAMPLE_WAVES * WAVE) void plan_sample_kernel(glgym_plan_sample_args a)
{
    __shared__ double s_e[SAMPLE_WAVES][NU][WAVE];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int n_child = a.P * a.K;
    const int c_raw = blockIdx.x * WAVE + lane;
    const bool live = c_raw < n_child;
    const int c = live ? c_raw : n_child - 1;           // lanes past the end shadow the last child and store nothing
    const int p = c / a.K, k = c - p * a.K;
    const uint64_t D = a.draw_index + (a.draw_base ? *a.draw_base : 0ull);
    int src = 0;
    const int kind = glcem::reserved(p, k, a.K, a.carry, a.prev_E, a.prev_elite_k, a.prev_n_elite, &src);
    const double sb = glcem::sb_of(a.beta);
    double n[NU] = {0, 0, 0, 0, 0, 0};
    for (int g = 0; g < a.H; g += SAMPLE_WAVES) {       // block-uniform trip count: every thread reaches both barriers
        const int h = g + w;
        if (h < a.H && kind == 0) {
            double e[NU];
            glcem::normals_of(c, h, D, a.seed, e);
            for (int j = 0; j < NU; ++j) s_e[w][j][lane] = e[j];
        }
        __syncthreads();
        double mine[NU] = {0, 0, 0, 0, 0, 0};
        if (kind == 0) {
            const int n_steps = a.H - g < SAMPLE_WAVES ? a.H - g : SAMPLE_WAVES;
            for (int s = 0; s < n_steps; ++s) {
                double e[NU];
                for (int j = 0; j < NU; ++j) e[j] = s_e[s][j][lane];
                glcem::colour(g + s, a.beta, sb, e, n);
                if (s == w)
                    for (int j = 0; j < NU; ++j) mine[j] = n[j];
            }
        }
        if (live && h < a.H) glcem::write_row(kind, src, h, p, c, a.P, a.K, a.mean, a.std, mine, a.prev_actions, a.actions);
        __syncthreads();                                // the group's normals have been read by everyone
    }
}

// grid = P * n_chunks blocks of ELITE_WAVES wavefronts: block (p, i) ranks the 64 candidates i*64 .. i*64 + 63 of parent p, lane =
// candidate.  The parent's keys (return, or NaN if not admissible) pass through LDS in tiles of 256; wave w counts the tile's
// w-th 64 keys against its lane's candidate -- each LDS read is a broadcast -- and the four partial ranks are added through LDS.
constexpr int ELITE_WAVES = glcem::TILE / glcem::CHUNK;
__global__ __launch_bounds__(glcem::TILE) void plan_elites_kernel(glgym_plan_elites_args a, int n_chunks)
{
    constexpr int TILE = glcem::TILE, CHUNK = glcem::CHUNK;
    __shared__ double s_key[TILE];
    __shared__ int s_rank[ELITE_WAVES][CHUNK];
    const int p = blockIdx.x / n_chunks, tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int k0 = (blockIdx.x - p * n_chunks) * CHUNK, t = k0 + lane;
    const double* ret = a.ret + (size_t)p * a.K;
    const uint8_t* failed = a.failed + (size_t)p * a.K;
    const double rk = t < a.K ? glcem::key(ret[t], failed[t]) : __builtin_nan("");
    int rank = 0, n_adm = 0;
    for (int j0 = 0; j0 < a.K; j0 += TILE) {            // block-uniform trip count: every thread reaches both barriers
        const int j = j0 + tid;
        const double kj = j < a.K ? glcem::key(ret[j], failed[j]) : __builtin_nan("");
        s_key[tid] = kj;
        n_adm += __syncthreads_count(kj == kj);         // a barrier, and the tile's number of admissible candidates
        const int c0 = j0 + w * CHUNK, n = a.K - c0 < CHUNK ? a.K - c0 : CHUNK;
        if (n > 0) rank += glcem::count_chunk(s_key + w * CHUNK, c0, n, rk, t, k0);
        __syncthreads();                                // the tile has been read by everyone
    }
    s_rank[w][lane] = rank;
    __syncthreads();
    if (w == 0) {
        for (int i = 1; i < ELITE_WAVES; ++i) rank += s_rank[i][lane];
        glcem::store_rank(t, a.K, a.E, rk == rk, rank, n_adm, a.elite_k + (size_t)p * a.E, a.n_elite + p);
    }
}

// grid = (P, H), one wavefront each
__global__ __launch_bounds__(WAVE) void plan_refit_kernel(glgym_plan_refit_args a)
{
    const int p = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    int n = a.n_elite[p];
    n = n < 0 ? 0 : (n > a.E ? a.E : n);
    const int32_t* elite = a.elite_k + (size_t)p * a.E;
    const float* rows = a.actions + ((size_t)h * a.P + p) * a.K * NU;
    const size_t o = ((size_t)h * a.P + p) * NU;
    double acc[NU], m[NU], s[NU];
    const bool ok = glcem::lane_sum(lane, n, elite, a.K, rows, acc);
    const bool keep = n == 0 || __any(!ok);             // wave-uniform
    if (!keep) {
        for (int j = 0; j < NU; ++j) m[j] = wave_sum(acc[j]) / (double)n;
        glcem::lane_sqdev(lane, n, elite, rows, m, acc);
        for (int j = 0; j < NU; ++j) s[j] = sqrt(wave_sum(acc[j]) / (double)n);
    }
    if (lane == 0)
        for (int j = 0; j < NU; ++j) {
            const float mean = a.mean[o + j], sd = a.std[o + j];      // read before the (possibly aliased) stores
            a.mean_out[o + j] = keep ? mean : (float)glcem::blend_mean(a.alpha, mean, m[j]);
            a.std_out[o + j] = keep ? sd : (float)glcem::blend_std(a.alpha, sd, s[j], a.min_std);
        }
}

// ---- the evolution strategy's stages (gl_es.hpp) ------------------------------------------------------------------------------------
// grid = (ceil(P*M / 64), ceil(H / SAMPLE_WAVES)) blocks of SAMPLE_WAVES wavefronts: lane = pair q = p*M + m, wave w of block (x, y)
// draws the plane h = y * SAMPLE_WAVES + w, so that a small population (P*M of a few thousand) still fills the chip with its planes.
// There is no recurrence along h (beta = 0), so nothing is staged: a lane draws its pair's six normals once and stores both rows, 48
// contiguous bytes (16-byte aligned: 48 q from an aligned base, P*K even) as three 16-byte stores; a wave writes 3 072 contiguous bytes.
__global__ __launch_bounds__(SAMPLE_WAVES * WAVE) void plan_es_sample_kernel(glgym_plan_es_sample_args a)
{
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    const int M = a.K / 2, n_pair = a.P * M;
    const int q = blockIdx.x * WAVE + lane, h = blockIdx.y * SAMPLE_WAVES + w;
    if (q >= n_pair || h >= a.H) return;                // no barrier below
    const int p = q / M;
    const uint64_t D = a.draw_index + (a.draw_base ? *a.draw_base : 0ull);
    const size_t row = ((size_t)h * a.P + p) * NU;
    float r[2 * NU];
    gles::pair_rows(q, h, D, a.seed, a.mean + row, a.std + row, r);
    float4* out = reinterpret_cast<float4*>(a.actions + ((size_t)h * a.P * a.K + 2 * (size_t)q) * NU);
    out[0] = make_float4(r[0], r[1], r[2], r[3]);
    out[1] = make_float4(r[4], r[5], r[6], r[7]);
    out[2] = make_float4(r[8], r[9], r[10], r[11]);
}

// plan_elites_kernel's grid and counting (P * n_chunks blocks, tiles of 256 keys in LDS, broadcast reads); every candidate stores its
// utility, thread 0 of a row's first block the row's number of admissible candidates.
__global__ __launch_bounds__(glcem::TILE) void plan_es_utilities_kernel(glgym_plan_es_utilities_args a, int n_chunks)
{
    constexpr int TILE = glcem::TILE, CHUNK = glcem::CHUNK;
    __shared__ double s_key[TILE];
    __shared__ int s_rank[ELITE_WAVES][CHUNK];
    const int p = blockIdx.x / n_chunks, tid = threadIdx.x, lane = tid & (WAVE - 1), w = tid / WAVE;
    const int k0 = (blockIdx.x - p * n_chunks) * CHUNK, t = k0 + lane;
    const double* ret = a.ret + (size_t)p * a.K;
    const uint8_t* failed = a.failed + (size_t)p * a.K;
    const double rk = t < a.K ? glcem::key(ret[t], failed[t]) : __builtin_nan("");
    int rank = 0, n_adm = 0;
    for (int j0 = 0; j0 < a.K; j0 += TILE) {            // block-uniform trip count: every thread reaches both barriers
        const int j = j0 + tid;
        const double kj = j < a.K ? glcem::key(ret[j], failed[j]) : __builtin_nan("");
        s_key[tid] = kj;
        n_adm += __syncthreads_count(kj == kj);
        const int c0 = j0 + w * CHUNK, n = a.K - c0 < CHUNK ? a.K - c0 : CHUNK;
        if (n > 0) rank += glcem::count_chunk(s_key + w * CHUNK, c0, n, rk, t, k0);
        __syncthreads();
    }
    s_rank[w][lane] = rank;
    __syncthreads();
    if (w == 0) {
        for (int i = 1; i < ELITE_WAVES; ++i) rank += s_rank[i][lane];
        if (t < a.K) a.u[(size_t)p * a.K + t] = gles::utility(rk == rk, rank, n_adm);
        if (t == 0) a.n_adm[p] = n_adm;
    }
}

// grid = (P, H), one wavefront each: lane l takes the pairs m = l, l + 64, ... -- 48 bytes of the plane as three 16-byte loads, the two
// utilities as one -- so a load round of the wavefront covers 3 072 contiguous bytes; the population is read once.  The sums end in
// every lane (butterfly); lane 0 updates and stores.
__global__ __launch_bounds__(WAVE) void plan_es_update_kernel(glgym_plan_es_update_args a)
{
    const gles::Hyper hp{a.optimizer, a.lr, a.lr_std, a.std_decay, a.min_std, a.max_std, a.beta1, a.beta2, a.eps};
    const int p = blockIdx.x, h = blockIdx.y, lane = threadIdx.x;
    const int M = a.K / 2;
    const size_t o = ((size_t)h * a.P + p) * NU;
    const float4* rows = reinterpret_cast<const float4*>(a.actions + ((size_t)h * a.P + p) * a.K * NU);
    const double2* u = reinterpret_cast<const double2*>(a.u + (size_t)p * a.K);
    double sigma[NU], g[NU], s[NU];
    for (int j = 0; j < NU; ++j) { sigma[j] = (double)a.std[o + j]; g[j] = s[j] = 0.0; }
    for (int m = lane; m < M; m += WAVE) {
        const float4 r0 = rows[3 * (size_t)m], r1 = rows[3 * (size_t)m + 1], r2 = rows[3 * (size_t)m + 2];
        const double2 um = u[m];
        const float r[2 * NU] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w, r2.x, r2.y, r2.z, r2.w};
        gles::pair_terms(r, um.x, um.y, sigma, g, s);
    }
    for (int j = 0; j < NU; ++j) {
        g[j] = wave_sum(g[j]) / (double)M;
        s[j] = wave_sum(s[j]) / (double)M;
    }
    if (lane != 0) return;
    const uint64_t t = a.t_index + (a.t_base ? *a.t_base : 0ull);
    const bool keep = a.n_adm[p] < 2 || t == 0 || !gles::finite6(g) || !gles::finite6(s);
    gles::update_row(hp, t, keep, g, s, a.mean + o, a.std + o, a.m1 ? a.m1 + o : nullptr, a.m2 ? a.m2 + o : nullptr, a.mean_out + o, a.std_out + o);
}

// ---- the CMA-ES stages (gl_cma.hpp) -------------------------------------------------------------------------------------------------
// grid = P * ceil(K / 256) blocks of four wavefronts: block (p, i) samples the children k = i*256 .. i*256 + 255 of row p, lane = child.
// The row's factor is staged in LDS once per block (N*N doubles, at most 8 KB); every later read of it is a broadcast.  A lane keeps
// its y in registers (unrolled indices, no scratch) and stores 6 consecutive floats per plane: 1 536 contiguous bytes per wavefront.
constexpr int CMA_THREADS = 256;
__global__ __launch_bounds__(CMA_THREADS) void plan_cma_sample_kernel(glgym_plan_cma_sample_args a, int n_chunks)
{
    __shared__ double s_chol[glcma::NMAX * glcma::NMAX];
    const int p = blockIdx.x / n_chunks, tid = threadIdx.x, N = a.N;
    const double* chol = a.chol + (size_t)p * N * N;
    for (int i = tid; i < N * N; i += CMA_THREADS) s_chol[i] = chol[i];
    __syncthreads();
    const int k = (blockIdx.x - p * n_chunks) * CMA_THREADS + tid;
    if (k >= a.K) return;                               // no barrier below
    const uint64_t D = a.draw_index + (a.draw_base ? *a.draw_base : 0ull);
    glcma::sample_child(p * a.K + k, p, a.P, a.K, N, D, a.seed, s_chol, a.mean, a.sigma[p], a.theta);
}

// grid = P, one block of four wavefronts per row.  The elites' y pass through LDS in tiles of min(256, 1 024 / N) elites (any E; a
// thread stages up to four values of a tile, index loads first, so that their latencies overlap); thread d < N owns yw[d] and every
// thread up to three entries (a, b <= a) of R -- the lower triangle's N (N + 1) / 2 entries are numbered row by row and dealt out
// 256 at a time -- each summed over the elites in ascending order by its owner alone.  The sequential parts -- forward substitution,
// the paths, the Cholesky factorisation -- run in wavefront 0 with lanes on rows (N <= 32 <= 64); a finished value reaches the other
// lanes by a shuffle or through LDS.  Every new value waits in LDS or in a register until the row's status is known; then the block
// commits all of them or none.  LDS: 8 KB of y, 2 KB of weights, 8 KB for the old and then the new factor, 8 KB of cov', a few vectors.
// row a of entry idx of the lower triangle numbered row by row (entry idx = a (a + 1) / 2 + b, b <= a)
__device__ __forceinline__ int cma_tri_row(int idx)
{
    int a = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
    while (a * (a + 1) / 2 > idx) --a;
    while ((a + 1) * (a + 2) / 2 <= idx) ++a;
    return a;
}

__global__ __launch_bounds__(CMA_THREADS) void plan_cma_update_kernel(glgym_plan_cma_update_args a)
{
    constexpr int NM = glcma::NMAX, NT = CMA_THREADS, SLOTS = NM * NM, TE_MAX = 256, STAGE = SLOTS / NT;
    constexpr int PER = (NM * (NM + 1) / 2 + NT - 1) / NT;
    __shared__ double s_y[SLOTS];                       // [e][d] with rows of N: TE * N <= 1 024
    __shared__ double s_w[TE_MAX];
    __shared__ double s_chol[NM * NM];
    __shared__ double s_cov[NM * NM];
    __shared__ double s_pc[NM];
    __shared__ float s_m[NM];
    __shared__ double s_a0;
    const glcma::Hyper hp{a.mu_eff, a.c_sigma, a.d_sigma, a.c_c, a.c_1, a.c_mu, a.chi_n, a.min_sigma, a.max_sigma};
    const int p = blockIdx.x, tid = threadIdx.x, N = a.N, E = a.E, K = a.K, NN = N * N, n_tri = N * (N + 1) / 2;
    const int TE = SLOTS / N < TE_MAX ? SLOTS / N : TE_MAX;
    const uint64_t t = a.t_index + (a.t_base ? *a.t_base : 0ull);
    const int32_t* elite = a.elite_k + (size_t)p * E;
    const size_t n_child = (size_t)a.P * K, first = (size_t)p * K, oN = (size_t)p * N, oNN = (size_t)p * NN;
    int bad_e = 0;
    for (int e = tid; e < E; e += NT) bad_e |= (elite[e] < 0 || elite[e] >= K) ? 1 : 0;
    const bool few = __syncthreads_or(bad_e) != 0 || a.n_elite[p] < E;
    if (t == 0 || few) {                                // block-uniform
        if (tid == 0) a.status[p] = t == 0 ? glcma::T_ZERO : glcma::FEW_ELITES;
        return;
    }
    const double sigma = a.sigma[p];
    for (int i = tid; i < NN; i += NT) s_chol[i] = a.chol[oNN + i];
    if (tid < N) s_m[tid] = a.mean[((size_t)(tid / NU) * a.P + p) * NU + tid % NU];
    __syncthreads();
    double yw = 0.0, R[PER];
    int ra[PER], rb[PER];                               // this thread's entries (a, b <= a) of the lower triangle; a = -1: none
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int idx = tid + r * NT;
        R[r] = 0.0;
        ra[r] = idx < n_tri ? cma_tri_row(idx) : -1;
        rb[r] = idx < n_tri ? idx - ra[r] * (ra[r] + 1) / 2 : 0;
    }
    for (int e0 = 0; e0 < E; e0 += TE) {                // block-uniform trip count: every thread reaches both barriers
        const int ne = E - e0 < TE ? E - e0 : TE, n_val = ne * N;
        int kk[STAGE];
        float xx[STAGE];
#pragma unroll
        for (int r = 0; r < STAGE; ++r) {
            const int idx = tid + r * NT;
            kk[r] = idx < n_val ? elite[e0 + idx / N] : 0;
        }
#pragma unroll
        for (int r = 0; r < STAGE; ++r) {
            const int idx = tid + r * NT, d = idx % N;
            xx[r] = idx < n_val ? a.theta[((size_t)(d / NU) * n_child + first + kk[r]) * NU + d % NU] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < STAGE; ++r) {
            const int idx = tid + r * NT;
            if (idx < n_val) s_y[idx] = glcma::elite_y(xx[r], s_m[idx % N], sigma);
        }
        if (tid < ne) s_w[tid] = a.w_dev[e0 + tid];
        __syncthreads();
        if (tid < N)
            for (int e = 0; e < ne; ++e) yw = glcma::add_yw(yw, s_w[e], s_y[e * N + tid]);
#pragma unroll
        for (int r = 0; r < PER; ++r)
            if (ra[r] >= 0)
                for (int e = 0; e < ne; ++e) R[r] = glcma::add_r(R[r], s_w[e], s_y[e * N + ra[r]], s_y[e * N + rb[r]]);
        __syncthreads();                                // the tile has been read by everyone
    }
    // wavefront 0, lane d = component d: forward substitution, the paths, the mean, the step size
    double ps_new = 0.0, pc_new = 0.0, sig_new = 0.0;
    float mean_new = 0.f;
    int bad = 0;
    if (tid < WAVE) {                                   // wave-uniform
        const int d = tid;
        const bool mine = d < N;
        double acc = mine ? yw : 0.0, zw = 0.0;
        for (int j = 0; j < N; ++j) {
            double zc = 0.0;
            if (d == j) zc = acc / s_chol[d * N + d];
            const double zj = __shfl(zc, j, WAVE);
            if (d == j) zw = zj;
            if (mine && d > j) acc = glcma::fsub_take(acc, s_chol[d * N + j], zj);
        }
        const double qs = glcma::q_of(hp.c_sigma, hp.mu_eff), qc = glcma::q_of(hp.c_c, hp.mu_eff);
        ps_new = mine ? glcma::blend(hp.c_sigma, a.p_sigma[oN + d], glcma::times(qs, zw)) : 0.0;
        double n2 = 0.0;
        for (int j = 0; j < N; ++j) n2 = glcma::add_sq(n2, __shfl(ps_new, j, WAVE));
        const double nrm = sqrt(n2);
        const bool hs = glcma::h_sigma(hp, N, t, nrm);
        pc_new = mine ? glcma::blend(hp.c_c, a.p_c[oN + d], hs ? glcma::times(qc, yw) : 0.0) : 0.0;
        mean_new = mine ? glcma::new_mean(s_m[mine ? d : 0], sigma, yw) : 0.f;
        sig_new = glcma::new_sigma(hp, sigma, nrm);
        if (mine) s_pc[d] = pc_new;
        if (tid == 0) s_a0 = glcma::a0_of(hp, hs);
        bad = !(std::isfinite(ps_new) && std::isfinite(pc_new) && std::isfinite(mean_new) && std::isfinite(sig_new)) ? 1 : 0;
    }
    __syncthreads();                                    // p_c' and a0 are there; the old factor is not read again
#pragma unroll
    for (int r = 0; r < PER; ++r) {
        const int ai = ra[r], bi = rb[r];
        if (ai >= 0) {
            const double v = glcma::cov_entry(hp, s_a0, a.cov[oNN + ai * N + bi], s_pc[ai], s_pc[bi], R[r]);
            s_cov[ai * N + bi] = v;
            s_cov[bi * N + ai] = v;
            bad |= std::isfinite(v) ? 0 : 1;
        }
    }
    for (int i = tid; i < NN; i += NT) s_chol[i] = 0.0;
    int status = __syncthreads_or(bad) != 0 ? glcma::NOT_FINITE : glcma::UPDATED;
    if (status == glcma::UPDATED) {                     // block-uniform
        int pivot_bad = 0;
        for (int j = 0; j < N; ++j) {                   // lanes on rows i >= j, j sequential
            if (tid < WAVE) {
                const int i = tid;
                const bool work = i >= j && i < N;
                const double v = work ? glcma::chol_take(s_cov[i * N + j], s_chol + i * N, s_chol + j * N, j) : 0.0;
                const double s = __shfl(v, j, WAVE);
                pivot_bad |= s > 0.0 ? 0 : 1;
                const double piv = sqrt(s);
                if (work) s_chol[i * N + j] = i == j ? piv : v / piv;
            }
            __syncthreads();                            // column j is there
        }
        int inf = 0;
        for (int i = tid; i < NN; i += NT) inf |= std::isfinite(s_chol[i]) ? 0 : 1;
        const bool np = __syncthreads_or(pivot_bad) != 0, nf = __syncthreads_or(inf) != 0;
        status = np ? glcma::NOT_POSITIVE : (nf ? glcma::NOT_FINITE : glcma::UPDATED);
    }
    if (tid == 0) a.status[p] = status;
    if (status != glcma::UPDATED) return;               // the row keeps its bits
    for (int i = tid; i < NN; i += NT) {
        a.cov[oNN + i] = s_cov[i];
        a.chol[oNN + i] = s_chol[i];
    }
    if (tid < N) {
        a.p_sigma[oN + tid] = ps_new;
        a.p_c[oN + tid] = pc_new;
        a.mean[((size_t)(tid / NU) * a.P + p) * NU + tid % NU] = mean_new;
    }
    if (tid == 0) a.sigma[p] = sig_new;
}

// grid = J, one wavefront per candidate.  Its S <= 256 returns are staged in LDS; every lane ranks its scenarios s = lane, lane + 64,
// ... by counting over the staged row (each LDS read a broadcast) and puts them into their slot of the ascending row; lane 0 then sums
// the first m slots in order.  Lanes 1..3 sum one violation row each in index order, lane 4 takes the minimum of the step counts.
__global__ __launch_bounds__(WAVE) void plan_aggregate_kernel(glgym_plan_aggregate_args a)
{
    __shared__ double s_val[glscen::MAX_S], s_sorted[glscen::MAX_S];
    const int lane = threadIdx.x;
    const size_t j = blockIdx.x, first = j * (size_t)a.S;
    bool is_bad = false;
    for (int s = lane; s < a.S; s += WAVE) {
        const double r = a.ret[first + s];
        s_val[s] = r;
        is_bad = is_bad || glscen::bad(r, a.failed[first + s]);
    }
    __syncthreads();
    is_bad = __any(is_bad);                             // wave-uniform
    if (!is_bad)
        for (int s = lane; s < a.S; s += WAVE) s_sorted[glscen::rank_asc(s_val, a.S, s)] = s_val[s];
    __syncthreads();
    if (lane == 0) {
        a.ret_cand[j] = is_bad ? glscen::nan_value() : glscen::tail_mean(s_sorted, a.m);
        a.failed_cand[j] = is_bad ? 1 : 0;
    } else if (lane <= 3) {
        if (a.viol_cand) a.viol_cand[(size_t)(lane - 1) * a.ld_cand + j] = glscen::seq_mean(a.viol + (size_t)(lane - 1) * a.ld + first, a.S);
    } else if (lane == 4) {
        if (a.steps_cand) a.steps_cand[j] = glscen::min_steps(a.n_steps + first, a.S);
    }
}

// What the candidates' kernels leave for plan_constrain_groups_kernel: G in score[j] and failed_out | infeasible << 1 in failed_out[j]
// (score never overlaps ret_cand; failed_out[j] is read, as failed_cand[j], by the thread that writes it).
__device__ __forceinline__ void constrain_store(const glgym_plan_constrain_args& a, int j, int R, double total, int n_viol, bool nonfinite)
{
    const double G = glconstr::mean_excess(total, R);
    const uint8_t flags = glconstr::flags_of(a.ret_cand[j], a.failed_cand[j], nonfinite, n_viol, a.n_allow);
    a.score[j] = G;
    a.failed_out[j] = flags;
    if (a.excess) a.excess[j] = G;
    if (a.n_viol) a.n_viol[j] = n_viol;
    if (a.feasible) a.feasible[j] = (flags & glconstr::FLAG_INFEASIBLE) ? 0 : 1;
}

// R <= SMALL_R: grid = ceil(J / 256), lane = candidate, its runs added in ascending r (gl_constr.hpp: the defined sum, bit for bit)
__global__ __launch_bounds__(256) void plan_constrain_few_runs_kernel(glgym_plan_constrain_args a, glconstr::Spec sp, int J)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= J) return;
    const glconstr::Part part = glconstr::thread_runs(sp, j / a.K, j % a.K, a.viol, (size_t)a.ld, a.n_steps);
    constrain_store(a, j, sp.O * sp.S, part.sum, part.n_viol, part.nonfinite);
}

// R > SMALL_R: grid = ceil(J / CONSTR_WAVES) blocks of CONSTR_WAVES wavefronts, one wavefront per candidate j = p*K + k
constexpr int CONSTR_WAVES = 4;
__global__ __launch_bounds__(CONSTR_WAVES * WAVE) void plan_constrain_candidates_kernel(glgym_plan_constrain_args a, glconstr::Spec sp, int J)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int j = blockIdx.x * CONSTR_WAVES + threadIdx.x / WAVE;
    if (j >= J) return;                                 // wave-uniform
    const int p = j / a.K, k = j - p * a.K;
    const glconstr::Part part = glconstr::lane_runs(lane, sp, p, k, a.viol, (size_t)a.ld, a.n_steps);
    double total = 0.0;
    for (int l = 0; l < WAVE; ++l) total = glconstr::combine(total, __shfl(part.sum, l, WAVE));
    int n_viol = part.n_viol;
    for (int m = WAVE / 2; m > 0; m >>= 1) n_viol += __shfl_xor(n_viol, m, WAVE);
    const bool nonfinite = __any(part.nonfinite);
    if (lane == 0) constrain_store(a, j, sp.O * sp.S, total, n_viol, nonfinite);
}

// grid = P, one block of GROUP_THREADS per ranking group: threads stride over its K candidates
__global__ __launch_bounds__(glconstr::GROUP_THREADS) void plan_constrain_groups_kernel(glgym_plan_constrain_args a)
{
    constexpr int T = glconstr::GROUP_THREADS;
    __shared__ double s_min[T];
    __shared__ int s_cnt[T];
    const int p = blockIdx.x, tid = threadIdx.x;
    const size_t first = (size_t)p * a.K;
    double mn = __builtin_inf();
    int cnt = 0;
    for (int k = tid; k < a.K; k += T)
        if (glconstr::counts_for_floor(a.failed_out[first + k])) {
            const double r = a.ret_cand[first + k];
            mn = r < mn ? r : mn;
            ++cnt;
        }
    s_min[tid] = mn;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int m = T / 2; m > 0; m >>= 1) {               // block-uniform trip count: every thread reaches the barrier
        if (tid < m) {
            s_min[tid] = s_min[tid + m] < s_min[tid] ? s_min[tid + m] : s_min[tid];
            s_cnt[tid] += s_cnt[tid + m];
        }
        __syncthreads();
    }
    const int n_feasible = s_cnt[0];
    const double floor_p = glconstr::floor_of(s_min[0], n_feasible);
    for (int k = tid; k < a.K; k += T) {                // every flag was read before the first barrier; k belongs to this thread alone
        const uint8_t flags = a.failed_out[first + k];
        a.score[first + k] = glconstr::score_of(a.mode, a.ret_cand[first + k], a.score[first + k], flags, floor_p, a.rho);
        a.failed_out[first + k] = flags & glconstr::FLAG_FAILED;
    }
    if (tid == 0 && a.n_feasible) a.n_feasible[p] = n_feasible;
}

}  // namespace

extern "C" {

// ---- the C entry points: argument checks and the launches ----
int glgym_plan_select(glgym_handle h, const glgym_plan_select_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_select: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_select", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    const bool wants_actions = a->best_action || a->best_sequence || a->mean_sequence;
    if (a->P < 1 || a->K < 1 || a->H < 1 || a->H > 65535 || (int64_t)a->P * a->K > INT32_MAX || !a->ret || !a->failed || !a->best_k ||
        !a->best_ret || (wants_actions && !a->actions) || (a->mean_sequence && !(a->temperature > 0.0 && std::isfinite(a->temperature))))
        return refuse("glgym_plan_select: bad arguments (P, K, H < 1, H > 65 535, null pointer, action outputs without actions, or mean_sequence "
                      "without a finite temperature > 0)");
    // the kernel multiplies by 1 / temperature: at 2^-1024 and below that is +inf and the best candidate's own (ret - max) * inf = 0 * inf a NaN
    if (a->mean_sequence && !std::isfinite(1.0 / a->temperature))
        return refuse("glgym_plan_select: temperature is too small (1 / temperature is not finite: it must be above 2^-1024, about 5.6e-309)");
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(plan_select_kernel, dim3(a->P), dim3(WAVE), 0, st, *a);
    HIPCHK(hipGetLastError());
    if (a->mean_sequence) {
        hipLaunchKernelGGL(plan_mean_kernel, dim3(a->P, a->H), dim3(WAVE), 0, st, *a);
        HIPCHK(hipGetLastError());
    }
    return GLGYM_OK;
}

// the cross-entropy method's stages (gl_cem.hpp): every check that needs no device memory happens here, before anything is launched
int glgym_plan_sample(glgym_handle h, const glgym_plan_sample_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_sample: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_sample", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->P < 1 || a->K < 1 || a->H < 1 || (int64_t)a->P * a->K > INT32_MAX - 255 || !a->mean || !a->std || !a->actions ||
        !(a->beta >= 0.0 && a->beta < 1.0) || a->carry < 0 ||
        (a->carry > 0 && (!a->prev_actions || !a->prev_elite_k || !a->prev_n_elite || a->prev_E < a->carry || a->prev_actions == a->actions)))
        return refuse("glgym_plan_sample: bad arguments (P, K, H < 1, null pointer, beta outside [0, 1), carry < 0, or with carry > 0: a missing "
                      "prev_ member, carry > prev_E, or prev_actions == actions -- sample into the other of two blocks)");
    DeviceGuard dev_guard(h);
    hipLaunchKernelGGL(plan_sample_kernel, dim3((unsigned)(((int64_t)a->P * a->K + WAVE - 1) / WAVE)), dim3(SAMPLE_WAVES * WAVE), 0, (hipStream_t)stream, *a);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_plan_elites(glgym_handle h, const glgym_plan_elites_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_elites: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_elites", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->P < 1 || a->K < 1 || a->E < 1 || a->E > a->K || (int64_t)a->P * a->K > INT32_MAX - 255 || !a->ret || !a->failed || !a->elite_k ||
        !a->n_elite)
        return refuse("glgym_plan_elites: bad arguments (P, K < 1, E outside 1..K, or null pointer)");
    DeviceGuard dev_guard(h);
    const int n_chunks = (a->K + glcem::CHUNK - 1) / glcem::CHUNK;
    hipLaunchKernelGGL(plan_elites_kernel, dim3((unsigned)((int64_t)a->P * n_chunks)), dim3(glcem::TILE), 0, (hipStream_t)stream, *a, n_chunks);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_plan_refit(glgym_handle h, const glgym_plan_refit_args* a, void* stream)
{
    if (!h || !a) { g_err = "glgym_plan_refit: null handle / arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_refit", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->P < 1 || a->K < 1 || a->H < 1 || a->H > 65535 || a->E < 1 || a->E > a->K || (int64_t)a->P * a->K > INT32_MAX - 255 ||
        !a->actions || !a->elite_k || !a->n_elite || !a->mean || !a->std || !a->mean_out || !a->std_out ||
        !(a->alpha >= 0.0 && a->alpha < 1.0) || !(a->min_std >= 0.0 && std::isfinite(a->min_std)))
        return refuse("glgym_plan_refit: bad arguments (P, K, H < 1, H > 65 535, E outside 1..K, null pointer, alpha outside [0, 1), or min_std "
                      "negative or not finite)");
    DeviceGuard dev_guard(h);
    hipLaunchKernelGGL(plan_refit_kernel, dim3(a->P, a->H), dim3(WAVE), 0, (hipStream_t)stream, *a);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

// the evolution strategy's stages (gl_es.hpp): checked before the handle is looked at, one text per mistake
static bool es_shape_ok(const char* who, int32_t P, int32_t K, int32_t H)
{
    const std::string w(who);
    if (P < 1 || H < 1) { g_err = w + ": P or H < 1"; return false; }
    if (K < 2) { g_err = w + ": K < 2 (a population is at least one mirrored pair)"; return false; }
    if (K % 2) { g_err = w + ": K is odd (mirrored sampling draws pairs)"; return false; }
    if ((int64_t)P * K > INT32_MAX - 255) { g_err = w + ": P * K past INT32_MAX - 255 (the lane indices would wrap)"; return false; }
    if (H > 65535) { g_err = w + ": H > 65 535"; return false; }
    return true;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int glgym_plan_es_sample(glgym_handle h, const glgym_plan_es_sample_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_es_sample: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_es_sample", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (!es_shape_ok("glgym_plan_es_sample", a->P, a->K, a->H)) return GLGYM_EINVAL;
    if (!a->mean || !a->std || !a->actions) { g_err = "glgym_plan_es_sample: null mean, std or actions"; return GLGYM_EINVAL; }
    if (!aligned16(a->actions)) { g_err = "glgym_plan_es_sample: actions is not 16-byte aligned"; return GLGYM_EINVAL; }
    if (!h) { g_err = "glgym_plan_es_sample: null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    const int64_t n_pair = (int64_t)a->P * (a->K / 2);
    hipLaunchKernelGGL(plan_es_sample_kernel, dim3((unsigned)((n_pair + WAVE - 1) / WAVE), (a->H + SAMPLE_WAVES - 1) / SAMPLE_WAVES), dim3(SAMPLE_WAVES * WAVE), 0, (hipStream_t)stream, *a);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_plan_es_utilities(glgym_handle h, const glgym_plan_es_utilities_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_es_utilities: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_es_utilities", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (!es_shape_ok("glgym_plan_es_utilities", a->P, a->K, 1)) return GLGYM_EINVAL;
    if (!a->ret || !a->failed || !a->u || !a->n_adm) { g_err = "glgym_plan_es_utilities: null ret, failed, u or n_adm"; return GLGYM_EINVAL; }
    if (!h) { g_err = "glgym_plan_es_utilities: null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    const int n_chunks = (a->K + glcem::CHUNK - 1) / glcem::CHUNK;
    hipLaunchKernelGGL(plan_es_utilities_kernel, dim3((unsigned)((int64_t)a->P * n_chunks)), dim3(glcem::TILE), 0, (hipStream_t)stream, *a, n_chunks);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_plan_es_update(glgym_handle h, const glgym_plan_es_update_args* a, void* stream)
{
    const char* who = "glgym_plan_es_update";
    const auto refuse = [&](const char* why) { g_err = std::string(who) + ": " + why; return (int)GLGYM_EINVAL; };
    if (!a) return refuse("null arguments");
    if (!plan_size_ok(who, a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (!es_shape_ok(who, a->P, a->K, a->H)) return GLGYM_EINVAL;
    if (a->optimizer != GLGYM_ES_SGD && a->optimizer != GLGYM_ES_ADAM) return refuse("optimizer is not GLGYM_ES_SGD or GLGYM_ES_ADAM");
    if (!a->actions || !a->u || !a->n_adm || !a->mean || !a->std || !a->mean_out || !a->std_out)
        return refuse("null actions, u, n_adm, mean, std, mean_out or std_out");
    if (!aligned16(a->actions) || !aligned16(a->u)) return refuse("actions or u is not 16-byte aligned");
    if (!(a->lr >= 0.0) || !std::isfinite(a->lr)) return refuse("lr negative or not finite");
    if (!(a->lr_std >= 0.0) || !std::isfinite(a->lr_std)) return refuse("lr_std negative or not finite");
    if (!(a->std_decay > 0.0) || !std::isfinite(a->std_decay)) return refuse("std_decay not finite or not > 0");
    if (!(a->min_std >= 0.0) || !std::isfinite(a->max_std) || !(a->min_std <= a->max_std))
        return refuse("min_std negative, max_std not finite, or min_std > max_std");
    if (a->t_index == 0) return refuse("t_index = 0 (the step count starts at 1)");
    if (a->optimizer == GLGYM_ES_ADAM) {
        if (!(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0)) return refuse("beta1 or beta2 outside [0, 1)");
        if (!(a->eps > 0.0) || !std::isfinite(a->eps)) return refuse("eps not finite or not > 0");
        if (!a->m1 || !a->m2) return refuse("GLGYM_ES_ADAM without m1 or m2");
    }
    if (!h) return refuse("null handle");
    DeviceGuard dev_guard(h);
    hipLaunchKernelGGL(plan_es_update_kernel, dim3(a->P, a->H), dim3(WAVE), 0, (hipStream_t)stream, *a);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

// the CMA-ES stages (gl_cma.hpp): checked before the handle is looked at, one text per mistake
static bool cma_shape_ok(const char* who, int32_t P, int32_t K, int32_t N)
{
    const std::string w(who);
    if (P < 1 || K < 1) { g_err = w + ": P or K < 1"; return false; }
    if (N < 1 || N > GLGYM_CMA_NMAX) { g_err = w + ": N outside 1..GLGYM_CMA_NMAX = " + std::to_string(GLGYM_CMA_NMAX); return false; }
    if ((int64_t)P * K > INT32_MAX - 255) { g_err = w + ": P * K past INT32_MAX - 255 (the lane indices would wrap)"; return false; }
    return true;
}

int glgym_plan_cma_sample(glgym_handle h, const glgym_plan_cma_sample_args* a, void* stream)
{
    const char* who = "glgym_plan_cma_sample";
    if (!a) { g_err = std::string(who) + ": null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok(who, a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (!cma_shape_ok(who, a->P, a->K, a->N)) return GLGYM_EINVAL;
    if (!a->mean || !a->sigma || !a->chol || !a->theta) { g_err = std::string(who) + ": null mean, sigma, chol or theta"; return GLGYM_EINVAL; }
    if (!h) { g_err = std::string(who) + ": null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    const int n_chunks = (a->K + CMA_THREADS - 1) / CMA_THREADS;
    hipLaunchKernelGGL(plan_cma_sample_kernel, dim3((unsigned)((int64_t)a->P * n_chunks)), dim3(CMA_THREADS), 0, (hipStream_t)stream, *a, n_chunks);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_plan_cma_update(glgym_handle h, const glgym_plan_cma_update_args* a, void* stream)
{
    const char* who = "glgym_plan_cma_update";
    const auto refuse = [&](const std::string& why) { g_err = std::string(who) + ": " + why; return (int)GLGYM_EINVAL; };
    if (!a) return refuse("null arguments");
    if (!plan_size_ok(who, a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (!cma_shape_ok(who, a->P, a->K, a->N)) return GLGYM_EINVAL;
    if (a->E < 1 || a->E > a->K) return refuse("E outside 1..K");
    if (!a->theta || !a->elite_k || !a->n_elite || !a->w || !a->w_dev || !a->mean || !a->sigma || !a->cov || !a->chol || !a->p_sigma ||
        !a->p_c || !a->status)
        return refuse("null theta, elite_k, n_elite, w, w_dev, mean, sigma, cov, chol, p_sigma, p_c or status");
    const struct { const char* name; double v; } consts[] = {{"mu_eff", a->mu_eff}, {"c_sigma", a->c_sigma}, {"d_sigma", a->d_sigma},
        {"c_c", a->c_c}, {"c_1", a->c_1}, {"c_mu", a->c_mu}, {"chi_n", a->chi_n}, {"min_sigma", a->min_sigma}, {"max_sigma", a->max_sigma}};
    for (const auto& c : consts)
        if (!std::isfinite(c.v)) return refuse(std::string(c.name) + " is not finite");
    for (int32_t e = 0; e < a->E; ++e) {
        if (!std::isfinite(a->w[e])) return refuse("weight " + std::to_string(e) + " is not finite");
        if (a->w[e] < 0.0) return refuse("weight " + std::to_string(e) + " is negative");
    }
    if (a->c_sigma < 0.0 || a->c_sigma > 1.0) return refuse("c_sigma outside [0, 1]");
    if (a->c_c < 0.0 || a->c_c > 1.0) return refuse("c_c outside [0, 1]");
    if (a->c_1 < 0.0 || a->c_1 > 1.0) return refuse("c_1 outside [0, 1]");
    if (a->c_mu < 0.0 || a->c_mu > 1.0) return refuse("c_mu outside [0, 1]");
    if (a->c_1 + a->c_mu > 1.0) return refuse("c_1 + c_mu > 1");
    if (!(a->d_sigma > 0.0)) return refuse("d_sigma not > 0");
    if (!(a->chi_n > 0.0)) return refuse("chi_n not > 0");
    if (!(a->mu_eff > 0.0)) return refuse("mu_eff not > 0");
    if (a->min_sigma < 0.0 || a->min_sigma > a->max_sigma) return refuse("min_sigma negative or > max_sigma");
    if (a->t_index == 0) return refuse("t_index = 0 (the generation count starts at 1)");
    if (!h) return refuse("null handle");
    DeviceGuard dev_guard(h);
    hipLaunchKernelGGL(plan_cma_update_kernel, dim3(a->P), dim3(CMA_THREADS), 0, (hipStream_t)stream, *a);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

int glgym_plan_aggregate(glgym_handle h, const glgym_plan_aggregate_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_aggregate: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_aggregate", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->J < 1 || a->S < 1 || a->S > 256 || a->m < 1 || a->m > a->S || (int64_t)a->J * a->S > INT32_MAX || !a->ret || !a->failed ||
        !a->ret_cand || !a->failed_cand || (a->viol_cand && (!a->viol || (int64_t)a->ld < (int64_t)a->J * a->S || a->ld_cand < a->J)) ||
        (a->steps_cand && !a->n_steps))
        return refuse("glgym_plan_aggregate: bad arguments (J, S < 1, S > 256, m outside 1 .. S, J*S > INT32_MAX, null pointer, or with viol_cand: "
                      "ld < J*S or ld_cand < J)");
    if (!h) { g_err = "glgym_plan_aggregate: null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    hipLaunchKernelGGL(plan_aggregate_kernel, dim3((unsigned)a->J), dim3(WAVE), 0, (hipStream_t)stream, *a);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

// constrained ranking (gl_constr.hpp).  As above, the arguments are checked before the handle is looked at.
int glgym_plan_constrain(glgym_handle h, const glgym_plan_constrain_args* a, void* stream)
{
    if (!a) { g_err = "glgym_plan_constrain: null arguments"; return GLGYM_EINVAL; }
    if (!plan_size_ok("glgym_plan_constrain", a->struct_size, sizeof *a)) return GLGYM_EINVAL;
    if (a->P < 1 || a->O < 1 || a->K < 1 || a->S < 1 || (int64_t)a->P * a->O > INT32_MAX || (int64_t)a->P * a->O * a->K > INT32_MAX ||
        (int64_t)a->P * a->O * a->K * a->S > INT32_MAX || (int64_t)a->ld < (int64_t)a->P * a->O * a->K * a->S)
        return refuse("glgym_plan_constrain: bad shape (P, O, K, S < 1, P*O*K*S > INT32_MAX, or ld < P*O*K*S)");
    const int64_t R = (int64_t)a->O * a->S, J = (int64_t)a->P * a->K;
    if ((a->per_step != 0 && a->per_step != 1) || a->n_allow < 0 || a->n_allow > R ||
        (a->mode != GLGYM_CONSTRAIN_PENALTY && a->mode != GLGYM_CONSTRAIN_FEASIBLE_FIRST))
        return refuse("glgym_plan_constrain: bad arguments (per_step not 0 | 1, n_allow outside 0 .. O*S, or an unknown mode)");
    for (int i = 0; i < 3; ++i)
        if (!(a->budget[i] >= 0.0) || !(a->weight[i] >= 0.0) || !std::isfinite(a->weight[i]))
            return refuse("glgym_plan_constrain: every budget must be >= 0 or +inf (not NaN), every weight finite and >= 0");
    if (!(a->rho >= 0.0) || !std::isfinite(a->rho)) { g_err = "glgym_plan_constrain: rho must be finite and >= 0"; return GLGYM_EINVAL; }
    if (!a->ret_cand || !a->failed_cand || !a->viol || !a->score || !a->failed_out || (a->per_step && !a->n_steps))
        return refuse("glgym_plan_constrain: null pointer (ret_cand, failed_cand, viol, score, failed_out, or n_steps with per_step)");
    const uintptr_t s0 = (uintptr_t)a->score, r0 = (uintptr_t)a->ret_cand, bytes = (uintptr_t)J * sizeof(double);
    if (s0 < r0 + bytes && r0 < s0 + bytes)
        return refuse("glgym_plan_constrain: score overlaps ret_cand (the stage reads the returns after it has begun to write the scores)");
    if (!h) { g_err = "glgym_plan_constrain: null handle"; return GLGYM_EINVAL; }
    DeviceGuard dev_guard(h);
    hipStream_t st = (hipStream_t)stream;
    glconstr::Spec sp{a->O, a->K, a->S, a->per_step, {a->budget[0], a->budget[1], a->budget[2]}, {a->weight[0], a->weight[1], a->weight[2]}};
    if (R <= glconstr::SMALL_R)
        hipLaunchKernelGGL(plan_constrain_few_runs_kernel, dim3((unsigned)((J + 255) / 256)), dim3(256), 0, st, *a, sp, (int)J);
    else
        hipLaunchKernelGGL(plan_constrain_candidates_kernel, dim3((unsigned)((J + CONSTR_WAVES - 1) / CONSTR_WAVES)), dim3(CONSTR_WAVES * WAVE), 0,
                           st, *a, sp, (int)J);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(plan_constrain_groups_kernel, dim3((unsigned)a->P), dim3(glconstr::GROUP_THREADS), 0, st, *a);
    HIPCHK(hipGetLastError());
    return GLGYM_OK;
}

}  // extern "C"
