// gl_mlp.hpp -- a small MLP policy for ONE row with that row's own weights (include/glgym.h glgym_policy_rows,
// glgym_plan_rollout_policy), for host and device code alike:
//   net_error       what is wrong with a glgym_mlp_net (NULL: nothing), checked on the host before anything is launched
//   layer_in / layer_out / n_params
//                   the shape of layer l = 0 .. n_hidden (the last one has the six actions as outputs) and D, the length of the flat
//                   parameter vector: layer by layer, weight [out][in] row-major, then bias [out]
//   theta_at        component i of the flat parameter vector of one row of the block theta [Ht][J][6]: theta[i / 6][j][i % 6]
//   dot             one output's sum over a tile of inputs, the weights fetched plane by plane, 6 consecutive floats at a time.  Every
//                   index it computes is the same for all lanes of a wavefront (the net is shared, only the row differs): scalar
//                   registers, scalar branches.
//   param           w_i = scale[g] * theta_i, one float32 product
//   normalise       o_i = fmin(fmax((obs_i - mean_i) * inv_std_i, -clip_obs), clip_obs), or obs_i without statistics
//   activate        relu: fmaxf(z, 0) (a NaN reads as 0) | tanhf | silu: z / (1 + expf(-z)), expf and IEEE division
//   squash          clip: fminf(fmaxf(z, -1), 1) | the same clip on tanhf(z).  fmaxf returns its other operand when one is a NaN, so
//                   a NaN reads as -1.  This is deliberate: the actions of a candidate go straight into the step kernel, and a NaN
//                   action must never reach it.
//   forward         the net of one row.  All float32, products and sums rounded separately (no fused multiply-add), so that NumPy
//                   restates it exactly: z_o = bias_o, then for i ascending z_o = z_o + w_oi * a_i.  Activations pass through a
//                   caller-supplied store of two buffers of `rows` floats (the kernel: LDS laid out [neuron][lane]; the host: two
//                   arrays); an input wider than TILE is staged in tiles of TILE, the partial sums kept in the output buffer, which
//                   leaves the order of the additions as it is.
//   policy_row      the row of theta that child c reads, by row mode
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "glgym.h"
#include "gl_plan.hpp"

namespace glmlp {

constexpr int NU = 6;
constexpr int MAX_HIDDEN = 3, MAX_WIDTH = 64, MAX_IN = 1024, MAX_GROUPS = 2 * (MAX_HIDDEN + 1);
constexpr int TILE = 64;                          // inputs staged at a time
constexpr int64_t MAX_HT = 65535;                 // glgym_plan_refit's limit on the planes of a block
static_assert(sizeof(((glgym_mlp_net*)nullptr)->width) == MAX_HIDDEN * sizeof(int32_t) &&
              sizeof(((glgym_mlp_net*)nullptr)->scale) == MAX_GROUPS * sizeof(float), "glgym_mlp_net: three widths, eight scales");

GLPLAN_HD int layer_in(const glgym_mlp_net& n, int l) { return l == 0 ? n.in_dim : n.width[l - 1]; }
GLPLAN_HD int layer_out(const glgym_mlp_net& n, int l) { return l >= MAX_HIDDEN || l == n.n_hidden ? NU : n.width[l]; }

// D.  Only for a net whose sizes net_error accepts
inline int64_t n_params(const glgym_mlp_net& n)
{
    int64_t d = 0;
    for (int l = 0; l <= n.n_hidden; ++l) d += (int64_t)layer_out(n, l) * (layer_in(n, l) + 1);
    return d;
}

// floats per activation buffer: the widest layer, a tile of inputs, or the six outputs
inline int buffer_rows(const glgym_mlp_net& n)
{
    int r = n.in_dim < TILE ? n.in_dim : TILE;
    if (r < NU) r = NU;
    for (int l = 0; l < n.n_hidden; ++l)
        if (n.width[l] > r) r = n.width[l];
    return r;
}

// NULL, or the reason a net is refused
inline const char* net_error(const glgym_mlp_net* n)
{
    if (!n) return "null net";
    if (n->in_dim < 1 || n->in_dim > MAX_IN) return "in_dim outside 1..1024";
    if (n->n_hidden < 0 || n->n_hidden > MAX_HIDDEN) return "n_hidden outside 0..3";
    for (int l = 0; l < n->n_hidden; ++l)
        if (n->width[l] < 1 || n->width[l] > MAX_WIDTH) return "a hidden width outside 1..64";
    if (n->activation != GLGYM_MLP_RELU && n->activation != GLGYM_MLP_TANH && n->activation != GLGYM_MLP_SILU)
        return "activation is not GLGYM_MLP_RELU, _TANH or _SILU";
    if (n->squash != GLGYM_MLP_SQUASH_CLIP && n->squash != GLGYM_MLP_SQUASH_TANH) return "squash is not GLGYM_MLP_SQUASH_CLIP or _TANH";
    for (int g = 0; g < 2 * (n->n_hidden + 1); ++g)
        if (!std::isfinite(n->scale[g]) || !(n->scale[g] > 0.0f)) return "a scale that is not finite and > 0";
    if ((!n->mean) != (!n->inv_std)) return "exactly one of mean / inv_std is NULL";
    if (n->mean && (!std::isfinite(n->clip_obs) || !(n->clip_obs > 0.0f))) return "clip_obs is not finite and > 0";
    if ((n_params(*n) + NU - 1) / NU > MAX_HT) return "more than 65 535 planes of parameters";
    return nullptr;
}

// component i of the flat parameter vector of the row that starts at theta_row; plane = floats from one plane of theta to the next
GLPLAN_HD float theta_at(const float* theta_row, size_t plane, int64_t i) { return theta_row[(size_t)(i / NU) * plane + (size_t)(i % NU)]; }

GLPLAN_HD float param(float scale, float theta)
{
#pragma clang fp contract(off)
    return scale * theta;
}

GLPLAN_HD float normalise(const glgym_mlp_net& n, float obs, int i)
{
#pragma clang fp contract(off)
    if (!n.mean) return obs;
    const float d = obs - n.mean[i];
    const float s = d * n.inv_std[i];
    return fminf(fmaxf(s, -n.clip_obs), n.clip_obs);
}

GLPLAN_HD float activate(int kind, float z)
{
#pragma clang fp contract(off)
    if (kind == GLGYM_MLP_RELU) return fmaxf(z, 0.0f);      // a NaN reads as 0
    if (kind == GLGYM_MLP_TANH) return tanhf(z);
    const float e = expf(-z);
    const float d = 1.0f + e;
    return z / d;
}

GLPLAN_HD float squash(int kind, float z)
{
    const float v = kind == GLGYM_MLP_SQUASH_TANH ? tanhf(z) : z;
    return fminf(fmaxf(v, -1.0f), 1.0f);                     // a NaN reads as -1: see the head of this file
}

GLPLAN_HD float mac(float z, float w, float a)
{
#pragma clang fp contract(off)
    const float prod = w * a;
    return z + prod;
}

// z + sum over k < tn of w_k * a_k, k ascending: w_k = component i0 + k of the row, a_k = buf(src, k).  The weights are fetched a
// GROUP of planes at a time, each plane as its 6 consecutive floats whichever of them this segment uses (a plane of the block is
// complete, padding included; what the segment does not use is not looked at), so that GROUP * 6 loads are in flight before the first
// product waits for one.  Which entries are used is the same for every row, so on the device the tests are scalar branches.
constexpr int GROUP = 4;
template <class Buf>
GLPLAN_HD float dot(float z, float sw, const float* theta_row, size_t plane, int64_t i0, int tn, Buf&& buf, int src)
{
    const float* p = theta_row + (size_t)(i0 / NU) * plane;
    for (int k = -(int)(i0 % NU); k < tn; k += GROUP * NU, p += GROUP * plane) {      // k: the input that entry 0 of plane p multiplies
        float c[GROUP][NU];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int g = 0; g < GROUP; ++g)
            if (k + g * NU < tn) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
                for (int e = 0; e < NU; ++e) c[g][e] = p[(size_t)g * plane + e];
            }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int g = 0; g < GROUP; ++g) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int e = 0; e < NU; ++e) {
                const int kk = k + g * NU + e;
                if (kk >= 0 && kk < tn) z = mac(z, param(sw, c[g][e]), buf(src, kk));
            }
        }
    }
    return z;
}

// The six actions of one row.  obs_row [in_dim]; theta_row = theta + j * 6, plane = J * 6.  buf(which, k): a reference to float k <
// buffer_rows(n) of activation buffer `which` (0 | 1) of THIS row.
template <class Buf>
GLPLAN_HD void forward(const glgym_mlp_net& n, const float* obs_row, const float* theta_row, size_t plane, Buf&& buf, float action[NU])
{
    int64_t off = 0;                              // flat index of the layer's first weight
    int src = 0;                                  // the buffer that holds the layer's inputs; layer 0 stages its own
    // unrolled over the at most four layers on the device, so that width[] and scale[] are indexed by constants: the net stays in
    // scalar registers, not in a stack copy
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int l = 0; l <= MAX_HIDDEN; ++l) {
        if (l > n.n_hidden) break;
        const int in = layer_in(n, l), out = layer_out(n, l), dst = 1 - src;
        const float sw = n.scale[2 * l], sb = n.scale[2 * l + 1];
        const bool last = l == n.n_hidden;
        for (int t0 = 0; t0 < in; t0 += TILE) {                      // hidden layers: one tile (width <= TILE)
            const int tn = in - t0 < TILE ? in - t0 : TILE;
            if (l == 0)
                for (int k = 0; k < tn; ++k) buf(src, k) = normalise(n, obs_row[t0 + k], t0 + k);
            for (int o = 0; o < out; ++o) {
                float z = t0 == 0 ? param(sb, theta_at(theta_row, plane, off + (int64_t)out * in + o)) : buf(dst, o);
                z = dot(z, sw, theta_row, plane, off + (int64_t)o * in + t0, tn, buf, src);
                buf(dst, o) = (t0 + tn < in || last) ? z : activate(n.activation, z);
            }
        }
        off += (int64_t)out * (in + 1);
        src = dst;
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < NU; ++i) action[i] = squash(n.squash, buf(src, i));
}

// the row of theta that child c reads
GLPLAN_HD int policy_row(int c, int S, int J, int mode)
{
    const int cand = S > 1 ? c / S : c;
    return mode == GLGYM_POLICY_ROW_CANDIDATE ? cand % J : cand;
}

}  // namespace glmlp
