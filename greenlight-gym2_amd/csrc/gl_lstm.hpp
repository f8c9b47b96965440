// gl_lstm.hpp -- the scalar logic of the recurrent PPO stages (include/glgym.h glgym_lstm_cell, glgym_lstm_cell_grad, glgym_seq_batch), for
// host and device code alike: ONE (row, unit) of an LSTM step behind the two gate products, its backward pass, and where a sequence of a
// minibatch lies in a collector's [T][B] buffer.  tests/lstmhost/lstmhost.cpp instantiates it on the host: a lane is a pass of a loop.
//   forward         float32, every operation rounded on its own, in this order (gates in torch's order i, f, g, o):
//                     keep = start == NULL || start[row] == 0
//                     a_k  = keep ? gx_k + gh_k : gx_k          k = i, f, g, o         -- a select, never a product with 1 - start
//                     c0   = keep ? c_prev : 0
//                     i = (float)(1 / (1 + exp(-(double) a_i))), likewise f and o;  g = (float) tanh((double) a_g)
//                     c = f * c0 + i * g   (two products, one sum);  tc = (float) tanh((double) c);  h = o * tc
//                   The five activations are the only transcendentals; a host and a device libm differ in them by an ulp, so activations()
//                   is apart from finish(), and a host build may take the device's own activations as inputs.
//   backward        float32, from act = (i, f, g, o, tc) and c0 as above, no transcendental:
//                     do = dh * tc;  dct = dc + (dh * o) * (1 - tc * tc)
//                     da_i = (dct * g) * (i * (1 - i));  da_f = (dct * c0) * (f * (1 - f));  da_g = (dct * i) * (1 - g * g)
//                     da_o = do * (o * (1 - o))
//                     d_gx_k = da_k;  d_gh_k = keep ? da_k : 0;  d_c_prev = keep ? dct * f : 0
//   seq_of          sequence q in [0, (T / L) B) is chunk q / B of environment q % B; its step l is buffer row (chunk L + l) B + env.  The
//                   minibatch's sequences are positions of glppo::perm with N = (T / L) B and glppo's tag: L = 1 is glgym_ppo_batch.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "glgym.h"
#include "gl_ppo.hpp"

namespace glstm {

constexpr int BLOCK = 256;
constexpr int MAX_BLOCKS = 2048;                 // the cell kernels' grid cap: 8 blocks on each of 256 CUs; beyond it a lane strides
constexpr int MAX_H = 1024;
constexpr int MAX_STATE = 4;
constexpr int N_ACT = 5;                         // i, f, g, o, tc
enum { A_I = 0, A_F, A_G, A_O, A_TC };

GLPLAN_HD float sigmoid_of(float a)
{
#pragma clang fp contract(off)
    const double e = std::exp(-(double)a);
    const double d = 1.0 + e;
    return (float)(1.0 / d);
}

GLPLAN_HD float tanh_of(float a) { return (float)std::tanh((double)a); }

// the four pre-activations of a unit and the cell state it starts from
GLPLAN_HD void preact(bool keep, const float gx[4], const float gh[4], float c_prev, float a[4], float& c0)
{
#pragma clang fp contract(off)
    for (int k = 0; k < 4; ++k) a[k] = keep ? gx[k] + gh[k] : gx[k];
    c0 = keep ? c_prev : 0.0f;
}

// c from the four gates
GLPLAN_HD float cell_of(float i, float f, float g, float c0)
{
#pragma clang fp contract(off)
    const float p0 = f * c0;
    const float p1 = i * g;
    return p0 + p1;
}

GLPLAN_HD float hidden_of(float o, float tc)
{
#pragma clang fp contract(off)
    return o * tc;
}

// one (row, unit), libm included: act = (i, f, g, o, tc)
GLPLAN_HD void forward(bool keep, const float gx[4], const float gh[4], float c_prev, float act[N_ACT], float& c, float& h)
{
    float a[4], c0;
    preact(keep, gx, gh, c_prev, a, c0);
    act[A_I] = sigmoid_of(a[A_I]);
    act[A_F] = sigmoid_of(a[A_F]);
    act[A_G] = tanh_of(a[A_G]);
    act[A_O] = sigmoid_of(a[A_O]);
    c = cell_of(act[A_I], act[A_F], act[A_G], c0);
    act[A_TC] = tanh_of(c);
    h = hidden_of(act[A_O], act[A_TC]);
}

// one (row, unit) of the backward pass: da [4], and d_c_prev
GLPLAN_HD void backward(bool keep, float dh, float dc, const float act[N_ACT], float c_prev, float da[4], float& d_c_prev)
{
#pragma clang fp contract(off)
    const float i = act[A_I], f = act[A_F], g = act[A_G], o = act[A_O], tc = act[A_TC];
    const float c0 = keep ? c_prev : 0.0f;
    const float d_o = dh * tc;
    const float t0 = dh * o;
    const float t1 = tc * tc;
    const float t2 = 1.0f - t1;
    const float t3 = t0 * t2;
    const float dct = dc + t3;
    const float i1 = 1.0f - i;
    const float i2 = i * i1;
    const float i3 = dct * g;
    da[A_I] = i3 * i2;
    const float f1 = 1.0f - f;
    const float f2 = f * f1;
    const float f3 = dct * c0;
    da[A_F] = f3 * f2;
    const float g1 = g * g;
    const float g2 = 1.0f - g1;
    const float g3 = dct * i;
    da[A_G] = g3 * g2;
    const float o1 = 1.0f - o;
    const float o2 = o * o1;
    da[A_O] = d_o * o2;
    const float p = dct * f;
    d_c_prev = keep ? p : 0.0f;
}

// ---- the launch shape of the cell kernels: a lane takes V consecutive units of a row ---------------------------------------------------
GLPLAN_HD int n_blocks(int64_t n_lane)
{
    const int64_t c = (n_lane + BLOCK - 1) / BLOCK;
    return (int)(c < MAX_BLOCKS ? c : MAX_BLOCKS);
}

// ---- sequences -----------------------------------------------------------------------------------------------------------------------------
// first buffer row of sequence q: chunk q / B of environment q % B; step l is L0 + l * B
GLPLAN_HD uint32_t first_row(uint32_t q, uint32_t B, uint32_t L)
{
    const uint32_t chunk = q / B, env = q - chunk * B;
    return chunk * L * B + env;
}

}  // namespace glstm
