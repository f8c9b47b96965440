// gl_bdf_wave.hpp -- the team of gl_bdf.hpp on one 64-lane wavefront, independent of the model: the butterfly reductions, the
// register solve and the lane layout of a finite-difference Jacobian, over a right-hand side given as a functor.
//
//   Rhs::operator()(const double xs[28], double k[28]) const      k = f(xs), callable from any lane
//
// Lane i < 28 owns state i in the vector work.  A trajectory evaluation of the right-hand side runs in lane 0; the 28 columns of a
// Jacobian (and the base point of a re-evaluated one, in lane 28) run side by side from the same call site, so a Jacobian costs one
// right-hand-side latency.  glgym_bdf.hip instantiates the team with the model's right-hand side and is its only user in the library.
#pragma once
#include <hip/hip_runtime.h>

#include "gl_bdf.hpp"

namespace glbdf {

constexpr int WAVE = 64;

__device__ __forceinline__ double bdf_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// v of lane k (k compile-time after unrolling): two v_readlane, no LDS round trip
__device__ __forceinline__ double bdf_lane(double v, int k)
{
    const long long bits = __double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)bits, k);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(bits >> 32), k);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

template <class Rhs> struct WaveTeam {
    static constexpr int width = WAVE;
    int ln;
    Rhs f;
    __device__ int lane() const { return ln; }
    __device__ double sum(double v) const { return bdf_wave_sum(v); }
    __device__ void sync() const { __syncthreads(); }
    // butterfly over (value, index): the largest value, the smallest index among equal values, in every lane
    __device__ void argmax(double& v, int& i) const
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(v, o, WAVE);
            const int oi = __shfl_xor(i, o, WAVE);
            if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
        }
    }
    // (I - c J) w = b: lane i holds w_i in a register; forward sweep in the serial order, back substitution as a column sweep
    // (w_k = w_k / U_kk final, then lanes i < k take U_ik w_k off).  Rows of lanes >= 28 mirror row 27 and are never stored.
    __device__ void lu_solve(BdfScratch& sh, double* b) const
    {
        const int ii = ln < NX ? ln : NX - 1;
        double w = b[sh.perm[ii]];
#pragma unroll
        for (int k = 0; k < NX - 1; ++k) {
            const double lik = sh.LU[ii * NX + k], wk = bdf_lane(w, k);
            if (ln > k) w -= lik * wk;
        }
#pragma unroll
        for (int k = NX - 1; k >= 0; --k) {
            const double uik = sh.LU[ii * NX + k], wk = bdf_lane(w, k) / sh.LU[k * NX + k];
            if (ln == k) w = wk;
            else if (ln < k) w -= uik * wk;
        }
        if (ln < NX) b[ln] = w;
        __syncthreads();
    }
    __device__ void eval1(const double* x, double* fx) const
    {
        if (ln == 0) {
            double xs[NX], k[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) xs[i] = x[i];
            f(xs, k);
#pragma unroll
            for (int i = 0; i < NX; ++i) fx[i] = k[i];
        }
        __syncthreads();
    }
    // lane j < 28: column j at x + dx_j e_j; lane 28 (need_f0): f0 = rhs(x) -- one call site, one right-hand-side latency
    __device__ void jac(const double* x, double* f0, bool need_f0, double* J) const
    {
        double k[NX], dxj = 1.0;
        if (ln < NX + (need_f0 ? 1 : 0)) {
            double xs[NX];
#pragma unroll
            for (int i = 0; i < NX; ++i) {
                const double xi = x[i];
                if (i == ln) { dxj = 1.4901161193847656e-8 * ::fmax(::fabs(xi), 1.0); xs[i] = xi + dxj; }
                else xs[i] = xi;
            }
            f(xs, k);
        }
        if (need_f0 && ln == NX) {
#pragma unroll
            for (int i = 0; i < NX; ++i) f0[i] = k[i];
        }
        __syncthreads();
        if (ln < NX) {
#pragma unroll
            for (int i = 0; i < NX; ++i) J[i * NX + ln] = (k[i] - f0[i]) / dxj;
        }
        __syncthreads();
    }
};

// The model's right-hand side at the row's constants (gl_model.hpp, the full right-hand side at every evaluation): the Rhs of the
// library's kernels.
struct ModelRhs {
    const glm::ModelConst<double>& m;
    const glm::CropConst<double>& cr;
    const glm::StepCoef<double>& s;
    __device__ void operator()(const double* xs, double* k) const { glm::rhs<double, true, false>(xs, s, m, cr, k); }
};

}  // namespace glbdf
