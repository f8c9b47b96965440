// gl_pcg64.hpp -- NumPy's default bit generator, PCG64 (O'Neill's PCG XSL-RR 128/64 with the default 128-bit multiplier), and the
// draws Generator makes from it, restated from the published algorithm for host and device code alike.
//
// One stream per environment reproduces what `np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))` returns, in order:
//   next_uint64   advance state = state * MULT + inc, then output XSL-RR of the NEW state
//   next_uint32   low half of a 64-bit draw first, the high half kept in NumPy's one-word buffer (has_uint32 / uinteger)
//   next_double   (next_uint64 >> 11) * 2^-53                      Generator.random / uniform
//   uniform       lo + (hi - lo) * next_double                     Generator.uniform(lo, hi): product and sum rounded separately
//   bounded(n)    Generator.choice(list of n) / integers(0, n):    nothing drawn for n == 1, otherwise Lemire's rejection method on
//                 buffered 32-bit draws (n <= 2^32).  next_uint64 does not clear the buffer: two choices use ONE 64-bit draw.
//   advance(k)    the state after k 64-bit draws, in O(1) from two 128-bit constants (advance_consts(k): a^k and 1 + a + .. + a^(k-1))
// The 128-bit state is a pair of 64-bit words; the products are 64 x 64 -> 128 from __umul64hi on the device (v_mul_hi_u32 chains,
// no library call) and unsigned __int128 on the host.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GLPCG_HD __host__ __device__ __forceinline__
#else
#define GLPCG_HD inline
#endif

namespace glpcg {

struct u128 {
    uint64_t lo, hi;
};

constexpr uint64_t MULT_HI = 0x2360ED051FC65DA4ull, MULT_LO = 0x4385DF649FCCF645ull;
constexpr int NDRAW_STEP = 34;          // uniform doubles per env-step: the crop block p[128..161] (noise.py:17-18)
constexpr int NWORD = 5;                // words of one stream in the SoA buffer: state lo / hi, inc lo / hi, buffer word

// high half of a 64 x 64 product from 32-bit pieces: for constant expressions (advance_consts) on either side
constexpr uint64_t mulhi_c(uint64_t a, uint64_t b)
{
    const uint64_t a0 = a & 0xFFFFFFFFull, a1 = a >> 32, b0 = b & 0xFFFFFFFFull, b1 = b >> 32;
    const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFull) + (p10 & 0xFFFFFFFFull);
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

GLPCG_HD uint64_t mulhi(uint64_t a, uint64_t b)
{
#if defined(__HIP_DEVICE_COMPILE__) || defined(__CUDA_ARCH__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

constexpr u128 mul_c(u128 a, u128 b) { return {a.lo * b.lo, mulhi_c(a.lo, b.lo) + a.hi * b.lo + a.lo * b.hi}; }
constexpr u128 add_c(u128 a, u128 b) { return {a.lo + b.lo, a.hi + b.hi + ((a.lo + b.lo) < a.lo ? 1u : 0u)}; }

GLPCG_HD u128 mul(u128 a, u128 b) { return {a.lo * b.lo, mulhi(a.lo, b.lo) + a.hi * b.lo + a.lo * b.hi}; }
GLPCG_HD u128 add(u128 a, u128 b)
{
    const uint64_t lo = a.lo + b.lo;
    return {lo, a.hi + b.hi + (lo < a.lo ? 1u : 0u)};
}

// state after k draws = mult * state + plus * inc with mult = a^k, plus = 1 + a + ... + a^(k-1)  (mod 2^128)
struct AdvanceConsts {
    u128 mult, plus;
};

constexpr AdvanceConsts advance_consts(uint64_t k)
{
    u128 acc_mult{1, 0}, acc_plus{0, 0}, cur_mult{MULT_LO, MULT_HI}, cur_plus{1, 0};
    while (k > 0) {                     // Brown, "Random number generation with arbitrary strides" (the PCG library's advance)
        if (k & 1) {
            acc_mult = mul_c(acc_mult, cur_mult);
            acc_plus = add_c(mul_c(acc_plus, cur_mult), cur_plus);
        }
        cur_plus = mul_c(add_c(cur_mult, u128{1, 0}), cur_plus);
        cur_mult = mul_c(cur_mult, cur_mult);
        k >>= 1;
    }
    return {acc_mult, acc_plus};
}

struct Pcg64 {
    u128 state, inc;
    uint32_t has_uint32, uinteger;

    GLPCG_HD void step() { state = add(mul(state, u128{MULT_LO, MULT_HI}), inc); }

    GLPCG_HD uint64_t next_uint64()
    {
        step();
        const uint64_t v = state.hi ^ state.lo;
        const unsigned r = (unsigned)(state.hi >> 58);
        return (v >> r) | (v << ((64u - r) & 63u));
    }

    GLPCG_HD uint32_t next_uint32()
    {
        if (has_uint32) {
            has_uint32 = 0;
            return uinteger;
        }
        const uint64_t n = next_uint64();
        has_uint32 = 1;
        uinteger = (uint32_t)(n >> 32);
        return (uint32_t)n;
    }

    GLPCG_HD double next_double() { return (double)(next_uint64() >> 11) * (1.0 / 9007199254740992.0); }

    // an integer in [0, n), 1 <= n <= 2^32: the index Generator.choice(a) takes from a list of n
    GLPCG_HD uint32_t bounded(uint64_t n)
    {
        if (n <= 1) return 0;
        const uint32_t rng = (uint32_t)(n - 1);
        if (rng == 0xFFFFFFFFu) return next_uint32();
        uint64_t m = (uint64_t)next_uint32() * n;
        uint32_t leftover = (uint32_t)m;
        if (leftover < n) {
            const uint32_t threshold = (uint32_t)((0xFFFFFFFFu - rng) % (uint32_t)n);
            while (leftover < threshold) {              // probability below n / 2^32 per draw
                m = (uint64_t)next_uint32() * n;
                leftover = (uint32_t)m;
            }
        }
        return (uint32_t)(m >> 32);
    }

    GLPCG_HD void advance(const AdvanceConsts& c) { state = add(mul(c.mult, state), mul(c.plus, inc)); }

    // the SoA stream buffer uint64 [5][ld] of the C ABI: buffer word = has_uint32 << 32 | uinteger
    GLPCG_HD void load(const uint64_t* s, size_t ld, size_t b)
    {
        state = {s[b], s[ld + b]};
        inc = {s[2 * ld + b], s[3 * ld + b]};
        const uint64_t w = s[4 * ld + b];
        has_uint32 = (uint32_t)(w >> 32) & 1u;
        uinteger = (uint32_t)w;
    }
    // inc never changes after seeding: only the state and the buffer word go back
    GLPCG_HD void store(uint64_t* s, size_t ld, size_t b) const
    {
        s[b] = state.lo;
        s[ld + b] = state.hi;
        s[4 * ld + b] = ((uint64_t)has_uint32 << 32) | uinteger;
    }
};

// product and sum rounded separately, as NumPy's C and its float64 ufuncs do: no fused multiply-add
// (hipcc contracts a * b + c by default, and through __dmul_rn / __dadd_rn as well: the pragma takes the permission off these two
// operations wherever they are inlined; other compilers get a volatile temporary)
GLPCG_HD double mul_rn(double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
    return a * b;
#else
    volatile double p = a * b;
    return p;
#endif
}
GLPCG_HD double add_rn(double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
    return a + b;
#else
    volatile double s = a + b;
    return s;
#endif
}

GLPCG_HD double uniform(Pcg64& g, double lo, double hi) { return add_rn(lo, mul_rn(hi - lo, g.next_double())); }

// parametric_crop_uncertainty (noise.py:16-22) on a float32 parameter block: noise = uniform(-scale/2, scale/2, 34);
// p[128..161] += noise * p[128..161] evaluated in float64 and rounded to float32; p[144] = p[141] / p[142] in float32.
GLPCG_HD float crop_entry(Pcg64& g, float p0, double lo, double hi)
{
    const double noise = uniform(g, lo, hi), p = (double)p0;
    return (float)add_rn(p, mul_rn(noise, p));
}

// p0 / out: the 34 entries p[128..161]
GLPCG_HD void crop_block(Pcg64& g, const float* p0, double scale, float* out)
{
    const double lo = -scale / 2, hi = scale / 2;
    for (int i = 0; i < NDRAW_STEP; ++i) out[i] = crop_entry(g, p0[i], lo, hi);
    out[144 - 128] = out[141 - 128] / out[142 - 128];
}

}  // namespace glpcg
