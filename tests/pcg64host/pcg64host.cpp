// Host (g++) instantiation of the product's csrc/gl_pcg64.hpp -- tests only (tests/test_np_stream_host.py).  A stream is the five
// uint64 words of the C ABI's SoA buffer with ld = 1: state low / high, increment low / high, buffer word.
#include <cstdint>

#include "gl_pcg64.hpp"

using glpcg::Pcg64;

namespace {
Pcg64 get(const uint64_t* s)
{
    Pcg64 g;
    g.load(s, 1, 0);
    return g;
}
}  // namespace

extern "C" {

void pcg64host_uint64(uint64_t* s, int n, uint64_t* out)
{
    Pcg64 g = get(s);
    for (int i = 0; i < n; ++i) out[i] = g.next_uint64();
    g.store(s, 1, 0);
}

void pcg64host_uint32(uint64_t* s, int n, uint32_t* out)
{
    Pcg64 g = get(s);
    for (int i = 0; i < n; ++i) out[i] = g.next_uint32();
    g.store(s, 1, 0);
}

void pcg64host_double(uint64_t* s, int n, double* out)
{
    Pcg64 g = get(s);
    for (int i = 0; i < n; ++i) out[i] = g.next_double();
    g.store(s, 1, 0);
}

void pcg64host_uniform(uint64_t* s, double lo, double hi, int n, double* out)
{
    Pcg64 g = get(s);
    for (int i = 0; i < n; ++i) out[i] = glpcg::uniform(g, lo, hi);
    g.store(s, 1, 0);
}

uint32_t pcg64host_bounded(uint64_t* s, uint64_t n)
{
    Pcg64 g = get(s);
    const uint32_t v = g.bounded(n);
    g.store(s, 1, 0);
    return v;
}

void pcg64host_advance(uint64_t* s, uint64_t k)
{
    Pcg64 g = get(s);
    g.advance(glpcg::advance_consts(k));
    g.store(s, 1, 0);
}

// the compile-time constants of the 34 draws of an env-step, as the kernel uses them
void pcg64host_advance_step(uint64_t* s)
{
    constexpr glpcg::AdvanceConsts jump = glpcg::advance_consts(glpcg::NDRAW_STEP);
    Pcg64 g = get(s);
    g.advance(jump);
    g.store(s, 1, 0);
}

void pcg64host_crop_block(uint64_t* s, const float* p0, double scale, float* out)
{
    Pcg64 g = get(s);
    glpcg::crop_block(g, p0, scale, out);
    g.store(s, 1, 0);
}

}  // extern "C"
