// Host (g++) instantiation of the product's csrc/gl_step_select.hpp -- tests only (tests/test_step_select_host.py): the selection in
// batches, and the build list expanded into rows.
#include <cstring>

#include "gl_step_select.hpp"

using namespace glsel;

namespace {
void put(const StepBuild& b, int* o)
{
    o[0] = b.family; o[1] = b.f64; o[2] = b.crop; o[3] = b.def; o[4] = b.pipe; o[5] = b.sch; o[6] = b.epi; o[7] = b.occ;
}
}  // namespace

extern "C" {

// in: n rows of 15 ints, StepSelectIn's fields in their order; out: n rows of 11 ints: error (0/1), the build's 8 fields, grid, fused
void stepselect_batch(int n, const int* in, int* out)
{
    for (int r = 0; r < n; ++r, in += 15, out += 11) {
        const StepSelectIn s{in[0] != 0, in[1], in[2] != 0, in[3] != 0, in[4] != 0, in[5], in[6], in[7], in[8], in[9] != 0, in[10] != 0,
                             in[11] != 0, in[12], in[13] != 0};
        const StepChoice c = select_step(s);
        out[0] = c.error != nullptr;
        put(c.build, out + 1);
        out[9] = (int)c.grid; out[10] = c.fused;
    }
}

// the same rows; out: n rows of 3 ints: select_step(..).error is non-null, step_pipe_error(pipe, crop, scheme) is non-null, and the two
// agree (both null, or the same text)
void stepselect_pipe_error_batch(int n, const int* in, int* out)
{
    for (int r = 0; r < n; ++r, in += 15, out += 3) {
        const StepSelectIn s{in[0] != 0, in[1], in[2] != 0, in[3] != 0, in[4] != 0, in[5], in[6], in[7], in[8], in[9] != 0, in[10] != 0,
                             in[11] != 0, in[12], in[13] != 0};
        const char* sel = select_step(s).error;
        const char* own = step_pipe_error(s.pipe, s.crop, s.scheme);
        out[0] = sel != nullptr;
        out[1] = own != nullptr;
        out[2] = (sel && own) ? std::strcmp(sel, own) == 0 : sel == own;
    }
}

const char* stepselect_error_text()
{
    return select_step(StepSelectIn{false, RK4, true, true, false, 0, 0, 1, 1, false, false, false, 0, false}).error;
}

// the build list as rows of 8 ints (at most cap rows are written); returns the number of builds
int stepselect_builds(int* out, int cap)
{
    int n = 0;
    for (int sch = 0; sch < 4; ++sch) {
#define ROW_ONE(CROP, DEF, PIPE, EPI, OCC)                                                         \
        if (one_lane_build_exists(PIPE, sch)) {                                                    \
            if (n < cap) put(StepBuild{ONE_LANE, false, CROP, DEF, PIPE, sch, EPI, OCC}, out + 8 * n); \
            ++n;                                                                                   \
        }
        GL_STEP_ONE_LANE_BUILDS(ROW_ONE)
#undef ROW_ONE
#define ROW_QUAD(F64, DEF, PIPE, CROP, PAIR)                                                       \
        if (n < cap) put(StepBuild{PAIR ? QUAD_PAIR : QUAD, F64, CROP, DEF, PIPE, sch, 0, 1}, out + 8 * n); \
        ++n;
        GL_STEP_QUAD_BUILDS(ROW_QUAD)
#undef ROW_QUAD
    }
    return n;
}

// ---- glgym_evalF (tests/test_step_select_host.py, tests/test_evalf_build_inputs_host.py) ----
// in: n rows of 9 ints, EvalfSelectIn's fields in their order; out: n rows of 7 ints: error (0/1), the build's 5 fields, grid
void evalfselect_batch(int n, const int* in, int* out)
{
    for (int r = 0; r < n; ++r, in += 9, out += 7) {
        const EvalfSelectIn s{in[0] != 0, in[1], in[2] != 0, in[3] != 0, in[4], in[5], in[6], in[7] != 0, in[8] != 0};
        const EvalfChoice c = select_evalf(s);
        out[0] = c.error != nullptr;
        out[1] = c.build.family; out[2] = c.build.f64; out[3] = c.build.crop; out[4] = c.build.pipe; out[5] = c.build.sch;
        out[6] = (int)c.grid;
    }
}

const char* evalfselect_error_text()
{
    return select_evalf(EvalfSelectIn{false, RK4, true, true, 0, 1, 1, false, false}).error;
}

// the evalF build list as rows of 5 ints (at most cap rows are written); returns the number of builds
int evalfselect_builds(int* out, int cap)
{
    int n = 0;
    const auto row = [&](int family, bool f64, bool crop, bool pipe, int sch) {
        if (n < cap) { int* o = out + 5 * n; o[0] = family; o[1] = f64; o[2] = crop; o[3] = pipe; o[4] = sch; }
        ++n;
    };
    for (int sch = 0; sch < 4; ++sch) {
#define ROW_QUAD(F64, PIPE, CROP, PAIR) row(PAIR ? QUAD_PAIR : QUAD, F64, CROP, PIPE, sch);
        GL_EVALF_QUAD_BUILDS(ROW_QUAD)
#undef ROW_QUAD
#define ROW_ONE(CROP, PIPE) if (one_lane_build_exists(PIPE, sch)) row(ONE_LANE, false, CROP, PIPE, sch);
        GL_EVALF_ONE_LANE_BUILDS(ROW_ONE)
#undef ROW_ONE
    }
    return n;
}

}  // extern "C"
