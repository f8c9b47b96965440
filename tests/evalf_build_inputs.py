"""Cases, inputs and references of the evalF build census (tests/test_gpu_evalf_builds.py) and its host checks
(tests/test_evalf_build_inputs_host.py).  Importable without a GPU.

The cases: one per build csrc/gl_step_select.hpp lists for glgym_evalF -- 20 four-lanes-per-row builds of evalf_kernel_quad (fp64 plain,
crop and PAIR, fp32 plain and PAIR, per scheme) and 9 one-lane-per-row fp32 builds of evalf_kernel (plain and crop per scheme, the RK4
ODE_pipe build) -- each with the recipe that reaches it at B = 65 through the public setters.  Two more cases run a build that is already
listed on its other run-time branch: the fp64 RK4 sequential and PAIR builds with GLGYM_ODE_PIPE set.  The lists are restated here on
purpose: a build added to the header has no case until it is added here as well, and tests/test_evalf_build_inputs_host.py fails until
then.

Per-row parameter blocks reach a crop build only where the call has more than one row (glgym_evalF treats p_rows = B = 1 as one shared
block): expected_build() says what the recipe runs at B = 1 -- the plain sibling.

The inputs: step_build_inputs.base(), the step census's 65 rows (even rows far off equilibrium, odd rows calm), with the raw controls as
u.  Where the oracle shows that a (dtype, scheme) lacks what the census needs (tests/test_evalf_build_inputs_host.py), odd rows are
replaced here by rows of tests/golden/step_tight_jump.npz: REPLACED says which.  The step census's own inputs stay as they are.

The references: step_build_inputs.state_reference (oracle.gl_oracle.rk_sc_guarded row by row, cached by content; shared with the step
census, which integrates the same rows)."""
import collections

import numpy as np

import envlayer_inputs as E
import step_build_inputs as S

RK4, RK2, RK3, LS5 = S.RK4, S.RK2, S.RK3, S.LS5
ONE_LANE, QUAD, QUAD_PAIR = S.ONE_LANE, S.QUAD, S.QUAD_PAIR
SCHEMES = S.SCHEMES
N_ROWS, BATCHES, DT = S.N_ENV, S.BATCHES, S.DT
VERIFY_AUTO, VERIFY_NEVER = 0, 2                 # include/glgym.h glgym_verify_mode
LAYOUT_AUTO, LAYOUT_ONE = 0, 1
NAN_ROWS = (0, 64)                               # the row whose lane the round-5 miscompile dropped; the lone row of the last wavefront
EXCLUDED_ROWS = 0                                # rows a case may leave out of a comparison

# csrc/gl_step_select.hpp GL_EVALF_QUAD_BUILDS: (F64, PIPE, CROP, PAIR)
QUAD_BUILDS = [(1, 1, 0, 0), (1, 1, 1, 0), (1, 1, 0, 1), (0, 0, 0, 0), (0, 0, 0, 1)]
# GL_EVALF_ONE_LANE_BUILDS: (CROP, PIPE); PIPE with RK4 only
ONE_LANE_BUILDS = [(0, 0), (1, 0), (0, 1)]

# build = (family, f64, crop, pipe compiled in, sch): the row tests/stepselecthost exports; glgym_last_evalf_build returns
# (family, f64, crop, pipe compiled in, pipe taken, sch, grid, rows)
Case = collections.namedtuple("Case", "id build scheme f64 crop pipe nd layout lanes")
Mode = collections.namedtuple("Mode", "name verify ladder_parallel layout")


def _case(build, scheme, run_pipe=False):
    family, f64, crop, pipe, sch = build
    bits = [S.FAMILY_NAME[family], "f64" if f64 else "f32"] + (["crop"] if crop else []) + \
           (["pipe"] if pipe and not f64 else []) + [scheme] + (["runpipe"] if run_pipe and f64 else [])
    # one lane per row is reached by forcing the layout; per-row blocks reach it anyway, but a single row carries none (expected_build)
    layout = LAYOUT_ONE if family == ONE_LANE else LAYOUT_AUTO
    return Case(id="-".join(bits), build=build, scheme=scheme, f64=bool(f64), crop=bool(crop), pipe=bool(run_pipe), nd=14 if run_pipe else 10,
                layout=layout, lanes={ONE_LANE: 1, QUAD: 4, QUAD_PAIR: 8}[family])


def cases():
    out = []
    for scheme, (sch, _, _, _) in SCHEMES.items():
        for f64, pipe, crop, pair in QUAD_BUILDS:
            out.append(_case((QUAD_PAIR if pair else QUAD, f64, crop, pipe, sch), scheme))
        for crop, pipe in ONE_LANE_BUILDS:
            if not pipe or sch == RK4:
                out.append(_case((ONE_LANE, 0, crop, pipe, sch), scheme, run_pipe=bool(pipe)))
    # the run-time ODE_pipe branch of the fp64 builds (RK4 only: select_evalf refuses the other schemes)
    out.append(_case((QUAD, 1, 0, 1, RK4), "rk4", run_pipe=True))
    out.append(_case((QUAD_PAIR, 1, 0, 1, RK4), "rk4", run_pipe=True))
    return out


CASES = cases()
BUILD_CASES = [c for c in CASES if not (c.pipe and c.f64)]           # the 29: one per build
BY_ID = {c.id: c for c in CASES}


def modes(c):
    """PAIR builds run verified only; every other build unverified, and verified on the sequential ladder (the fp32 plain and pipe
    one-lane builds keep layout = one there, which the recipe sets anyway)."""
    if c.build[0] == QUAD_PAIR:
        return [Mode("verified", VERIFY_AUTO, 1, c.layout)]
    return [Mode("plain", VERIFY_NEVER, 1, c.layout), Mode("verified", VERIFY_AUTO, 0, c.layout)]


RUNS = [(c, m) for c in CASES for m in modes(c)]


def expected_build(c, B):
    """The build the recipe runs at B rows: per-row blocks need more than one row."""
    family, f64, crop, pipe, sch = c.build
    return (family, f64, int(bool(crop) and B > 1), pipe, sch)


def grid(c, B):
    return -(-c.lanes * B // 64)


def select_inputs(c, m, B, n_simd):
    """The row tests/stepselecthost's evalfselect_batch takes (EvalfSelectIn's fields in order) for what the recipe sets."""
    return [int(c.f64), SCHEMES[c.scheme][0], int(c.pipe), int(c.crop and B > 1), m.layout, B, n_simd, int(m.verify != VERIFY_NEVER),
            m.ladder_parallel]


def record(c, B):
    """What glgym_last_evalf_build returns after the recipe's call on B rows."""
    fam, f64, crop, pipe, sch = expected_build(c, B)
    return (fam, f64, crop, pipe, int(c.pipe), sch, grid(c, B), B)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
# (f64, scheme) -> {odd row of base(): row of tests/golden/step_tight_jump.npz that replaces it}.  Filled where the oracle shows that the
# 65 rows lack a row accepted beyond the second rung (tests/test_evalf_build_inputs_host.py test_rows_are_what_the_census_needs): with
# base() alone every row of every (dtype, scheme) is accepted at the second rung (n_sub against 2 n_sub), so a PAIR build would never
# run its second round.  Rows 1 and 3 of the jump fixture go to the third rung or beyond in all eight; they sit in different
# wavefronts at four and at eight lanes per row.
REPLACED = {(f64, scheme): {1: 1, 33: 3} for f64 in (False, True) for scheme in SCHEMES}
_inputs = {}


def rows(f64, scheme):
    """X [65, 28], U [65, 6], D [65, 10], CROP [65, 34] in float64 before rounding: base() with this (dtype, scheme)'s replacements."""
    b = S.base()
    X, U, D, CROP = b["X"].copy(), b["U"].copy(), b["D"].copy(), b["CROP"].copy()
    repl = REPLACED.get((bool(f64), scheme), {})
    if repl:
        g = np.load(S.GOLDEN / "step_tight_jump.npz", allow_pickle=False)
        for i, j in repl.items():
            assert i % 2 == 1
            X[i, :27], U[i], D[i] = g["X"][j][:27], g["U"][j], g["D"][j][:10]
    return X, U, D, CROP


def host_inputs(c):
    """What a case's call reads, as the handle's dtype stores it and widened again (float64 arrays), so that the kernels' double-to-T
    load is exact.  p: the handle's block; P: [65, 208] per-row blocks for the crop cases (p with each row's own p[128..161])."""
    key = (c.f64, c.scheme, c.crop, c.nd)
    if key not in _inputs:
        X, U, D, CROP = rows(c.f64, c.scheme)
        r = lambda a: E.rounded(a, c.f64)                                # noqa: E731
        d = D
        if c.nd != 10:
            d = S.weather_table(c.nd).copy()
            d[:, :10] = D
        p = S.params("handle")
        h = dict(x=r(X), u=r(U), d=r(d), p=p, crop=None, P=None)
        if c.crop:
            h["crop"] = r(CROP)
            h["P"] = np.tile(p, (N_ROWS, 1))
            h["P"][:, 128:162] = h["crop"]
        for v in h.values():
            if v is not None:
                v.setflags(write=False)
        _inputs[key] = h
    return _inputs[key]


def reference(c, m):
    """-> (x_next [65, 28], retries [65], refined sub-steps [65], failed [65]) of the oracle for case c in mode m."""
    h = host_inputs(c)
    return S.state_reference(h["x"], h["u"], h["d"], h["p"], h["crop"], c.scheme, c.pipe, verify=m.verify != VERIFY_NEVER)


def tiny_of(x):
    """2^-40 |x| per state: far below fp32 spacing (2^-24 |x|), far above fp64 spacing (2^-53 |x|)."""
    return np.ldexp(np.abs(x), -40)
