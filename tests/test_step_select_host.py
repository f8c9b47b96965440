"""CPU test of the env-step kernel selection: csrc/gl_step_select.hpp (host instantiation, tests/stepselecthost/stepselecthost.cpp)
against a Python restatement of the rules written from the header's comments and DESIGN.md section 5, over the full product of the
inputs that can change the choice; and the no-dead-kernel checks both ways: every selected build is in the build list, every listed
build is selected by some input.  Everything is integers and comparisons: EXACT."""
import ctypes as C
import itertools
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
RK4, RK2, RK3, LS5 = 0, 1, 2, 3
ONE_LANE, QUAD, QUAD_PAIR = 0, 1, 2
OBS, RESET = 8, 16
N_SIMD = 1024
FIELDS = ("f64", "scheme", "pipe", "crop", "default", "layout", "occupancy", "B", "n_simd", "verify", "ladder_parallel", "obs_ok",
          "obs_dim", "reset_ok")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = tmp_path_factory.mktemp("stepselecthost") / "libstepselecthost.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", f"-I{CSRC}", "-o", str(so),
                           str(ROOT / "tests" / "stepselecthost" / "stepselecthost.cpp")])
    lib = C.CDLL(str(so))
    lib.stepselect_batch.argtypes, lib.stepselect_batch.restype = [C.c_int, C.c_void_p, C.c_void_p], None
    lib.stepselect_builds.argtypes, lib.stepselect_builds.restype = [C.c_void_p, C.c_int], C.c_int
    lib.stepselect_pipe_error_batch.argtypes, lib.stepselect_pipe_error_batch.restype = [C.c_int, C.c_void_p, C.c_void_p], None
    lib.stepselect_error_text.restype = C.c_char_p
    lib.evalfselect_batch.argtypes, lib.evalfselect_batch.restype = [C.c_int, C.c_void_p, C.c_void_p], None
    lib.evalfselect_builds.argtypes, lib.evalfselect_builds.restype = [C.c_void_p, C.c_int], C.c_int
    lib.evalfselect_error_text.restype = C.c_char_p
    return lib


def inputs():
    """The full product: [n, 15] int32 (column 14 is padding)."""
    rows = itertools.product((0, 1), (RK4, RK2, RK3, LS5), (0, 1), (0, 1), (0, 1), (0, 1, 2), (0, 1, 2),
                             (1, 8192, 8193, 16384, 16385, 131071, 131072), (N_SIMD,), (0, 1), (0, 1), (0, 1),
                             (0, 1, 292, 293, 512, 513), (0, 1), (0,))
    return np.array(list(rows), dtype=np.int32)


def restated(f64, scheme, pipe, crop, default, layout, occupancy, B, n_simd, verify, ladder_parallel, obs_ok, obs_dim, reset_ok):
    """(error, family, f64, crop, default, pipe, scheme, epilogue, occ, grid, fused) by the documented rules."""
    if pipe and (crop or scheme != RK4):
        return (1,) + (0,) * 10
    lanes = 8 if (verify and ladder_parallel and not crop and 8 * B <= 64 * n_simd) else 4     # per environment, on a quad build
    family = QUAD_PAIR if lanes == 8 else QUAD
    if f64:             # always quad: ODE_pipe compiled in, never the default block, per-env crop blocks taken
        return (0, family, 1, crop, 0, 1, scheme, 0, 1, -(-lanes * B // 64), 0)
    small = B <= 16 * n_simd
    if not pipe and not crop and (layout == 2 or (layout == 0 and small)):
        return (0, family, 0, 0, default, 0, scheme, 0, 1, -(-lanes * B // 64), 0)
    grid = -(-B // 64)
    if pipe:            # the single generic RK4 build, no epilogue
        return (0, ONE_LANE, 0, 0, 0, 1, RK4, 0, 1, grid, 0)
    two_waves = bool(default and not crop and (occupancy == 2 or (occupancy == 0 and B >= 2 * 64 * n_simd)))
    with_obs = bool(obs_ok and 1 <= obs_dim <= (292 if two_waves else 512))
    with_reset = with_obs and bool(reset_ok) and not crop
    epilogue = (OBS if with_obs else 0) | (RESET if with_reset else 0)
    return (0, ONE_LANE, 0, crop, default, 0, scheme, epilogue, 2 if two_waves else 1, grid, int(with_obs) + int(with_reset))


def builds(host):
    n = host.stepselect_builds(None, 0)
    out = np.zeros((n, 8), dtype=np.int32)
    assert host.stepselect_builds(out.ctypes.data, n) == n
    return out


@pytest.fixture(scope="module")
def selected(host):
    rows = inputs()
    out = np.full((len(rows), 11), -7, dtype=np.int32)
    host.stepselect_batch(len(rows), rows.ctypes.data, out.ctypes.data)
    return rows, out


def test_selection_matches_the_documented_rules(selected):
    rows, out = selected
    assert len(rows) == 2 * 4 * 2 * 2 * 2 * 3 * 3 * 7 * 4 * 2 * 6 * 2
    want = np.array([restated(*r[:14]) for r in rows.tolist()], dtype=np.int32)
    err = want[:, 0] == 1
    assert np.array_equal(out[:, 0], want[:, 0])
    bad = np.nonzero((out[~err] != want[~err]).any(axis=1))[0]
    assert len(bad) == 0, (dict(zip(FIELDS, rows[~err][bad[0]].tolist())), out[~err][bad[0]].tolist(), want[~err][bad[0]].tolist())


def test_error_text(host):
    assert host.stepselect_error_text() == (b"glgym_step: GLGYM_ODE_PIPE supports neither per-env crop parameters nor schemes other than "
                                            b"GLGYM_SCHEME_RK4")


def test_pipe_rule_on_its_own_is_what_select_step_reports(host):
    """glsel::step_pipe_error(pipe, crop, scheme) -- what glgym_step's host-side check asks before anything is launched -- against
    select_step over the full product: one is non-null exactly when the other is, and then the two texts are equal."""
    rows = inputs()
    out = np.full((len(rows), 3), -7, dtype=np.int32)
    host.stepselect_pipe_error_batch(len(rows), rows.ctypes.data, out.ctypes.data)
    assert np.array_equal(out[:, 0], out[:, 1])
    assert (out[:, 2] == 1).all()
    want = (rows[:, 2] == 1) & ((rows[:, 3] == 1) | (rows[:, 1] != RK4))
    assert np.array_equal(out[:, 1] == 1, want) and 0 < want.sum() < len(rows)


def test_build_list_is_the_81_kernels(host):
    b = builds(host)
    assert len(b) == 81 and len({tuple(r) for r in b.tolist()}) == 81
    one, quad = b[b[:, 0] == ONE_LANE], b[b[:, 0] != ONE_LANE]
    assert len(one) == 4 * 13 + 1 and len(quad) == 4 * 7
    assert not one[:, 1].any() and (quad[:, 1] == 1).sum() == 4 * 3                  # one lane per environment: fp32 only


def test_every_selected_build_is_listed_and_every_listed_build_is_selected(host, selected):
    _, out = selected
    chosen = {tuple(r) for r in out[out[:, 0] == 0][:, 1:9].tolist()}
    listed = {tuple(r) for r in builds(host).tolist()}
    assert chosen - listed == set(), sorted(chosen - listed)[:5]
    assert listed - chosen == set(), sorted(listed - chosen)[:5]


# ---- glgym_evalF: select_evalf and the list of the 29 evalF builds --------------------------------------------------------------------
EVALF_FIELDS = ("f64", "scheme", "pipe", "crop", "layout", "B", "n_simd", "verify", "ladder_parallel")


def evalf_inputs():
    """The full product: [n, 9] int32."""
    rows = itertools.product((0, 1), (RK4, RK2, RK3, LS5), (0, 1), (0, 1), (0, 1, 2), (1, 8, 65, 8192, 8193, 16384, 16385), (256, 1024),
                             (0, 1), (0, 1))
    return np.array(list(rows), dtype=np.int32)


def evalf_restated(f64, scheme, pipe, crop, layout, B, n_simd, verify, ladder_parallel):
    """(error, family, f64, crop, pipe compiled in, scheme, grid) by the documented rules (include/glgym.h at glgym_set_ladder_parallel
    and glgym_step's layouts)."""
    if pipe and (crop or scheme != RK4):
        return (1, 0, 0, 0, 0, 0, 0)
    free_lanes = 8 * B <= 64 * n_simd                      # at most one wavefront per SIMD at eight lanes per row
    two_rungs = bool(verify and ladder_parallel and not crop and free_lanes)
    if f64:                                                # four lanes per row always, ODE_pipe compiled in, per-row crop blocks taken
        lanes = 8 if two_rungs else 4
        return (0, QUAD_PAIR if two_rungs else QUAD, 1, crop, 1, scheme, -(-lanes * B // 64))
    if pipe:                                               # the only fp32 kernel with the pipe equation
        return (0, ONE_LANE, 0, 0, 1, RK4, -(-B // 64))
    if two_rungs and layout != 1:                          # a forced one-lane layout keeps the sequential ladder
        return (0, QUAD_PAIR, 0, 0, 0, scheme, -(-8 * B // 64))
    if not crop and (layout == 2 or (layout == 0 and B <= 16 * n_simd)):
        return (0, QUAD, 0, 0, 0, scheme, -(-4 * B // 64))
    return (0, ONE_LANE, 0, crop, 0, scheme, -(-B // 64))


def evalf_builds(host):
    n = host.evalfselect_builds(None, 0)
    out = np.zeros((n, 5), dtype=np.int32)
    assert host.evalfselect_builds(out.ctypes.data, n) == n
    return out


@pytest.fixture(scope="module")
def evalf_selected(host):
    rows = evalf_inputs()
    out = np.full((len(rows), 7), -7, dtype=np.int32)
    host.evalfselect_batch(len(rows), rows.ctypes.data, out.ctypes.data)
    return rows, out


def test_evalf_selection_matches_the_documented_rules(evalf_selected):
    rows, out = evalf_selected
    assert len(rows) == 2 * 4 * 2 * 2 * 3 * 7 * 2 * 2 * 2
    want = np.array([evalf_restated(*r) for r in rows.tolist()], dtype=np.int32)
    err = want[:, 0] == 1
    assert np.array_equal(out[:, 0], want[:, 0])
    bad = np.nonzero((out[~err] != want[~err]).any(axis=1))[0]
    assert len(bad) == 0, (dict(zip(EVALF_FIELDS, rows[~err][bad[0]].tolist())), out[~err][bad[0]].tolist(), want[~err][bad[0]].tolist())


def test_evalf_error_text(host):
    assert host.evalfselect_error_text() == (b"glgym_evalF: GLGYM_ODE_PIPE supports neither per-row parameter blocks nor schemes other "
                                             b"than GLGYM_SCHEME_RK4")


def test_evalf_build_list_is_the_29_kernels(host):
    b = evalf_builds(host)
    assert len(b) == 29 and len({tuple(r) for r in b.tolist()}) == 29
    one, quad = b[b[:, 0] == ONE_LANE], b[b[:, 0] != ONE_LANE]
    assert len(one) == 4 * 2 + 1 and len(quad) == 4 * 5
    assert not one[:, 1].any() and (quad[:, 1] == 1).sum() == 4 * 3                  # one lane per row: fp32 only
    assert (b[:, 0] == QUAD_PAIR).sum() == 4 * 2 and not b[b[:, 0] == QUAD_PAIR][:, 2].any()     # PAIR: both dtypes, never with crop blocks
    assert b[b[:, 1] == 1][:, 3].all()                                               # ODE_pipe: compiled into every fp64 build ...
    assert b[(b[:, 1] == 0) & (b[:, 3] == 1)].tolist() == [[ONE_LANE, 0, 0, 1, RK4]]  # ... and into one fp32 build


def test_every_selected_evalf_build_is_listed_and_every_listed_build_is_selected(host, evalf_selected):
    _, out = evalf_selected
    chosen = {tuple(r) for r in out[out[:, 0] == 0][:, 1:6].tolist()}
    listed = {tuple(r) for r in evalf_builds(host).tolist()}
    assert chosen - listed == set(), sorted(chosen - listed)[:5]
    assert listed - chosen == set(), sorted(listed - chosen)[:5]
