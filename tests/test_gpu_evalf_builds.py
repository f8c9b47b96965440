"""Every build of glgym_evalF's integrator kernels (csrc/gl_step_select.hpp: 20 four-lanes-per-row builds of evalf_kernel_quad, 9
one-lane-per-row builds of evalf_kernel) called through the C ABI on host arrays at ragged batches -- B = 65, which leaves one row in the
last wavefront at 1, 4 and 8 lanes per row, and B = 1 -- and compared with the oracle's restatement of the scheme, never with a kernel.
Cases, inputs and references: tests/evalf_build_inputs.py (checked on the CPU by tests/test_evalf_build_inputs_host.py).  Which build
ran is read back with glgym_last_evalf_build, so that a case cannot pass on another build's results.  The output array has a guard row
in front and behind, and every row of it holds a sentinel before the call.

Bounds.  State: tests/test_gpu_fuzz.py's metric and bounds (1e-11 fp64, 5e-6 fp32), which were set on these kernels; STATE_BOUND below
says where a (dtype, scheme, verify mode) departs from them and why.  A build whose error stands out from its siblings of the same
dtype, scheme and verify mode by more than 4x their median fails test_no_build_stands_out_from_its_siblings.  Everything between
siblings -- B = 1 against row 0 and row 64 of B = 65, PAIR against the sequential ladder, crop builds against plain builds on equal
blocks, the two routes to the same parameter block, the rows beside a failed row -- is compared bit for bit.

The sub-fp32 contract (include/glgym.h at glgym_evalF): the returned state is the caller's double x plus the increment computed in the
handle's dtype.  test_sub_fp32_bits_of_x_come_back holds every unverified fp32 build to it.

Not reached: rhs_kernel (glgym_rhs), and the PAIR limit at 8 192 rows, which tests/test_step_select_host.py reaches on the CPU.

With GLGYM_EVALF_CENSUS=<path> in the environment the measured figures of every case and mode are written there
(profiles/evalf_build_census.txt is such a file)."""
import ctypes as C
import os

import numpy as np
import pytest

import envlayer_inputs as E
import evalf_build_inputs as V
import step_build_inputs as S

pytestmark = pytest.mark.gpu

STAND_OUT = 4.0
# (f64, scheme, verified) -> bound on the state error; tests/test_gpu_fuzz.py's unless a line below says otherwise
STATE_BOUND = {(f64, s, v): (1e-11 if f64 else 5e-6) for f64 in (False, True) for s in V.SCHEMES for v in (False, True)}
# fp32 rk2, both modes: measured 5.98e-6 (quad, PAIR) and 6.08e-6 (one lane, with and without crop blocks) against the oracle, at row 33
# in all seven builds alike; every other row is at most 4.0e-6, the step census's figure.  Rows 1 and 33 are the two rows of the jump
# fixture that evalf_build_inputs.REPLACED puts in so that the PAIR builds run their second round: the oracle integrates them with
# 54 948 and 63 587 sub-steps in all (third rung, every attempt refined by the stability control), fifty times the 1 181 of the heaviest
# other row -- and of anything tests/test_gpu_fuzz.py's bound was set on.  Rounding in fp32 accumulates with the number of sub-steps: as
# a random walk over 50x the sub-steps it allows 7x; twice the fuzz bound is kept, so that the check still bites.  The other three
# schemes stay below 5e-6 on the same two rows (rk4 3.9e-6, rk3 3.2e-6, ls5 1.3e-6) and keep the bound.
STATE_BOUND[(False, "rk2", False)] = STATE_BOUND[(False, "rk2", True)] = 1e-5
SENTINEL =-1.2345678e300                  # no state of any row comes near it
_runs, _measured = {}, {}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return S.stepselect_host(tmp_path_factory.mktemp("stepselecthost"))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def call(f64, scheme, mode, x, u, d, p=None, p_rows=1, params=None, pipe=False, nd=10, integrator=0, first=None):
    """One handle, one glgym_evalF call on host arrays (after `first`, a call whose record the handle then holds) -> dict: rc, message,
    the B output rows, the record (None where glgym_last_evalf_build returns EINVAL), untouched (no output row was written)."""
    from gl_gym_amd import _lib as L
    hd = E.Handle(f64, V.DT, nd=nd, params=params)
    lib = hd.lib
    sch, n_sub, _, _ = V.SCHEMES[scheme]
    for rc in (lib.glgym_set_scheme(hd.h, sch), lib.glgym_set_n_sub(hd.h, n_sub), lib.glgym_set_verify(hd.h, mode.verify),
               lib.glgym_set_ladder_parallel(hd.h, mode.ladder_parallel), lib.glgym_set_layout(hd.h, mode.layout),
               lib.glgym_set_model_variant(hd.h, L.ODE_PIPE if pipe else L.ODE), lib.glgym_set_integrator(hd.h, integrator)):
        assert rc == L.OK, hd.error()
    rec = (C.c_int32 * 8)()
    assert lib.glgym_last_evalf_build(hd.h, rec) == L.EINVAL                     # no glgym_evalF yet
    dx = np.full(28, 0.5)
    assert lib.glgym_rhs(hd.h, _dp(np.ascontiguousarray(x[0])), _dp(np.ascontiguousarray(u[0])), _dp(np.ascontiguousarray(d[0])), 1, _dp(dx)) == L.OK
    assert lib.glgym_last_evalf_build(hd.h, rec) == L.EINVAL, "glgym_rhs must not touch the record"
    if first is not None:
        first(hd)
    ins = [np.ascontiguousarray(a, dtype=np.float64).copy() for a in (x, u, d)] + ([] if p is None else [np.ascontiguousarray(p, dtype=np.float64).copy()])
    kept = [a.copy() for a in ins]
    B = len(ins[0])
    out = np.full((B + 2, 28), SENTINEL)
    rc = lib.glgym_evalF(hd.h, _dp(ins[0]), _dp(ins[1]), _dp(ins[2]), None if p is None else _dp(ins[3]), p_rows, B, _dp(out[1:]))
    msg = hd.error()
    try:
        hd.sync()
    except RuntimeError as e:                        # a device fault: nothing more is launched in this session
        pytest.exit(f"device error after glgym_evalF ({scheme}, f64={f64}, {mode}): {e}", returncode=3)
    if rc == L.EHIP:
        pytest.exit(f"GLGYM_EHIP from glgym_evalF ({scheme}, f64={f64}, {mode}, B={B}): {msg}", returncode=3)
    for a, k in zip(ins, kept):
        assert np.array_equal(E.bits(a), E.bits(k)), "glgym_evalF wrote to an input array"
    assert np.all(out[0] == SENTINEL) and np.all(out[-1] == SENTINEL), "a guard row of the output was written"
    has = lib.glgym_last_evalf_build(hd.h, rec) == L.OK
    r = dict(rc=rc, msg=msg, out=out[1:-1].copy(), record=tuple(rec) if has else None, untouched=bool(np.all(out == SENTINEL)), B=B,
             n_simd=4 * hd.t.cuda.get_device_properties(0).multi_processor_count, hd=hd)
    return r


def run(c, m, rows=None, nan_row=None, route="handle", tiny=False, equal=False):
    """Case c's recipe in mode m on the given rows of its 65 (default: all).  nan_row: x[nan_row, 2] = NaN.  route "handle": the handle is
    created with the block and the call passes p = NULL (per-row blocks for the crop cases); "call": a default handle and the block
    (or the per-row blocks) in the call.  tiny: x + 2^-40 |x|.  equal: a crop case with every row's block equal to the handle's.
    Cached: a sibling is launched once."""
    rows = tuple(range(V.N_ROWS)) if rows is None else tuple(rows)
    key = (c.id, m.name, rows, nan_row, route, tiny, equal)
    if key in _runs:
        return _runs[key]
    h = V.host_inputs(c)
    idx = list(rows)
    x = h["x"][idx].copy()
    if tiny:
        x = x + V.tiny_of(x)
    if nan_row is not None:
        x[nan_row, 2] = np.nan
    p, p_rows = None, 1
    if c.crop:
        P = np.tile(h["p"], (V.N_ROWS, 1)) if equal else h["P"]
        p, p_rows = (P[idx], len(idx)) if len(idx) > 1 else (P[idx[0]], 1)
    elif route == "call":
        p = h["p"]
    r = call(c.f64, c.scheme, m, x, h["u"][idx], h["d"][idx], p, p_rows, params=None if route == "call" else h["p"], pipe=c.pipe, nd=c.nd)
    r["hd"].close()
    del r["hd"]
    r["x"] = x
    _runs[key] = r
    return r


def ok(r):
    from gl_gym_amd import _lib as L
    assert r["rc"] == L.OK, (r["rc"], r["msg"])
    assert np.all(np.isfinite(r["out"])), "a row of a successful call was not written"
    return r


def same_bits(a, b, what):
    assert np.array_equal(E.bits(a), E.bits(b)), (what, float(np.nanmax(np.abs(a - b))))


def measure(c, m):
    """Worst state error of case c in mode m at B = 65 against the oracle -> dict (cached)."""
    if (c.id, m.name) not in _measured:
        r = ok(run(c, m))
        ref, retries, refined, failed = V.reference(c, m)
        assert not failed.any()
        err = S.state_error(r["out"], ref, V.host_inputs(c)["x"])               # all 28 states, the time state included
        _measured[(c.id, m.name)] = dict(state=float(err.max()), row=int(err.argmax()), refined=int((refined > 0).sum()),
                                         beyond2=int((retries >= 2).sum()))
    return _measured[(c.id, m.name)]


def siblings(c, m):
    """The cases of c's dtype and scheme that have a run in this verify mode.  An ODE_pipe run is alone with its right-hand side (and, in
    fp64 verified, with its bit-identical PAIR twin): it is held to the level of the same dtype's rk4 builds of the default ODE -- the
    same kernels but for the pipe equation -- on its own inputs, and does not count among their siblings."""
    return [d for d in V.CASES if d.f64 == c.f64 and d.scheme == c.scheme and not d.pipe and d.id != c.id and
            any(mm.name == m.name for mm in V.modes(d))]


def mode_of(d, name):
    return next(mm for mm in V.modes(d) if mm.name == name)


@pytest.mark.parametrize("c,m", V.RUNS, ids=[f"{c.id}-{m.name}" for c, m in V.RUNS])
def test_build(c, m, host):
    from gl_gym_amd import _lib as L
    full = ok(run(c, m))
    # which build ran
    assert full["record"] == V.record(c, V.N_ROWS), (c.id, m.name, full["record"])
    sel = np.full((1, 7), -7, dtype=np.int32)
    row = np.array([V.select_inputs(c, m, V.N_ROWS, full["n_simd"])], dtype=np.int32)
    host.evalfselect_batch(1, row.ctypes.data, sel.ctypes.data)
    assert sel[0].tolist() == [0, *full["record"][:4], full["record"][5], full["record"][6]]
    # state against the oracle
    q = measure(c, m)
    bound = STATE_BOUND[(c.f64, c.scheme, m.name == "verified")]
    print(f"evalF build {c.id} {m.name}: worst scaled |state - oracle| = {q['state']:.2e} (row {q['row']}, bound {bound:.1e}), "
          f"{q['refined']} of 65 rows refined, {q['beyond2']} beyond the second rung")
    assert q["state"] < bound, (c.id, m.name, q["state"], q["row"])
    # a row does not depend on the rows around it
    for r0 in (0, 64):
        one = ok(run(c, m, rows=(r0,)))
        assert one["record"] == V.record(c, 1), (c.id, m.name, one["record"])
        same_bits(one["out"][0], full["out"][r0], f"row {r0} alone against row {r0} of 65")
    # the block in the handle and the block in the call
    same_bits(ok(run(c, m, route="call"))["out"], full["out"], "p = NULL on a handle created with the block against the block in the call")
    # a failed row: NaN, GLGYM_EODE, counted, and no other row notices
    for r0 in V.NAN_ROWS:
        bad = run(c, m, nan_row=r0)
        assert bad["rc"] == L.EODE and "failed for 1 of 65 rows" in bad["msg"], (bad["rc"], bad["msg"])
        assert np.all(np.isnan(bad["out"][r0])), "the failed row is NaN in every state"
        others = np.arange(V.N_ROWS) != r0
        same_bits(bad["out"][others], full["out"][others], f"rows beside failed row {r0}")
        assert bad["record"] == full["record"]


PAIRS = [c for c in V.CASES if c.build[0] == V.QUAD_PAIR]


@pytest.mark.parametrize("c", PAIRS, ids=[c.id for c in PAIRS])
def test_pair_equals_the_sequential_ladder(c):
    seq = next(d for d in V.CASES if d.build == (V.QUAD,) + c.build[1:] and d.pipe == c.pipe and d.scheme == c.scheme)
    a, b = ok(run(c, mode_of(c, "verified"))), ok(run(seq, mode_of(seq, "verified")))
    assert a["record"][0] == V.QUAD_PAIR and b["record"][0] == V.QUAD and a["record"][4] == b["record"][4] == int(c.pipe)
    same_bits(a["out"], b["out"], "PAIR against the sequential ladder")


CROPS = [(c, m) for c, m in V.RUNS if c.crop]


@pytest.mark.parametrize("c,m", CROPS, ids=[f"{c.id}-{m.name}" for c, m in CROPS])
def test_crop_build_equals_plain_build_on_equal_blocks(c, m):
    """Every row's crop block equal to the handle's: the crop build computes each row's crop constants itself, the plain build takes
    them from the handle's block."""
    plain = next(d for d in V.CASES if d.build == c.build[:2] + (0,) + c.build[3:] and not d.pipe and d.scheme == c.scheme)
    a, b = ok(run(c, m, equal=True)), ok(run(plain, mode_of(plain, m.name)))
    assert a["record"][:3] == c.build[:3] and b["record"][:3] == plain.build[:3]
    same_bits(a["out"], b["out"], "crop build on equal blocks against the plain build")


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
def test_ode_pipe_refusals(f64):
    """GLGYM_ODE_PIPE with per-row blocks, and with a scheme other than RK4: GLGYM_EINVAL, nothing written, the record as it was."""
    from gl_gym_amd import _lib as L
    c = V.BY_ID["quad-f64-rk4-runpipe" if f64 else "one-f32-pipe-rk4"]
    m = V.modes(c)[0]
    h = V.host_inputs(c)
    before = {}

    def valid_call_then(scheme):                     # a valid single-row call, so that there is a record to keep; then the scheme
        def first(hd):
            x1 = np.empty((1, 28))
            assert hd.lib.glgym_evalF(hd.h, _dp(h["x"][:1].copy()), _dp(h["u"][:1].copy()), _dp(h["d"][:1].copy()), None, 1, 1, _dp(x1)) == L.OK
            rec = (C.c_int32 * 8)()
            assert hd.lib.glgym_last_evalf_build(hd.h, rec) == L.OK
            before["record"] = tuple(rec)
            assert hd.lib.glgym_set_scheme(hd.h, V.SCHEMES[scheme][0]) == L.OK
        return first

    blocks = dict(p=np.tile(h["p"], (5, 1)), p_rows=5)
    for scheme, kw in (("rk4", blocks), ("rk3", {})):
        before.clear()
        r = call(f64, "rk4", m, h["x"][:5], h["u"][:5], h["d"][:5], params=h["p"], pipe=True, nd=14, first=valid_call_then(scheme), **kw)
        r["hd"].close()
        assert r["rc"] == L.EINVAL and "GLGYM_ODE_PIPE supports neither" in r["msg"] and r["untouched"], (scheme, r["rc"], r["msg"])
        assert r["record"] == before["record"] == V.record(c, 1), (scheme, r["record"])


@pytest.mark.parametrize("f64,bdf", [(False, 0), (True, 0), (True, 1)], ids=["f32", "f64", "f64-bdf"])
def test_row_at_a_time_fallback(f64, bdf):
    """Five rows whose row 3 differs from row 0 outside p[128..161]: five single-row calls, bit for bit; the record is the last one's."""
    from gl_gym_amd import _lib as L
    c = V.BY_ID["pair-f64-rk4" if f64 else "pair-f32-rk4"]
    m = mode_of(c, "verified")                       # ladder_parallel on: a single verified row takes the PAIR build
    h = V.host_inputs(c)
    P = np.tile(h["p"], (5, 1))
    P[3, 50] *= 1.01
    stats = {}

    def keep_stats(hd, n):
        s = np.zeros((n, L.NSOLVER_STAT), dtype=np.int32)
        assert hd.lib.glgym_get_solver_stats(hd.h, n, s.ctypes.data_as(C.POINTER(C.c_int32))) == L.OK, hd.error()
        return s

    r = call(f64, "rk4", m, h["x"][:5], h["u"][:5], h["d"][:5], P, 5, integrator=bdf)
    if bdf:
        stats["batch"] = keep_stats(r["hd"], 5)
    r["hd"].close()
    ok(r)
    singles = []
    for i in range(5):
        s = call(f64, "rk4", m, h["x"][i:i + 1], h["u"][i:i + 1], h["d"][i:i + 1], P[i], 1, integrator=bdf)
        if bdf:
            singles.append(keep_stats(s["hd"], 1)[0])
        s["hd"].close()
        same_bits(ok(s)["out"][0], r["out"][i], f"row {i} of the batch against its own call")
        last = s["record"]
    assert r["record"] == last and last[7] == 1
    assert last[0] == (-1 if bdf else V.QUAD_PAIR)
    if bdf:
        assert np.array_equal(stats["batch"], np.array(singles)) and np.all(stats["batch"][:, 0] > 0)


def test_bdf_call_records_no_build():
    from gl_gym_amd import _lib as L
    c = V.BY_ID["quad-f64-ls5"]
    h = V.host_inputs(c)
    r = call(True, "ls5", V.modes(c)[0], h["x"][:3], h["u"][:3], h["d"][:3], integrator=L.INTEGRATORS["bdf"])
    r["hd"].close()
    ok(r)
    assert r["record"] == (-1, 0, 0, 0, 0, 0, 0, 3)


UNVERIFIED_F32 = [c for c in V.CASES if not c.f64 and c.build[0] != V.QUAD_PAIR]


@pytest.mark.parametrize("c", UNVERIFIED_F32, ids=[c.id for c in UNVERIFIED_F32])
def test_sub_fp32_bits_of_x_come_back(c):
    """x is fp32-representable, x + tiny rounds to the same fp32 state: the integration is the same, bit for bit, and the two results
    differ by tiny -- to the two roundings of the final double addition, one spacing of the result each."""
    m = mode_of(c, "plain")
    a, b = ok(run(c, m)), ok(run(c, m, tiny=True))
    assert np.array_equal(b["x"].astype(np.float32), a["x"].astype(np.float32))
    shift = b["x"] - a["x"]                                       # tiny as the double x + tiny holds it (the subtraction is exact)
    assert np.all((shift != 0) == (a["x"] != 0))
    slack = 2 * np.spacing(np.maximum(np.abs(a["out"]), np.abs(b["out"])))
    miss = np.abs((b["out"] - a["out"]) - shift) > slack
    assert not miss.any(), (c.id, int(miss.sum()), "states lost the bits of x below fp32 spacing; first (row, state):", np.argwhere(miss)[0].tolist())


def test_no_build_stands_out_from_its_siblings():
    """The census: every case's figure in every mode (measured here for whatever the session has not run yet), each build's state error
    against the median of its siblings of the same dtype, scheme and verify mode."""
    lines, bad = [], []
    for c, m in V.RUNS:
        q = measure(c, m)
        sib = [measure(d, mode_of(d, m.name))["state"] for d in siblings(c, m)]
        med = float(np.median(sib)) if sib else float("nan")
        bound = STATE_BOUND[(c.f64, c.scheme, m.name == "verified")]
        origin = "tests/test_gpu_fuzz.py" if bound == (1e-11 if c.f64 else 5e-6) else "STATE_BOUND in tests/test_gpu_evalf_builds.py"
        lines.append(f"{c.id:24s} {m.name:8s} state {q['state']:.2e} (row {q['row']:2d}; siblings' median {med:.2e}; bound {bound:.1e}, "
                     f"{origin})  refined rows {q['refined']:2d}  rows beyond the second rung {q['beyond2']}")
        if sib and q["state"] > STAND_OUT * med:
            bad.append(lines[-1])
    print("\n".join(lines))
    path = os.environ.get("GLGYM_EVALF_CENSUS")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert not bad, "\n".join(bad)
