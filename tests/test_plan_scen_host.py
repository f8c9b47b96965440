"""CPU tests of robust planning's scalar logic: csrc/gl_scen.hpp (host instantiation, tests/scenhost/scenhost.cpp -- a lane is a call,
the aggregating wavefront a loop over 64 lanes) against NumPy / Python restatements written from include/glgym.h.

Bounds.
* Scenario crop blocks: EXACT (uint32 view).  Every operation of the definition is a correctly rounded double or float32 operation, and
  NumPy performs the same ones in the same order.
* Aggregate: EXACT (uint64 view) against a Python loop over the sorted returns -- not np.sum, whose pairwise order differs.
* Moments of z / scale = u - 0.5 over N = 4 096 (p, s, h) triples, per crop parameter: mean within 5 standard errors sqrt(1 / (12 N)) of
  0, variance within 5 standard errors sqrt(1 / (180 N)) of 1/12 (a uniform's fourth central moment is 1/80: (1/80 - 1/144) / N); the
  generator is deterministic and MOMENT_SEED was picked once so that the NumPy restatement itself passes."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_controller_and_noise import philox4x32_10
from test_plan_cem_host import np_philox

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SRC = ROOT / "tests" / "scenhost" / "scenhost.cpp"
KEY_TAG = 0x5343454E
M32 = 0xFFFFFFFF
NCROP = 34
MOMENT_SEED = 2026
SEED, DRAW = 0xDEADBEEF12345678, (7 << 32) | 41                # both with a nonzero high word


def build_host(path):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.scenhost_sizeof.argtypes, lib.scenhost_sizeof.restype = [C.c_int], C.c_int
    lib.scenhost_scenario.argtypes = [C.c_int] * 6 + [C.c_double, C.c_uint64, C.c_uint64] + [C.c_void_p] * 4
    lib.scenhost_scenario.restype = None
    lib.scenhost_centred.argtypes, lib.scenhost_centred.restype = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p], None
    lib.scenhost_aggregate.argtypes, lib.scenhost_aggregate.restype = [C.c_int] * 5 + [C.c_void_p] * 8, None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_scen.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    return build_host(tmp_path_factory.mktemp("scenhost") / "libscenhost.so")


def ptr(a):
    return None if a is None else a.ctypes.data


def nominal_crop():
    """float32 p[128..161] of the default parameters: what a handle keeps on the device."""
    from gl_gym_amd.parameters import init_default_params
    return np.asarray(init_default_params(), dtype=np.float64)[128:162].astype(np.float32)


# ---- restatements (from the header's text, not from gl_scen.hpp) --------------------------------------------------------------
def np_scen_words(P, S, h, hold, seed, D):
    """The 34 used words of every (greenhouse, scenario) at step h: [P*S, 34] uint64."""
    hh = 0 if hold else h
    ps = np.arange(P * S, dtype=np.uint64)                                 # p*S + s
    return np.concatenate([np_philox(ps, D & M32, D >> 32, 16 * hh + blk, seed & M32, (seed >> 32) ^ KEY_TAG) for blk in range(9)],
                          axis=-1)[:, :NCROP]


def np_scen_crop(P, K, S, h, hold, scale, seed, D, p0):
    """The crop blocks of the P*K*S children at step h: [34, C] float32, child c = (p*K + k)*S + s."""
    u = (np_scen_words(P, S, h, hold, seed, D).astype(np.float64) + 0.5) * 2.0 ** -32
    z = (u - 0.5) * np.float64(scale)
    p64 = p0.astype(np.float64)[None, :]
    t = z * p64
    v = (p64 + t).astype(np.float32)
    v[:, 16] = v[:, 13] / v[:, 14]                                         # float32 / float32
    v = np.broadcast_to(v.reshape(P, 1, S, NCROP), (P, K, S, NCROP)).reshape(P * K * S, NCROP)
    return np.ascontiguousarray(v.T)


def py_aggregate(J, S, m, ret, failed, viol=None, n_steps=None):
    """The header's definition as a Python loop (Python floats are doubles; every + and / is one rounded operation)."""
    rc, fc = np.empty(J), np.zeros(J, np.uint8)
    vc = None if viol is None else np.empty((3, J))
    sc = None if n_steps is None else np.empty(J, np.int32)
    for j in range(J):
        rs = [float(v) for v in ret[j * S:(j + 1) * S]]
        if failed[j * S:(j + 1) * S].any() or not all(np.isfinite(rs)):
            rc[j], fc[j] = np.nan, 1
        else:
            a, acc = sorted(rs), 0.0
            for i in range(m):
                acc = acc + a[i]
            rc[j] = acc / float(m)
        if vc is not None:
            for i in range(3):
                acc = 0.0
                for s in range(S):
                    acc = acc + float(viol[i, j * S + s])
                vc[i, j] = acc / float(S)
        if sc is not None:
            sc[j] = min(int(v) for v in n_steps[j * S:(j + 1) * S])
    return rc, fc, vc, sc


def aggregate_case(rng, J, S):
    """Scenario returns of J >= 6 candidates: row 0 holds a NaN, row 1 a +inf, row 2 a failed scenario, row 3 exact ties, row 4 both
    zeros among other values, the rest half-integers with ties by chance; violations; step counts.  ld = J*S + 3."""
    n = J * S
    ret = np.round(rng.normal(size=n) * 3.0) / 2.0                         # half-integers: many exact ties
    mask = rng.random(n) < 0.4
    ret[mask] += rng.normal()                                              # ... among other values
    failed = np.zeros(n, np.uint8)
    ret[0 * S + S // 2] = np.nan
    ret[1 * S + S - 1] = np.inf
    failed[2 * S] = 1
    if S >= 2:
        ret[3 * S + S - 1] = ret[3 * S]
        ret[4 * S], ret[4 * S + S - 1] = 0.0, -0.0
    ld = n + 3
    viol = np.zeros((3, ld))
    viol[:, :n] = np.abs(rng.normal(size=(3, n))) * (rng.random((3, n)) < 0.5)
    n_steps = rng.integers(1, 49, size=n).astype(np.int32)
    return ret, failed, viol, n_steps, ld


def run_scenario(host, P, K, S, h, hold, scale, seed, D, p0, actions=None, ld=None):
    n = P * K * S
    ld = n if ld is None else ld
    crop = np.full((NCROP, ld), 7, np.float32)
    out = None if actions is None else np.full((n, 6), 7, np.float32)
    host.scenhost_scenario(P, K, S, ld, h, hold, scale, seed, D, ptr(p0), ptr(crop), ptr(actions), ptr(out))
    return crop, out


def run_aggregate(host, J, S, m, ld, ret, failed, viol, n_steps):
    rc, fc, vc, sc = np.full(J, 7.0), np.full(J, 7, np.uint8), np.full((3, J + 2), 7.0), np.full(J, 7, np.int32)
    host.scenhost_aggregate(J, S, m, ld, J + 2, ptr(ret), ptr(failed), ptr(viol), ptr(n_steps), ptr(rc), ptr(fc), ptr(vc), ptr(sc))
    return rc, fc, vc, sc


def same_f64(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


AGG_SHAPES = [(S, m) for S in (1, 5, 64, 65, 256) for m in sorted({1, min(2, S), S})]


# ---- tests -------------------------------------------------------------------------------------------------------------------
def test_args_structs_have_the_headers_sizes(host):
    from gl_gym_amd import _lib as L
    for which, cls in enumerate((L.PlanScenarioArgs, L.PlanRolloutScenariosArgs, L.PlanAggregateArgs)):
        assert C.sizeof(cls) == host.scenhost_sizeof(which), cls.__name__
        assert cls._fields_[0][0] == "struct_size"
    hdr = (ROOT / "include" / "glgym.h").read_text()
    for name in ("glgym_plan_scenario", "glgym_plan_rollout_scenarios", "glgym_plan_aggregate"):
        assert name in L.PROTOTYPES and re.search(rf"\bint {name}\s*\(", hdr), name
    assert L.ABI_VERSION == 7 == int(re.search(r"#define GLGYM_ABI_VERSION (\d+)", hdr).group(1))
    assert L.MAX_SCENARIOS == 256


def test_vectorised_words_are_the_scalar_definition():
    w = np_scen_words(2, 5, 2, 0, SEED, DRAW)
    for ps in (0, 7, 9):
        exp = []
        for blk in range(9):
            exp += philox4x32_10([ps, DRAW & M32, DRAW >> 32, 16 * 2 + blk], [SEED & M32, (SEED >> 32) ^ KEY_TAG])
        assert w[ps].tolist() == exp[:NCROP]
    # apart from the CEM stream and the environment's crop noise: the untagged key gives other words
    assert philox4x32_10([0, DRAW & M32, DRAW >> 32, 32], [SEED & M32, SEED >> 32]) != w[0, :4].tolist()


@pytest.mark.parametrize("hold", [0, 1])
@pytest.mark.parametrize("P,K,S,H", [(2, 3, 5, 3), (1, 1, 1, 1)])
def test_crop_blocks_are_exact(host, P, K, S, H, hold):
    p0, scale = nominal_crop(), 0.2
    n = P * K * S
    blocks = []
    for h in range(H):
        got, _ = run_scenario(host, P, K, S, h, hold, scale, SEED, DRAW, p0, ld=n + 5)
        exp = np_scen_crop(P, K, S, h, hold, scale, SEED, DRAW, p0)
        assert np.array_equal(got[:, :n].view(np.uint32), exp.view(np.uint32)), (h, np.abs(got[:, :n] - exp).max())
        assert (got[:, n:] == 7).all()                                    # nothing past the last child
        blocks.append(got[:, :n])
        b = got[:, :n].reshape(NCROP, P, K, S)
        assert (b == b[:, :, :1]).all()                                   # common random numbers: identical across k for equal (p, s)
        if S > 1:
            assert not (b[:13] == b[:13, :, :, :1]).all()                 # ... and the scenarios differ
        lo, hi = p0[:13].astype(np.float64) * (1 - scale / 2), p0[:13].astype(np.float64) * (1 + scale / 2)
        lo, hi = np.minimum(lo, hi), np.maximum(lo, hi)
        ulp = np.spacing(np.abs(p0[:13])).astype(np.float64)
        g13 = got[:13, :n].astype(np.float64)
        assert (g13 >= (lo - ulp)[:, None]).all() and (g13 <= (hi + ulp)[:, None]).all()
        assert np.array_equal(got[16, :n], got[13, :n] / got[14, :n])     # float32(row 13) / float32(row 14), exactly
    for h in range(1, H):
        assert np.array_equal(blocks[h], blocks[0]) == bool(hold)         # held over the horizon | a fresh draw at every step
    # another scenario draw, another seed: other futures
    other, _ = run_scenario(host, P, K, S, 0, hold, scale, SEED, DRAW + 1, p0)
    assert not np.array_equal(other, blocks[0])
    other, _ = run_scenario(host, P, K, S, 0, hold, scale, SEED + 1, DRAW, p0)
    assert not np.array_equal(other, blocks[0])


def test_scale_zero_gives_the_nominal_block(host):
    p0 = nominal_crop()
    got, _ = run_scenario(host, 2, 3, 5, 1, 0, 0.0, SEED, DRAW, p0)
    exp = p0.copy()
    exp[16] = exp[13] / exp[14]
    assert np.array_equal(got.view(np.uint32), np.broadcast_to(exp[:, None], got.shape).copy().view(np.uint32))


def test_action_plane_is_expanded_per_candidate(host):
    P, K, S = 3, 7, 4
    acts = np.random.default_rng(1).uniform(-1, 1, (P * K, 6)).astype(np.float32)
    _, out = run_scenario(host, P, K, S, 0, 0, 0.2, 1, 0, nominal_crop(), acts)
    assert np.array_equal(out, np.repeat(acts, S, axis=0))


def moment_checks(x):
    """x [N, 34] = u - 0.5: the five-standard-error checks of the module docstring; -> the worst of each."""
    N = x.shape[0]
    worst = np.abs(x.mean(axis=0)).max(), np.abs(x.var(axis=0) - 1 / 12).max()
    assert worst[0] <= 5 * np.sqrt(1 / (12 * N)), worst
    assert worst[1] <= 5 * np.sqrt(1 / (180 * N)), worst
    return worst


def test_moments_of_the_draw(host):
    P, S, H = 8, 16, 32                                                    # 4 096 (p, s, h) triples, 34 parameters each
    ref = np.concatenate([(np_scen_words(P, S, h, 0, MOMENT_SEED, 0).astype(np.float64) + 0.5) * 2.0 ** -32 - 0.5 for h in range(H)])
    w_ref = moment_checks(ref)                                             # the seed's own NumPy restatement passes
    got = np.empty((H * P * S, NCROP))
    for h in range(H):
        for ps in range(P * S):
            host.scenhost_centred(ps, h, 0, MOMENT_SEED, got[h * P * S + ps].ctypes.data)
    assert same_f64(got, ref)
    w = moment_checks(got)
    N = len(got)
    print(f"moments of u - 0.5 over N = {N} per parameter: |mean| {w[0]:.5f} (NumPy {w_ref[0]:.5f}, bound {5 * np.sqrt(1 / (12 * N)):.5f}), "
          f"|var - 1/12| {w[1]:.5f} ({w_ref[1]:.5f}, {5 * np.sqrt(1 / (180 * N)):.5f})")
    # the stored values carry that draw: z / scale recovered from the float32 block to float32 precision
    p0, scale = nominal_crop(), 0.2
    crop, _ = run_scenario(host, P, 1, S, 3, 0, scale, MOMENT_SEED, 0, p0)
    rows = [i for i in range(NCROP) if i != 16 and p0[i] != 0]
    zs = (crop[rows].astype(np.float64) / p0[rows, None].astype(np.float64) - 1.0) / scale
    assert np.abs(zs.T - ref[3 * P * S:4 * P * S][:, rows]).max() <= 2.0 ** -23 / scale


@pytest.mark.parametrize("S,m", AGG_SHAPES)
def test_aggregate_is_the_sequential_sum_of_the_sorted_returns(host, S, m):
    J = 6
    ret, failed, viol, n_steps, ld = aggregate_case(np.random.default_rng(1000 * S + m), J, S)
    rc, fc, vc, sc = run_aggregate(host, J, S, m, ld, ret, failed, viol, n_steps)
    e_rc, e_fc, e_vc, e_sc = py_aggregate(J, S, m, ret, failed, viol, n_steps)
    assert same_f64(rc, e_rc), (rc, e_rc)                                 # NaN where a scenario failed or is not finite: the same bits
    assert np.array_equal(fc, e_fc) and fc.tolist() == [1, 1, 1, 0, 0, 0]
    assert same_f64(vc[:, :J], e_vc) and (vc[:, J:] == 7).all()
    assert np.array_equal(sc, e_sc)
    ok = fc == 0
    if m == S:                                                            # the mean: any order is within S ulps of np.mean
        assert np.allclose(rc[ok], ret.reshape(J, S)[ok].mean(axis=1), rtol=0, atol=S * 2.0 ** -50)
    if m == 1:                                                            # the worst case
        assert np.array_equal(rc[ok], ret.reshape(J, S)[ok].min(axis=1))
    if S >= 2:
        assert len(np.unique(ret[3 * S:4 * S])) < S                       # an admissible row really has ties


def test_aggregate_edge_rows(host):
    # -0.0 and +0.0 tie and are interchangeable: the sum starts at +0.0
    ret = np.array([0.0, -0.0, -0.0, 0.0, -1.5, -1.5, 2.0, -0.0])
    failed = np.zeros(8, np.uint8)
    for m in (1, 2, 4):
        rc, fc, _, _ = run_aggregate(host, 2, 4, m, 8, ret, failed, np.zeros((3, 8)), np.ones(8, np.int32))
        e_rc, e_fc, _, _ = py_aggregate(2, 4, m, ret, failed)
        assert same_f64(rc, e_rc) and np.array_equal(fc, e_fc), m
    assert not np.signbit(run_aggregate(host, 2, 4, 4, 8, ret, failed, np.zeros((3, 8)), np.ones(8, np.int32))[0][0])
    # -inf is not finite either
    ret2 = np.array([1.0, -np.inf, 1.0, 2.0])
    rc, fc, _, _ = run_aggregate(host, 2, 2, 1, 4, ret2, np.zeros(4, np.uint8), np.zeros((3, 4)), np.ones(4, np.int32))
    assert np.isnan(rc[0]) and fc.tolist() == [1, 0] and rc[1] == 1.0
    # risk ordering: worst case <= tail mean <= mean
    rng = np.random.default_rng(3)
    r3, f3 = rng.normal(size=40), np.zeros(40, np.uint8)
    by_m = [run_aggregate(host, 5, 8, m, 40, r3, f3, np.zeros((3, 40)), np.ones(40, np.int32))[0] for m in (1, 2, 8)]
    assert (by_m[0] <= by_m[1]).all() and (by_m[1] <= by_m[2]).all()


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every check happens before the handle is looked at: with good arguments and no handle the refusal names the handle, with a bad
    argument it names the entry point's argument list."""
    import __graft_entry__ as g
    from gl_gym_amd import _lib as L
    if not L.LIB_PATH.exists():
        g.build()
    lib = L.load()
    P_ = 0x1000                                                            # a non-null pointer: never followed, nothing is launched

    def refused(fn, a, null_handle):
        assert fn(None, C.byref(a), None) == L.EINVAL
        return (b"null handle" in lib.glgym_last_error()) == null_handle

    scen = lambda: L.make_plan_args(L.PlanScenarioArgs, 2, 3, 5, 64, 0, 0, 0.2, 1, 0, None, P_, P_, P_)  # noqa: E731
    assert refused(lib.glgym_plan_scenario, scen(), True)
    for field, value in (("struct_size", 8), ("S", 257), ("S", 0), ("scale", -0.1), ("scale", float("nan")), ("scale", float("inf")),
                         ("crop", None), ("h_step", 65536), ("h_step", -1), ("hold", 2), ("ld", 29), ("actions_in", None),
                         ("actions_out", None), ("P", 2 ** 30)):
        a = scen()
        setattr(a, field, value)
        assert refused(lib.glgym_plan_scenario, a, False), field
        assert b"glgym_plan_scenario" in lib.glgym_last_error()
    agg = lambda: L.make_plan_args(L.PlanAggregateArgs, 6, 5, 2, 32, 8, P_, P_, P_, P_, P_, P_, P_, P_)  # noqa: E731
    assert refused(lib.glgym_plan_aggregate, agg(), True)
    for field, value in (("struct_size", 0), ("S", 257), ("S", 0), ("m", 0), ("m", 6), ("J", 0), ("ret", None), ("failed_cand", None),
                         ("ld", 29), ("ld_cand", 5), ("viol", None), ("n_steps", None)):
        a = agg()
        setattr(a, field, value)
        assert refused(lib.glgym_plan_aggregate, a, False), field
        assert b"glgym_plan_aggregate" in lib.glgym_last_error()
    a = agg()
    a.viol = a.viol_cand = a.n_steps = a.steps_cand = None                # the two optional outputs may be left out
    assert refused(lib.glgym_plan_aggregate, a, True)

    def roll():
        step = L.make_step_args(30, 64, P_, P_, None, None, P_, 100, P_, P_, P_, 97, P_, P_, P_, None, P_)
        r = L.make_plan_args(L.PlanRolloutArgs, 3, 0.99, step, P_, None, P_, P_, P_, P_, P_)
        return L.make_plan_args(L.PlanRolloutScenariosArgs, 2, 3, 5, 0, 0.2, 1, 0, None, P_, r)

    assert refused(lib.glgym_plan_rollout_scenarios, roll(), True)
    for path, value in ((("struct_size",), 8), (("S",), 257), (("scale",), -1.0), (("staging",), None), (("hold",), -1),
                        (("rollout", "struct_size"), 4), (("rollout", "controls"), P_), (("rollout", "actions"), None),
                        (("rollout", "H"), 0), (("rollout", "H"), 65537), (("rollout", "gamma"), -1.0), (("rollout", "ret"), None),
                        (("rollout", "step", "crop_p"), None), (("rollout", "step", "B"), 6), (("rollout", "step", "ld"), 29)):
        a = roll()
        obj = a
        for name in path[:-1]:
            obj = getattr(obj, name)
        setattr(obj, path[-1], value)
        assert refused(lib.glgym_plan_rollout_scenarios, a, False), path
        assert b"glgym_plan_rollout_scenarios" in lib.glgym_last_error()
    a = roll()
    a.rollout.controls = P_
    lib.glgym_plan_rollout_scenarios(None, C.byref(a), None)
    assert b"raw-control" in lib.glgym_last_error()


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """tests/scenhost/scenhost.cpp with its own main, AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (nothing is
    loaded into Python): exactly sized heap buffers at the awkward shapes, so an index past a row end is reported."""
    exe = tmp_path / "scenhost_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSCENHOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "scenhost ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
