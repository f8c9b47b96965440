"""CPU tests of closed-loop rule-based rollouts: csrc/gl_rule.hpp (host instantiation, tests/rulehost/rulehost.cpp -- a lane is a call)
against a NumPy restatement of the decode written from include/glgym.h and against gl_gym_amd.baseline.RuleBasedController.predict; the
refusals of glgym_rule_rows / glgym_plan_rollout_rule through libglgym.so (no device: every check precedes the handle); the host side
of gl_gym_amd.planner.RuleSearch (RuleParams, check_rule_dt).

Bounds.
* Decode: EXACT (uint64 view).  t = fmin(fmax(theta, -1), 1), half = 0.5 * (t + 1), span = hi - lo, v = lo + span * half: four correctly
  rounded double operations, which NumPy performs in the same order.
* Controls: RULE_RTOL = 1e-12, RULE_ATOL = 1e-14 against predict (tests/envlayer_inputs.py, the project's controller tolerance).
* encode -> decode: theta is the float32 nearest to t in [-1, 1], so |theta - t| <= 2^-24 (half a float32 ulp at 1, the widest in the
  range), and v = lo + (hi - lo) * (theta + 1) / 2 moves by (hi - lo) / 2 times that: |v' - v| <= (hi - lo) * 2^-25, which is inside the
  1 float32 ulp on theta -- (hi - lo) * 2^-24 -- the test allows, plus 8 double roundings at the magnitude of the bounds."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import envlayer_inputs as E

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SRC = ROOT / "tests" / "rulehost" / "rulehost.cpp"
NF, NU = 29, 6
CONFIGS = ("defaults", "distinct", "lamps_overnight", "lamps_never", "lamps_winter", "no_blackout")
BANDS = (11, 14, 16, 19, 22, 26, 27)                             # positions of E.RULE_BANDS in glgym_rule_cfg


def build_host(path):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.rulehost_sizeof.argtypes, lib.rulehost_sizeof.restype = [C.c_int], C.c_int
    lib.rulehost_space_error.argtypes, lib.rulehost_space_error.restype = [C.c_void_p, C.c_char_p, C.c_int], C.c_int
    lib.rulehost_decode.argtypes, lib.rulehost_decode.restype = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p], None
    lib.rulehost_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_void_p]
    lib.rulehost_rows.restype = None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_rule.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    return build_host(tmp_path_factory.mktemp("rulehost") / "librulehost.so")


def make_space(base, fields, lo, hi):
    """A glgym_rule_space from base [29] and the tuned fields with their bounds."""
    from gl_gym_amd import _lib as L
    s = L.RuleSpace()
    s.base = L.RuleCfg(*[float(v) for v in base])
    s.D = len(fields)
    for i, (f, a, b) in enumerate(zip(fields, lo, hi)):
        s.field[i], s.lo[i], s.hi[i] = int(f), float(a), float(b)
    return s


def component(theta, i):
    """Component i of every row of theta [Ht, J, 6]: theta[i / 6][j][i % 6]."""
    return theta[i // NU, :, i % NU]


def np_decode(base, fields, lo, hi, theta, S, B):
    """The constants of rows 0 .. B-1, [B, 29] float64, from the header's text: row b reads theta row b / max(S, 1)."""
    rows = np.arange(B) // max(S, 1)
    cfg = np.tile(np.asarray(base, dtype=np.float64), (B, 1))
    for i, f in enumerate(fields):
        t = np.fmin(np.fmax(component(theta, i)[rows].astype(np.float64), -1.0), 1.0)      # fmax / fmin: a NaN reads as -1
        half = 0.5 * (t + 1.0)
        span = np.float64(hi[i]) - np.float64(lo[i])
        cfg[:, f] = np.float64(lo[i]) + span * half
    return cfg


def host_decode(host, space, theta, J, S, B):
    cfg = np.empty((B, NF), dtype=np.float64)
    host.rulehost_decode(C.addressof(space), theta.ctypes.data, J, S, B, cfg.ctypes.data)
    return cfg


def host_rows(host, space, theta, J, S, X, D, hour, doy):
    B = len(X)
    X, D = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(D, dtype=np.float64)
    hour, doy = np.ascontiguousarray(hour, dtype=np.float64), np.ascontiguousarray(doy, dtype=np.float64)
    U = np.empty((B, NU), dtype=np.float64)
    host.rulehost_rows(C.addressof(space), theta.ctypes.data, J, S, B, X.ctypes.data, D.ctypes.data, D.shape[1], hour.ctypes.data,
                       doy.ctypes.data, U.ctypes.data)
    return U


def bracket(values, fields, seed=0):
    """Bounds around the values of the tuned fields, the value nowhere in the middle, never an interval over 0 -> (lo, hi)."""
    rng = np.random.default_rng([seed, len(fields)])
    v = np.asarray(values, dtype=np.float64)[list(fields)]
    below, above = rng.uniform(0.1, 0.6, len(v)), rng.uniform(0.1, 0.6, len(v))
    w = np.maximum(np.abs(v), 1.0)
    lo, hi = v - below * w, v + above * w
    lo = np.where((v > 0) & (lo <= 0), v * 0.5, lo)              # a band keeps its sign (and the others lose nothing by it)
    hi = np.where((v < 0) & (hi >= 0), v * 0.5, hi)
    return lo, hi


def theta_of(values, fields, lo, hi, J):
    """theta [Ht, J, 6] float32 whose rows all encode `values` (NaN in the padding: it is ignored) -> (theta, the values it decodes to)."""
    Ht = (len(fields) + NU - 1) // NU
    v = np.asarray(values, dtype=np.float64)[list(fields)]
    span = hi - lo
    t = np.where(span > 0, 2.0 * (v - lo) / np.where(span > 0, span, 1.0) - 1.0, 0.0).astype(np.float32)
    flat = np.full((J, Ht * NU), np.nan, dtype=np.float32)
    flat[:, :len(fields)] = t
    theta = np.ascontiguousarray(flat.reshape(J, Ht, NU).transpose(1, 0, 2))
    decoded = np.asarray(values, dtype=np.float64).copy()
    decoded[list(fields)] = lo + span * (0.5 * (np.fmin(np.fmax(t.astype(np.float64), -1.0), 1.0) + 1.0))
    return theta, decoded


def mixed_batch(g, n=12):
    """Rows whose lamp windows differ: lamps_on <, > and == lamps_off, and a day-of-year window that wraps over new year, with clocks
    on both sides of the switching times -> (per-row values [n, 29], X, D, hour, doy)."""
    base = np.asarray(g["defaults_cfg"], dtype=np.float64)
    vals = np.tile(base, (n, 1))
    on_off = [(6.0, 18.0), (18.0, 6.0), (12.0, 12.0)]
    days = [(-1.0, 366.0), (300.0, 60.0), (100.0, 200.0)]
    hour, doy = np.empty(n), np.empty(n)
    for b in range(n):
        vals[b, 0], vals[b, 1] = on_off[b % 3]
        vals[b, 2], vals[b, 3] = days[(b // 3) % 3]
        hour[b] = (5.5, 6.5, 12.0, 17.5, 18.5, 23.0)[b % 6]
        doy[b] = (10.0, 150.0, 330.0, 250.0)[b % 4]
        vals[b, 6] = 18.0 + 0.25 * b                             # every row a day setpoint of its own
    idx = np.arange(n) % len(g["X"])
    D = np.array(g["D"][idx], dtype=np.float64)
    D[:, 0], D[:, 7] = 50.0, 2.0                                 # dim and short of light: the lamps follow their clocks
    return vals, np.array(g["X"][idx]), D, hour, doy


# ---- 1. decode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 1, 3])
@pytest.mark.parametrize("D", [1, 6, 7, 29])
def test_decode_is_exact(host, D, S):
    rng = np.random.default_rng([D, S])
    J = 5
    B = J * max(S, 1) - (1 if S == 3 else 0)                     # B <= J * max(S, 1), once with the last candidate short of a child
    fields = rng.permutation(NF)[:D]
    base = rng.uniform(1.0, 9.0, NF)
    lo = rng.uniform(-5.0, 5.0, D)
    hi = lo + rng.uniform(0.0, 7.0, D)
    hi[0] = lo[0]                                                # an empty interval
    Ht = (D + NU - 1) // NU
    flat = rng.uniform(-1.2, 1.2, (J, Ht * NU)).astype(np.float32)              # flat[j, i] = component i of row j
    special = np.array([-1.0, 1.0, 1.5, -1.5, np.nan, np.inf, -np.inf, -0.0], dtype=np.float32)
    for n, v in enumerate(special):                              # every special value in a component that IS read
        flat[n % J, (n // J + n) % D] = v
    flat[:, D:] = np.nan if D % 2 else 1e30                      # padding garbage
    theta = np.ascontiguousarray(flat.reshape(J, Ht, NU).transpose(1, 0, 2))
    sp = make_space(base, fields, lo, hi)
    got = host_decode(host, sp, theta, J, S, B)
    exp = np_decode(base, fields, lo, hi, theta, S, B)
    assert np.array_equal(got.view(np.uint64), exp.view(np.uint64))
    assert np.isfinite(got).all()                                # no NaN or inf theta reaches a constant
    tuned = got[:, fields]
    assert (tuned >= lo).all() and (tuned <= hi).all()
    if S == 3:                                                   # row b really reads theta row b / 3
        assert np.array_equal(got[0], got[2]) and np.array_equal(got[3], got[5])


def test_padding_is_ignored(host):
    rng = np.random.default_rng(5)
    J, D = 4, 7
    fields, lo = np.arange(D), np.full(D, 1.0)
    hi, base = lo + 2.0, rng.uniform(1, 2, NF)
    theta = rng.uniform(-1, 1, (2, J, NU)).astype(np.float32)
    other = theta.copy()
    other[1, :, 1:] = np.nan
    sp = make_space(base, fields, lo, hi)
    assert np.array_equal(host_decode(host, sp, theta, J, 0, J), host_decode(host, sp, other, J, 0, J))


# ---- 2. the controls of the fixture's configs -----------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 29])
@pytest.mark.parametrize("name", CONFIGS)
def test_controls_of_the_fixture_configs_agree_with_predict(host, golden, name, D):
    from gl_gym_amd import _lib as L
    from gl_gym_amd.baseline import RuleBasedController
    g = golden("controller_kat_configs")
    values = np.asarray(g[f"{name}_cfg"], dtype=np.float64)
    fields = np.arange(NF) if D == NF else np.array([6, 7, 10, 26])          # all 29, or two setpoints, co2_day and a band
    lo, hi = bracket(values, fields, seed=D)
    J = len(g["X"])
    theta, decoded = theta_of(values, fields, lo, hi, J)
    sp = make_space(values, fields, lo, hi)
    for hour_explicit, doy_explicit in ((True, True), (False, False)):
        hour, doy, _ = E.rule_clocks(g, name, hour_explicit, doy_explicit)
        got = host_rows(host, sp, theta, J, 0, g["X"], g["D"], hour, doy)
        ref = RuleBasedController(**dict(zip(L.RULE_FIELDS, decoded))).predict(g["X"], g["D"], hour, doy)
        assert np.allclose(got, ref, rtol=E.RULE_RTOL, atol=E.RULE_ATOL), np.abs(got - ref).max()
    # the decoded constants are the fixture's up to the float32 rounding of theta
    assert np.abs(decoded - values).max() <= np.abs(hi - lo).max() * 2.0 ** -24 + 1e-12


# ---- 3. rows of one batch on different sides of the lamp comparisons ------------------------------------------------------------
def test_rows_take_their_own_side_of_the_lamp_comparisons(host, golden):
    from gl_gym_amd import _lib as L
    from gl_gym_amd.baseline import RuleBasedController
    g = golden("controller_kat_configs")
    vals, X, D, hour, doy = mixed_batch(g)
    n = len(vals)
    fields = np.array([0, 1, 2, 3, 6])
    lo, hi = np.array([0.0, 0.0, -1.0, 0.0, 15.0]), np.array([24.0, 24.0, 366.0, 366.0, 25.0])
    Ht = 1
    theta = np.zeros((Ht, n, NU), dtype=np.float32)
    theta[0, :, :5] = (2.0 * (vals[:, fields] - lo) / (hi - lo) - 1.0).astype(np.float32)
    sp = make_space(vals[0], fields, lo, hi)
    cfg = host_decode(host, sp, theta, n, 0, n)
    # the chosen values are exact in theta (multiples of 1/8 of the intervals would not all be): the three orders survive the decode
    order = np.sign(cfg[:, 0] - cfg[:, 1])
    assert set(order) == {-1.0, 0.0, 1.0} and (cfg[:, 2] > cfg[:, 3]).any() and (cfg[:, 2] < cfg[:, 3]).any()
    got = host_rows(host, sp, theta, n, 0, X, D, hour, doy)
    lamps = set()
    for b in range(n):
        c = RuleBasedController(**dict(zip(L.RULE_FIELDS, cfg[b])))
        ref = c.predict(X[b:b + 1], D[b:b + 1], hour[b:b + 1], doy[b:b + 1])[0]
        assert np.allclose(got[b], ref, rtol=E.RULE_RTOL, atol=E.RULE_ATOL), (b, got[b], ref)
        lamps.add(bool(ref[4] > 0))
    assert lamps == {False, True}                                # lamps on in some rows, off in others


# ---- 4. refusals through the library, no device -------------------------------------------------------------------------------------
def good_space():
    from gl_gym_amd.baseline import RULE_BASED_DEFAULTS
    from gl_gym_amd import _lib as L
    base = [RULE_BASED_DEFAULTS[n] for n in L.RULE_FIELDS]
    return make_space(base, [6, 7, 26], [17.0, 14.0, -3.0], [23.0, 18.0, -0.5])


SPACE_REFUSALS = [("D", 0, b"D outside"), ("D", 30, b"D outside"), ("D", -1, b"D outside"), (("field", 1), 29, b"field index outside"),
                  (("field", 1), -1, b"field index outside"), (("field", 1), 6, b"twice"), (("lo", 0), float("nan"), b"finite"),
                  (("hi", 0), float("inf"), b"finite"), (("lo", 1), 18.5, b"lo > hi"), (("hi", 2), 0.0, b"contains 0"),
                  (("hi", 2), 1.0, b"contains 0"), (("base", "co2Band"), 0.0, b"zero proportional band"),
                  (("base", "thScrPband"), 0.0, b"zero proportional band")]


def set_path(obj, path, value):
    path = path if isinstance(path, tuple) else (path,)
    for name in path[:-1]:
        obj = getattr(obj, name)
    if isinstance(path[-1], int):
        obj[path[-1]] = value
    else:
        setattr(obj, path[-1], value)


def test_search_space_refusals(host):
    sp = good_space()
    assert host.rulehost_space_error(C.addressof(sp), None, 0) == 0
    for path, value, word in SPACE_REFUSALS:
        sp = good_space()
        set_path(sp, path, value)
        msg = C.create_string_buffer(128)
        assert host.rulehost_space_error(C.addressof(sp), msg, 128) == 1 and word in msg.value, (path, msg.value)
    sp = good_space()                                            # a tuned band may have any base value, zero included
    sp.base.tHeatBand = 0.0
    assert host.rulehost_space_error(C.addressof(sp), None, 0) == 0
    from gl_gym_amd import _lib as L
    for i, n in enumerate(E.RULE_BANDS):
        assert L.RULE_FIELDS.index(n) == BANDS[i] and L.RULE_BANDS[i] == n
    assert [host.rulehost_sizeof(i) for i in range(3)] == [C.sizeof(L.RuleSpace), C.sizeof(L.RuleRowsArgs), C.sizeof(L.PlanRolloutRuleArgs)]


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every check happens before the handle is looked at: with good arguments and no handle the refusal names the handle, with a bad
    argument it names the argument."""
    import __graft_entry__ as g
    from gl_gym_amd import _lib as L
    if not L.LIB_PATH.exists():
        g.build()
    lib = L.load()
    P_ = 0x1000                                                  # a non-null pointer: never followed, nothing is launched

    def refused(fn, a, word):
        assert fn(None, C.byref(a), None) == L.EINVAL
        msg = lib.glgym_last_error()
        assert msg and word in msg, (word, msg)

    def rows():
        rule = L.RuleArgs(130, 192, P_, P_, 100, P_, P_, P_, None, None, P_)
        return L.make_plan_args(L.RuleRowsArgs, 44, 3, rule, good_space(), P_)

    refused(lib.glgym_rule_rows, rows(), b"null handle")
    for path, value, word in SPACE_REFUSALS:
        a = rows()
        set_path(a.space, path, value)
        refused(lib.glgym_rule_rows, a, word)
    for path, value, word in (("struct_size", 8, b"struct_size"), ("theta", None, b"null theta"), (("rule", "control"), None, b"control"),
                              (("rule", "ld"), 129, b"ld < B"), (("rule", "B"), 0, b"B < 1"), ("S", -1, b"S outside"),
                              ("S", 257, b"S outside"), ("J", 43, b"B > J"), ("J", 0, b"J < 1"), ("S", 2, b"B > J"),
                              (("rule", "B"), 133, b"B > J"), (("rule", "x"), None, b"null x"), (("rule", "weather"), None, b"null x"),
                              (("rule", "w_off"), None, b"null x"), (("rule", "timestep"), None, b"null x"),
                              (("rule", "weather_rows"), 0, b"weather_rows"), (("rule", "start_day"), None, b"start_day")):
        a = rows()
        set_path(a, path, value)
        refused(lib.glgym_rule_rows, a, word)
        assert b"glgym_rule_rows" in lib.glgym_last_error()
    a = rows()                                                   # S = 0: one row of theta per row
    a.S, a.J = 0, 130
    refused(lib.glgym_rule_rows, a, b"null handle")
    a.J = 129
    refused(lib.glgym_rule_rows, a, b"B > J")
    assert lib.glgym_rule_rows(None, None, None) == L.EINVAL

    def roll(S=3):
        B = 30 if S else 6
        step = L.make_step_args(B, 64, P_, P_, None, None, P_, 100, P_, P_, P_ if S else None, 97, P_, P_, P_, None, P_)
        r = L.make_plan_args(L.PlanRolloutArgs, 3, 0.99, step, None, P_, P_, P_, P_, P_, P_)
        return L.make_plan_args(L.PlanRolloutRuleArgs, 0, r, good_space(), P_, P_, 10 if S else 6, 2, 5, S, 0, 0.2, 1, 0, None)

    for S in (3, 0):
        refused(lib.glgym_plan_rollout_rule, roll(S), b"null handle")
        for path, value, word in SPACE_REFUSALS:
            a = roll(S)
            set_path(a.space, path, value)
            refused(lib.glgym_plan_rollout_rule, a, word)
        for path, value, word in (("struct_size", 8, b"struct_size"), (("rollout", "struct_size"), 4, b"struct_size"),
                                  ("theta", None, b"null theta"), (("rollout", "controls"), None, b"controls"),
                                  (("rollout", "actions"), P_, b"rollout.actions must be NULL"), ("record", 2, b"record"),
                                  ("record", -1, b"record"), (("rollout", "H"), 0, b"H < 1"), (("rollout", "gamma"), -1.0, b"gamma"),
                                  (("rollout", "gamma"), float("nan"), b"gamma"), (("rollout", "gamma"), float("inf"), b"gamma"),
                                  ("S", 257, b"S outside"), ("S", -1, b"S outside"), (("rollout", "step", "ld"), 5, b"step.ld"),
                                  (("rollout", "step", "B"), 0, b"step.B < 1"), ("start_day", None, b"start_day"),
                                  (("rollout", "ret"), None, b"accumulators"), (("rollout", "failed"), None, b"accumulators"),
                                  (("rollout", "step", "reward"), None, b"reward"), (("rollout", "step", "done"), None, b"done")):
            a = roll(S)
            set_path(a, path, value)
            refused(lib.glgym_plan_rollout_rule, a, word)
            assert b"glgym_plan_rollout_rule" in lib.glgym_last_error()
    for path, value in ((("rollout", "step", "B"), 29), ("J", 9), ("J", 30), (("rollout", "step", "crop_p"), None), ("hold", 2),
                        ("scale", -0.5), ("scale", float("nan")), ("P", 0), (("rollout", "H"), 65537)):
        a = roll(3)
        set_path(a, path, value)
        refused(lib.glgym_plan_rollout_rule, a, b"with scenarios")
    a = roll(0)                                                  # without scenarios: step.B <= J, fewer children than rows are fine
    a.J = 5
    refused(lib.glgym_plan_rollout_rule, a, b"step.B <= J")
    a.J = 60
    refused(lib.glgym_plan_rollout_rule, a, b"null handle")
    a = roll(0)                                                  # ... P, K, hold, scale are not looked at, and a long horizon is fine
    a.P, a.hold, a.scale, a.rollout.H = 0, 7, -1.0, 70000
    refused(lib.glgym_plan_rollout_rule, a, b"null handle")
    assert lib.glgym_plan_rollout_rule(None, None, None) == L.EINVAL


# ---- 5. the Python side without a device -------------------------------------------------------------------------------------------
def test_rule_params_argument_checks():
    from gl_gym_amd.baseline import RuleBasedController
    from gl_gym_amd.planner import RuleParams, check_rule_dt
    with pytest.raises(ValueError, match="unknown"):
        RuleParams({"temp_setpoint_day": (17, 23), "temp_setpoint_evening": (1, 2)})
    for empty in ({}, None):
        with pytest.raises(ValueError, match="at least one"):
            RuleParams(empty)
    with pytest.raises(ValueError, match="lo <= hi"):
        RuleParams({"co2_day": (900, 600)})
    with pytest.raises(ValueError, match="finite"):
        RuleParams({"co2_day": (600, float("inf"))})
    with pytest.raises(ValueError, match="contain 0"):
        RuleParams({"tHeatBand": (-2, 0.5)})
    with pytest.raises(ValueError, match="is 0"):
        RuleParams({"co2_day": (600, 900)}, base=RuleBasedController(co2Band=0))
    with pytest.raises(ValueError, match="pair"):
        RuleParams({"co2_day": 600})
    RuleParams({"co2Band": (-200, -50)}, base=RuleBasedController(co2Band=0))      # tuned: its base value is not used
    for dt in (300.0, 100.0, 0.0, 451.0, -900.0):
        with pytest.raises(ValueError, match="450"):
            check_rule_dt(dt)
    for dt in (450.0, 900.0, 1800.0, 3600.0):
        check_rule_dt(dt)
    p = RuleParams({"temp_setpoint_day": (17, 23), "co2_day": (600, 1000)})
    assert (p.D, p.Ht, p.field) == (2, 1, [6, 10]) and p.struct().D == 2 and p.struct().base.lamps_off == 18.0
    with pytest.raises(ValueError, match="outside"):
        p.encode(RuleBasedController(co2_day=1200))
    with pytest.raises(ValueError, match="unknown"):
        p.encode({"co2_night": 3})
    assert not p.inside({"co2_day": 500}) and p.inside(RuleBasedController())


@pytest.mark.parametrize("D", [1, 6, 7, 29])
def test_encode_decode_round_trip(host, D):
    from gl_gym_amd import _lib as L
    from gl_gym_amd.baseline import RULE_BASED_DEFAULTS, RuleBasedController
    from gl_gym_amd.planner import RuleParams
    rng = np.random.default_rng(D)
    names = [L.RULE_FIELDS[i] for i in rng.permutation(NF)[:D]]
    base = RuleBasedController()
    lo, hi = bracket([RULE_BASED_DEFAULTS[n] for n in L.RULE_FIELDS], [L.RULE_FIELDS.index(n) for n in names], seed=D)
    p = RuleParams({n: (a, b) for n, a, b in zip(names, lo, hi)}, base)
    theta = p.encode(base)
    assert theta.shape == ((D + 5) // 6, 1, 6) and theta.dtype == np.float32 and np.abs(theta).max() <= 1.0
    assert (theta.reshape(-1)[D:] == 0).all()                    # padding 0
    dec = p.decode(theta)
    assert list(dec) == names
    for i, n in enumerate(names):
        bound = (hi[i] - lo[i]) * 2.0 ** -24 + 8 * np.finfo(np.float64).eps * max(abs(lo[i]), abs(hi[i]))
        assert dec[n].shape == (1,) and abs(dec[n][0] - RULE_BASED_DEFAULTS[n]) <= bound, (n, dec[n][0], RULE_BASED_DEFAULTS[n], bound)
    # a dict gives the same block as the controller, and the header's own decode (the host instantiation) the same values bit for bit
    assert np.array_equal(p.encode({n: RULE_BASED_DEFAULTS[n] for n in names}), theta)
    sp = p.struct()
    cfg = host_decode(host, sp, np.ascontiguousarray(theta), 1, 0, 1)
    for n in names:
        assert cfg[0, L.RULE_FIELDS.index(n)] == dec[n][0]
    for n in set(L.RULE_FIELDS) - set(names):
        assert cfg[0, L.RULE_FIELDS.index(n)] == RULE_BASED_DEFAULTS[n]
    # the ends of the intervals are exact
    ends = p.decode(np.concatenate([np.full_like(theta, -1.0), np.full_like(theta, 1.0), np.full_like(theta, np.nan)], axis=1))
    for i, n in enumerate(names):
        assert ends[n][0] == lo[i] and abs(ends[n][1] - hi[i]) <= 2 * np.finfo(np.float64).eps * max(abs(lo[i]), abs(hi[i])) and ends[n][2] == lo[i]


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """tests/rulehost/rulehost.cpp with its own main, AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (nothing is
    loaded into Python): exactly sized heap buffers, so an index past a theta row or a control row is reported."""
    exe = tmp_path / "rulehost_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DRULEHOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "rulehost ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
