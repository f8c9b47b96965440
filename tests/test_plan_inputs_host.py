"""The inputs of the planning-kernel edge tests are fair: at every shape and pattern of tests/plan_inputs.py the g++ host instantiations
of the kernels' scalar logic (planhost, cemhost, scenhost, wscenhost, built as their own host tests build them) equal the references
the device is compared with, at the bounds of those host tests: indices, returns, gathered rows, copies, crop blocks, scores and
windows EXACT; sampled actions within np.spacing(np.float32(1)); stored means and refitted values within one float32 ulp.  No GPU.

best_sequence beyond 64 entries (H*6 = 66, 132, 288) is a plain nested loop on the host; the point is that np_select is right before
the device's strided gather is compared with it.  fork has no host instantiation: its reference is checked on its documented rules.

Subnormal temperature: the scalar logic multiplies by 1 / temperature, which is +inf at 2^-1024 and below; the best candidate's own
(ret - max) * inf is 0 * inf = NaN and the whole mean comes back NaN (measured here: all H*6 values of every parent with an admissible
candidate).  glgym_plan_select and Planner.select refuse such a temperature; the arithmetic is unchanged."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import plan_inputs as I
import test_plan_cem_host as cem
import test_plan_scen_host as scen
import test_plan_wscen_host as wscen
from test_plan_host import CSRC, ROOT, ptr, run_select


@pytest.fixture(scope="module")
def planhost(tmp_path_factory):
    so = tmp_path_factory.mktemp("planhost_inputs") / "libplanhost.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(so), str(ROOT / "tests" / "planhost" / "planhost.cpp")])
    lib = C.CDLL(str(so))
    lib.planhost_accumulate.argtypes, lib.planhost_accumulate.restype = [C.c_int, C.c_int] + [C.c_void_p] * 10, None
    lib.planhost_select.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_double, C.c_void_p, C.c_void_p]
    lib.planhost_select.restype = None
    return lib


@pytest.fixture(scope="module")
def cemhost(tmp_path_factory):
    return cem.build_host(tmp_path_factory.mktemp("cemhost_inputs") / "libcemhost.so")


@pytest.fixture(scope="module")
def scenhost(tmp_path_factory):
    return scen.build_host(tmp_path_factory.mktemp("scenhost_inputs") / "libscenhost.so")


@pytest.fixture(scope="module")
def wscenhost(tmp_path_factory):
    return wscen.build_host(tmp_path_factory.mktemp("wscenhost_inputs") / "libwscenhost.so")


# ---- fork: the reference follows the documented rules -------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,P,kind", I.FORK_TABLE)
def test_fork_reference_with_a_table(C_, P, kind):
    par, parent = I.fork_case(C_, P, kind)
    ref = I.fork_reference(par, parent, C_, 1, np.float32)
    if kind == "bad":
        at = list(I.FORK_BAD_AT)
        assert parent[at].tolist() == [-1, P, I.INT32_MIN, I.INT32_MAX]
        assert (ref["alive"][at] == 0).all() and (ref["failed"][at] == 1).all()
        assert np.array_equal(ref["x"][:, at], np.repeat(par["x"].astype(np.float32)[0][:, None], 4, axis=1))
        assert (ref["timestep"][at] == par["timestep"][0]).all()
    ok = ref["failed"] == 0
    assert ok.sum() == C_ - (4 if kind == "bad" else 0) and (ref["alive"] == ok).all()
    assert np.array_equal(ref["w_off"][ok], par["w_off"][parent[ok]])
    assert np.array_equal(ref["crop"][:, ok], par["crop"].astype(np.float32)[parent[ok]].T)
    for k in ("ret", "viol"):
        assert (I.bits(ref[k]) == 0).all()                                      # +0.0 by its bits


@pytest.mark.parametrize("C_,P,K", I.FORK_PLAIN)
def test_fork_reference_without_a_table(C_, P, K):
    par, parent = I.fork_case(C_, P)
    assert parent is None and C_ <= P * K
    ref = I.fork_reference(par, None, C_, K, np.float64)
    for c in (0, C_ // 2, C_ - 1):
        assert np.array_equal(ref["u"][:, c], par["u"][c // K]) and ref["start_day"][c] == par["start_day"][c // K]
    assert ref["alive"].all() and not ref["failed"].any() and not ref["n_steps"].any()


# ---- accumulate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_flags", [False, True])
@pytest.mark.parametrize("alive_kind", I.ACC_ALIVE)
@pytest.mark.parametrize("B", I.ACC_BATCHES)
def test_accumulate_step_is_the_host_logic(planhost, B, alive_kind, with_flags):
    prior = I.accumulate_prior(B, alive_kind)
    w = 1.0
    for call, wk in enumerate(I.ACC_WEIGHTS + (0.99,)):
        reward, info, done, flags = I.accumulate_inputs(B, with_flags, seed=call)
        exp = I.accumulate_step(prior, wk, reward, info, done, flags)
        got = {k: v.copy() for k, v in prior.items()}
        f = np.zeros(B, np.int32) if flags is None else flags
        info3 = np.ascontiguousarray(info[list(I.INFO_VIOL)][None])
        planhost.planhost_accumulate(1, B, ptr(np.array([wk])), ptr(reward), ptr(info3), ptr(done), ptr(f), ptr(got["ret"]), ptr(got["viol"]),
                                     ptr(got["n_steps"]), ptr(got["alive"]), ptr(got["failed"]))
        for k in exp:
            assert np.array_equal(I.bits(got[k]), I.bits(exp[k])), (k, call)
        dead = prior["alive"] == 0
        for k in exp:                                                           # a dead child keeps every accumulator's bits
            assert np.array_equal(I.bits(exp[k][..., dead]), I.bits(prior[k][..., dead])), k
        assert (exp["failed"] >= prior["failed"]).all()                         # failed stays
        if flags is None:
            assert np.array_equal(exp["failed"], prior["failed"])
        prior, w = exp, w * 0.99
    if alive_kind == "mixed" and B > 1:
        assert 0 < (I.accumulate_prior(B, alive_kind)["alive"]).sum() < B


# ---- select -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", I.SELECT_PATTERNS)
@pytest.mark.parametrize("P,K,H", I.SELECT_SHAPES)
def test_select_reference_is_the_host_logic(planhost, P, K, H, pattern):
    ret, failed, actions = I.select_case(P, K, H, pattern)
    for temperature in I.SELECT_TEMPERATURES:
        got = run_select(planhost, P, K, ret, failed, actions, temperature)
        exp = I.select_reference(P, K, ret, failed, actions, temperature)
        ok = exp[0] >= 0
        assert np.array_equal(got[0], exp[0])
        assert np.array_equal(I.bits(got[1][ok]), I.bits(exp[1][ok])) and np.isnan(got[1][~ok]).all()
        assert np.array_equal(I.bits(got[2]), I.bits(exp[2])) and np.array_equal(I.bits(got[3]), I.bits(exp[3]))     # all H*6 entries
        assert I.within_one_f32_ulp(got[4], exp[4]), (temperature, np.abs(got[4] - exp[4]).max())
    check_pattern(P, K, pattern, ret, failed, exp)


def check_pattern(P, K, pattern, ret, failed, exp):
    """What each pattern is there for, on the reference's own output."""
    best_k, best_ret = exp[0], exp[1]
    for p in range(P):
        if pattern == "last":
            assert best_k[p] == K - 1
        elif pattern == "ties":
            a, b = I.tie_pair(p, K)
            assert best_k[p] == a and ret[p * K + a] == ret[p * K + b]
        elif pattern == "zeros":
            assert best_k[p] == K // 3 and I.bits(best_ret[p:p + 1])[0] == 1 << 63        # the lower k's -0.0, not the +0.0 behind it
        elif pattern in ("failed", "nan"):
            assert best_k[p] == -1 and np.isnan(best_ret[p]) and not exp[3][:, p].any() and not exp[4][:, p].any()


def test_extreme_temperatures_are_the_tied_and_the_plain_mean(planhost):
    P, K, H = 3, 129, 11
    ret, failed, actions = I.select_case(P, K, H, "ties")
    cold = run_select(planhost, P, K, ret, failed, actions, 1e-300)[5]
    hot = run_select(planhost, P, K, ret, failed, actions, 1e300)[5]
    for p in range(P):
        a, b = I.tie_pair(p, K)
        tied = (actions[:, p * K + a].astype(np.float64) + actions[:, p * K + b]) / 2
        assert np.abs(cold[:, p] - tied).max() <= 2.0 ** -52
        adm = (failed[p * K:(p + 1) * K] == 0) & np.isfinite(ret[p * K:(p + 1) * K])
        plain = actions[:, p * K:(p + 1) * K][:, adm].astype(np.float64).mean(axis=1)
        assert np.abs(hot[:, p] - plain).max() <= 1e-12                         # test_plan_host's bound on the double accumulators


def test_a_subnormal_temperature_gives_nan_and_is_refused(planhost):
    from gl_gym_amd.planner import _select_temperature
    P, K, H = 3, 65, 2
    ret, failed, actions = I.select_case(P, K, H, "random")
    got = run_select(planhost, P, K, ret, failed, actions, I.SMALLEST_SUBNORMAL)
    assert (got[0] >= 0).all() and np.isnan(got[4]).all() and got[4].size == H * P * 6     # 0 * inf: every mean of every parent
    edge = float(np.nextafter(2.0 ** -1024, 1.0))                               # the smallest temperature whose reciprocal is finite
    assert np.isfinite(1.0 / edge) and np.isinf(1.0 / float(np.nextafter(edge, 0.0)))
    fine = run_select(planhost, P, K, ret, failed, actions, edge)
    exp = I.select_reference(P, K, ret, failed, actions, 1e-300)                # both: the mean over the exactly tied maxima
    assert np.isfinite(fine[4]).all() and I.within_one_f32_ulp(fine[4], exp[4])
    assert _select_temperature(edge) == edge and _select_temperature(0.05) == 0.05
    for bad in (I.SMALLEST_SUBNORMAL, float(np.nextafter(edge, 0.0)), 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            _select_temperature(bad)
    src = (ROOT / "greenlight-gym2_amd" / "csrc" / "glgym_search.hip").read_text()
    assert "glgym_plan_select: temperature is too small" in src and "2^-1024" in (ROOT / "include" / "glgym.h").read_text()


# ---- sample -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,K,H,beta", I.SAMPLE_COMBOS)
def test_sample_reference_is_the_host_logic(cemhost, P, K, H, beta):
    mean, std, prev = I.sample_case(P, K, H)
    D = I.DRAW + I.BASE
    fresh = cem.run_sample(cemhost, P, K, H, mean, std, beta, I.SEED, D)
    exp, exact = I.np_sample(P, K, H, mean, std, beta, I.SEED, D)
    assert np.abs(fresh.astype(np.float64) - exp).max() <= I.F32_STEP and (np.abs(fresh) <= 1).all()
    assert np.array_equal(fresh[:, exact], exp[:, exact].astype(np.float32)) and exact.sum() == P
    for invalid in (False, True):
        carry, elite, n_elite = I.carry_tables(P, K, invalid)
        got = cem.run_sample(cemhost, P, K, H, mean, std, beta, I.SEED, D, carry, carry, prev, elite, n_elite)
        exp, exact = I.np_sample(P, K, H, mean, std, beta, I.SEED, D, carry, carry, prev, elite, n_elite)
        assert np.abs(got.astype(np.float64) - exp).max() <= I.F32_STEP
        assert np.array_equal(I.bits(got[:, exact]), I.bits(exp[:, exact].astype(np.float32)))
        assert np.array_equal(I.bits(got[:, ~exact]), I.bits(fresh[:, ~exact]))        # not followed = sampled as without carry
        copies = sum(sum(1 for k in range(1, min(carry, K - 1) + 1) if k - 1 < n_elite[p] and 0 <= elite[p, k - 1] < K) for p in range(P))
        assert exact.sum() == P + copies
        if not invalid:                                                         # with valid tables: what today's callers get
            old, old_exact = cem.np_sample(P, K, H, mean, std, beta, I.SEED, D, carry, prev, elite, n_elite)
            assert np.array_equal(old, exp) and np.array_equal(old_exact, exact)
        elif K > 4:
            assert copies < sum(min(carry, int(n)) for n in n_elite)           # some index really was not followed


# ---- elites -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", I.ELITE_PATTERNS)
@pytest.mark.parametrize("P,K,E", I.ELITE_SHAPES)
def test_elites_reference_is_the_host_logic(cemhost, P, K, E, pattern):
    ret, failed = I.elites_case(P, K, E, pattern)
    got = cem.run_elites(cemhost, P, K, E, ret, failed)
    exp = I.np_elites(P, K, E, ret, failed)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    check_elites_pattern(P, K, E, pattern, ret, exp)


def check_elites_pattern(P, K, E, pattern, ret, exp):
    elite, n = exp
    if pattern == "equal":
        assert (elite == np.arange(E)).all()
    elif pattern == "increasing":
        assert (elite == K - 1 - np.arange(E)).all()
    elif pattern == "none":
        assert (elite == -1).all() and not n.any()
    elif pattern in ("E-1", "E", "E+1"):
        want = min(max(E + {"E-1": -1, "E": 0, "E+1": 1}[pattern], 0), K)
        assert (n == min(want, E)).all() and ((elite >= 0).sum(axis=1) == min(want, E)).all()
    elif pattern == "pairs":
        for a, b in ((63, 64), (255, 256)):
            if b < K:
                assert (ret.reshape(P, K)[:, a] == ret.reshape(P, K)[:, b]).all()
                for p in range(P):
                    row = elite[p].tolist()
                    if a in row and b in row:
                        assert row.index(b) == row.index(a) + 1                 # the tie goes to the lower index, side by side


# ---- refit --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,min_std", I.REFIT_PARAMS)
@pytest.mark.parametrize("variant", I.REFIT_VARIANTS)
@pytest.mark.parametrize("P,K,H,E", I.REFIT_SHAPES)
def test_refit_reference_is_the_host_logic(cemhost, P, K, H, E, variant, alpha, min_std):
    actions, elite, n_elite, n_ref, mean, std = I.refit_case(P, K, H, E, variant)
    mo, so, _, _ = cem.run_refit(cemhost, P, K, H, E, actions, elite, n_elite, alpha, min_std, mean, std)
    e_mo, e_so = I.refit_reference(P, K, H, actions, elite, n_ref, alpha, min_std, mean, std)
    assert I.within_one_f32_ulp(mo, e_mo) and I.within_one_f32_ulp(so, e_so)
    check_refit_variant(P, variant, alpha, min_std, n_ref, mean, std, mo, so)
    mi, si = mean.copy(), std.copy()
    cem.run_refit(cemhost, P, K, H, E, actions, elite, n_elite, alpha, min_std, mi, si, in_place=True)
    assert np.array_equal(I.bits(mi), I.bits(mo)) and np.array_equal(I.bits(si), I.bits(so))


def check_refit_variant(P, variant, alpha, min_std, n_ref, mean, std, mo, so):
    for p in range(P):
        if n_ref[p] == 0:                                                       # no elite, a count below 0, or an index outside 0..K-1: kept
            assert np.array_equal(I.bits(mo[:, p]), I.bits(mean[:, p])) and np.array_equal(I.bits(so[:, p]), I.bits(std[:, p]))
    if variant == "full" and alpha == 0.0 and min_std == 0.0:
        assert (so[:, 0] == 0).all()                                            # identical elite rows: a spread of exactly 0
    if variant == "invalid":
        assert n_ref[0] == 0 and (P < 2 or n_ref[1] == 0)


# ---- scenario, aggregate ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,K,S", I.SCEN_SHAPES)
def test_scenario_reference_is_the_host_logic(scenhost, P, K, S):
    n, acts = P * K * S, I.scenario_actions(P, K)
    for h, hold, scale, pair, base in I.SCEN_CALLS:
        D = I.DRAW + (I.BASE if base else 0)
        got, out = scen.run_scenario(scenhost, P, K, S, h, hold, scale, I.SEED, D, I.crop_p0(), acts if pair else None, ld=n + I.PAD)
        exp = I.scenario_reference(P, K, S, h, hold, scale, I.SEED, D)
        assert np.array_equal(I.bits(got[:, :n]), I.bits(exp)) and (got[:, n:] == 7).all()
        if pair:
            assert np.array_equal(I.bits(out), I.bits(np.repeat(acts, S, axis=0)))
        if scale == 0.0:
            nominal = I.crop_p0().copy()
            nominal[16] = nominal[13] / nominal[14]
            assert (exp == nominal[:, None]).all()


@pytest.mark.parametrize("J,S,m,kind", I.AGG_CASES)
def test_aggregate_reference_is_the_host_logic(scenhost, J, S, m, kind):
    ret, failed, viol, n_steps, ld = I.aggregate_edge_case(J, S, m, kind)
    rc, fc, vc, sc = scen.run_aggregate(scenhost, J, S, m, ld, ret, failed, viol, n_steps)
    e_rc, e_fc, e_vc, e_sc = I.py_aggregate(J, S, m, ret, failed, viol, n_steps)
    assert I.same_f64(rc, e_rc) and np.array_equal(fc, e_fc) and I.same_f64(vc[:, :J], e_vc) and np.array_equal(sc, e_sc)
    if kind == "equal":
        assert e_rc[0] == -1.25
    if kind == "case":
        assert e_rc[5] == 2.5 and e_fc.tolist()[:6] == [1, 1, 1, 0, 0, 0]


# ---- weather windows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("P,S,H,K,nd,rows,first", I.WEATHER_CASES)
def test_weather_reference_is_the_host_logic(wscenhost, P, S, H, K, nd, rows, first, dtype):
    weather = I.table(dtype, rows=rows, nd=nd)
    w_off, ts, kinds = I.weather_parents(P, H, rows, first)
    D = I.DRAW + I.BASE
    got, child = wscen.run_window(wscenhost, P, K, S, H, weather, w_off, ts, I.SIGMA, I.PHI, I.SEED, D, pad=I.PAD)
    exp, exp_child = I.weather_reference(P, K, S, H, weather, w_off, ts, I.PHI, I.SEED, D)
    n = P * S * H
    assert np.array_equal(I.bits(got[:n]), I.bits(exp)) and (got[n:] == -7).all()
    assert np.array_equal(child[:P * K * S], exp_child) and (child[P * K * S:] == -7).all()
    win = exp.reshape(P, S, H, nd)
    for p, kd in enumerate(kinds):
        first_row = min(max(int(w_off[p]) + int(ts[p]), 0), rows - 1)
        assert np.array_equal(I.bits(win[p, :, 0]), I.bits(np.repeat(weather[first_row][None], S, axis=0)))      # h = 0: a measurement
        assert np.array_equal(I.bits(win[p, 0, :, 7:]), I.bits(weather[np.clip(int(w_off[p]) + int(ts[p]) + np.arange(H), 0, rows - 1), 7:]))
        if kd == "negative":
            assert int(w_off[p]) + int(ts[p]) < 0 and first_row == 0             # the lower clamp
        if kd in ("beyond", "straddle") and rows > 1:
            assert int(w_off[p]) + int(ts[p]) + H - 1 >= rows - 1
        if kd == "far":
            assert exp_child[p * K * S] == p * S * H + 2 ** 30
