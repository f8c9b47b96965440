"""Held-out off-trajectory one-step maps (VERDICT weak item 4, next-round item 3) on the CPU: tests/golden/holdout_stress.npz (with
_part2 and _bdf; make_golden.py g_holdout_stress) holds 1 025 tuples of oracle/studies/stress_sc.py's five kinds from seeds that nothing
else in the tree draws from, a truth that no integrator of the project produced (Radau 1e-11 cross-checked with plain RK4 at 32 768
sub-steps, else RK4 32 768 against 16 384), and beside it what the REFERENCE code gives per tuple: the oracle's fp64 state, failed flag,
step_flags word and error for ls5-128 window 2 (throughput) and ls5-192 window 1 (parity), each unverified and verified; the error of
the product's fp32 host build on the same four; the CPU BDF port's rows at 1e-6 and 1e-8.  Checked here: the fixture itself, that the
recorded verdicts reproduce, the conditions the reference alone must meet, and the judging code that tests/test_gpu_holdout_stress.py
holds the kernels to.  Nothing is regenerated.

The fp32 margin.  m32[c] is the largest |error of the fp32 host build - error of the fp64 oracle| over the tuples whose oracle error lies
in [5e-5, 2e-4]: what fp32 rounding does to this metric near the bar, measured on reference code.  A tuple is in configuration c's
ALLOWED set -- an fp32 kernel may be above the bar on it -- if its recorded oracle error or its recorded fp32-host error exceeds
1e-4 - 2 m32[c]: the kernel may differ from the host fp32 build by as much again as that build differs from fp64."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from conftest import STATE_NAMES
from test_jump_fixture import COLMAX, judge, sce

N_ROWS = 1025
CONFIGS = ("throughput", "throughput_verified", "parity", "parity_verified")      # ls5 (128, window 2), (192, window 1); the fixture's order
VERIFIED = (1, 3)
BAR = 1e-4
CLEAN, FLOOR, REAL = 0, 1, 2
KIND_NAMES = ("spun-up", "extreme weather", "corner controls", "off-trajectory state", "control jump")


def verdicts(got, truth, abs_floor=1e-4):
    """tests/test_jump_fixture.py::judge per row: REAL (a state above 1e-4 that is not at the metric's floor), FLOOR (above 1e-4 only in
    temperatures within 1e4 x abs_floor of 0 C that are off by less than abs_floor kelvin) or CLEAN."""
    e = sce(got, truth)
    bad = e > BAR
    floor = bad & (np.abs(got - truth) < abs_floor) & (np.arange(28)[None, :] < 22) & (np.abs(truth) < 1e4 * abs_floor)
    v = np.where((bad & ~floor).any(axis=1), REAL, np.where(floor.any(axis=1), FLOOR, CLEAN))
    assert (int((v == REAL).sum()), int((v == FLOOR).sum())) == judge(got, truth, abs_floor)
    return v


def param_blocks(g, p0):
    """[n, 208] per-row parameter blocks: the default block with each row's p[128..161]."""
    P = np.tile(np.asarray(p0, dtype=np.float64), (len(g["X"]), 1))
    P[:, 128:162] = g["P_crop"].astype(np.float64)
    return P


def allowed(g, c):
    """Rows on which an fp32 kernel may be a real offender in configuration c (the module docstring)."""
    cut = BAR - 2.0 * float(g["m32"][c])
    return (g["e_oracle"][c] > cut) | (g["e_host32"][c] > cut)


def verdict_mismatches(got, g, c):
    """Rows of an fp64 result whose verdict differs from the recorded oracle's in configuration c."""
    return np.flatnonzero(verdicts(got, g["X_tight"]) != verdicts(g["X_oracle"][c], g["X_tight"]))


def classification(g, b):
    """The table of the issue from the recorded data -> lines."""
    XT, kind = g["X_tight"], g["kind"]
    lines = [f"{len(XT)} tuples, per kind {np.bincount(kind, minlength=5).tolist()} ({', '.join(KIND_NAMES)}); "
             f"{int(g['crop_flag'].sum())} with a crop block; truth by fine RK4 on {int((g['truth_kind'] == 1).sum())}"]

    def describe(name, Y, failed, extra=""):
        v = verdicts(Y, XT)
        e = sce(Y, XT)
        real = np.flatnonzero(v == REAL)
        lines.append(f"{name:34s} real above 1e-4: {len(real):3d}  at the floor only: {int((v == FLOOR).sum()):3d}  failed: {int(failed.sum())}  "
                     f"max error {e.max():.1e} (row {int(e.max(axis=1).argmax())}, {STATE_NAMES[int(e.max(axis=0).argmax())]}){extra}")
        if len(real):
            states = sorted({STATE_NAMES[j] for i in real for j in np.flatnonzero(e[i] > BAR)})
            lines.append(f"{'':34s} real offenders by kind {np.bincount(kind[real], minlength=5).tolist()}, states {states}, rows {real.tolist()}")
        fl = np.flatnonzero(v == FLOOR)
        if len(fl):
            lines.append(f"{'':34s} floor rows by kind {np.bincount(kind[fl], minlength=5).tolist()}, rows {fl.tolist()}")
    for c, name in enumerate(CONFIGS):
        describe(f"oracle fp64 ls5 {name}", g["X_oracle"][c], g["failed"][c],
                 f"; fp32 host build max {g['e_host32'][c].max():.1e}, m32 {g['m32'][c]:.1e}, fp32-allowed rows {int(allowed(g, c).sum())}")
    for t, tol in enumerate(b["tols"]):
        rhs = b["bdf_stats"][t][:, 1]
        describe(f"oracle.bdf rtol = atol = {tol:g}", b["X_bdf"][t], b["bdf_status"][t] != 0, f"; RHS evaluations mean {rhs.mean():.0f} max {rhs.max()}")
    return lines


def test_fixture_is_what_it_says(golden):
    g, b, jump = golden("holdout_stress"), golden("holdout_stress_bdf"), golden("step_tight_jump")
    p0 = golden("params_default")["p"]
    n = len(g["X"])
    assert n == N_ROWS and [str(s) for s in g["config_names"]] == list(CONFIGS)
    assert g["configs"].tolist() == [[128, 2, 0], [128, 2, 1], [192, 1, 0], [192, 1, 1]] and b["tols"].tolist() == [1e-6, 1e-8]
    counts = np.bincount(g["kind"], minlength=5)
    assert counts[3] >= 384 and all(counts[k] >= 128 for k in (0, 1, 2, 4)) and np.array_equal(g["kind"], g["seed"] % 5)
    assert np.all(g["truth_agreement"] < 2e-7) and np.all(np.isfinite(g["X_tight"])) and np.all(np.isfinite(g["X"]))
    seeds = g["seed"]
    assert len(set(seeds.tolist())) == n and np.all(np.diff(seeds) > 0) and int(g["seed_base"]) == seeds.min() - seeds.min() % 5
    assert not set(seeds.tolist()) & set(jump["seed"].tolist()) and np.all(seeds >= 20000)       # the studies draw from 0 ... 19 999
    # a third of the rows carry a crop block; the others hold the default block
    share = g["crop_flag"].mean()
    assert 0.30 < share < 0.37, share
    default = np.asarray(p0, dtype=np.float32)[128:162]
    assert np.all((g["P_crop"] == default).all(axis=1) == ~g["crop_flag"])
    noisy = g["P_crop"][g["crop_flag"]]
    rel = np.abs(noisy / default - 1)
    assert np.delete(rel, 16, axis=1).max() < 0.1001             # noise.py at scale 0.1 ...
    assert np.array_equal(noisy[:, 16], noisy[:, 13] / noisy[:, 14])                               # ... with p[144] = p[141] / p[142] in float32
    # no recorded error where a last-bit difference could flip the verdict
    for e in (g["e_oracle"], g["e_host32"], b["e_bdf"]):
        assert e.shape[1] == n and np.all(np.isfinite(e)) and np.all(np.abs(e / BAR - 1) >= 1e-6)
    for c in range(4):
        assert np.array_equal(g["e_oracle"][c], sce(g["X_oracle"][c], g["X_tight"]).max(axis=1))
        band = (g["e_oracle"][c] >= 5e-5) & (g["e_oracle"][c] <= 2e-4)
        want = np.abs(g["e_host32"][c] - g["e_oracle"][c])[band].max() if band.any() else 0.0
        assert g["m32"][c] == want
    for t in range(2):
        assert np.array_equal(b["e_bdf"][t], sce(b["X_bdf"][t], g["X_tight"]).max(axis=1))


def test_recorded_verdicts_reproduce(golden, oracle, hostmath):
    """Every eighth tuple: the oracle's four configurations and the BDF port's two tolerances again, bit for bit; the fp32 host build's
    error to 1e-9 (its libm calls are not pinned to the last bit across C libraries; the allowed set is cut at 1e-4 - 2 m32, never
    nearer than 1e-6 relative to a recorded error -- the test below)."""
    g, b = golden("holdout_stress"), golden("holdout_stress_bdf")
    P = param_blocks(g, golden("params_default")["p"])
    X, U, D, XT = g["X"], g["U"], g["D"], g["X_tight"]
    oracle.lib()

    def run(i):
        out = []
        for c, (n_sub, window, verify) in enumerate(g["configs"].tolist()):
            y, retries, refined, failed, flags = oracle.rk_sc_guarded(X[i], U[i], D[i], P[i], 900.0, n_sub, 5, window, verify=bool(verify), want_flags=True)
            y32 = hostmath.step_guarded(X[i], U[i], D[i], P[i], True, 900.0, n_sub, 5, window, verify=bool(verify))
            out.append((y, failed, flags, float(sce(y32[0], XT[i]).max())))
        bdf = [oracle.bdf(X[i], U[i], D[i], P[i], 900.0, tol, tol) for tol in b["tols"]]
        return out, bdf
    rows = list(range(0, len(X), 8))
    with ThreadPoolExecutor(8) as ex:
        R = list(ex.map(run, rows))
    for i, (out, bdf) in zip(rows, R):
        for c, (y, failed, flags, e32) in enumerate(out):
            assert np.array_equal(y.view(np.uint64), g["X_oracle"][c][i].view(np.uint64)), (i, c)
            assert failed == bool(g["failed"][c][i]) and flags == int(g["flags"][c][i]), (i, c, flags)
            assert abs(e32 - g["e_host32"][c][i]) <= 1e-9, (i, c, e32, g["e_host32"][c][i])
        for t, (y, nfev, st) in enumerate(bdf):
            assert np.array_equal(y.view(np.uint64), b["X_bdf"][t][i].view(np.uint64)), (i, t)
            assert [int(st[0]), nfev, int(st[1]), int(st[2]), int(st[3])] == b["bdf_stats"][t][i].tolist() and b["bdf_status"][t][i] == 0


def test_conditions_the_reference_alone_meets(golden):
    g, b = golden("holdout_stress"), golden("holdout_stress_bdf")
    XT = g["X_tight"]
    assert not g["failed"].any() and not b["bdf_status"].any() and np.all(np.isfinite(b["X_bdf"])) and np.all(np.isfinite(g["X_oracle"]))
    for c in VERIFIED:
        assert judge(g["X_oracle"][c], XT)[0] == 0, CONFIGS[c]                  # verified: nothing real above the bar
    assert judge(g["X_oracle"][0], XT)[0] >= 1                                  # unverified throughput: the fixture does bite
    for c in range(4):
        a = allowed(g, c)
        assert a.mean() <= 0.02, (CONFIGS[c], int(a.sum()))
        assert np.all(a[verdicts(g["X_oracle"][c], XT) == REAL])                # what the oracle itself misses is allowed, by construction
    for t in range(2):                                                          # the BDF port at either tolerance: nothing real
        assert judge(b["X_bdf"][t], XT)[0] == 0


def test_classification(golden):
    """The table DESIGN.md section 2.8 is written from."""
    print("\n".join(classification(golden("holdout_stress"), golden("holdout_stress_bdf"))))


def test_a_wrong_row_would_be_caught(golden):
    """The judging code's self-check: one clean row of a copy of the recorded verified results moved by 2e-4 (scaled) in one state -- the
    verdict comparison and the state comparison of tests/test_gpu_holdout_stress.py both fail, and only on that row."""
    g = golden("holdout_stress")
    XT = g["X_tight"]
    for c in VERIFIED:
        ref = g["X_oracle"][c]
        assert len(verdict_mismatches(ref.copy(), g, c)) == 0
        row = int(np.flatnonzero((verdicts(ref, XT) == CLEAN) & ~allowed(g, c))[100])
        for state in (0, 2, 25):                                                # a concentration, a temperature, a crop state
            got = ref.copy()
            got[row, state] += 2e-4 * max(abs(XT[row, state]), 1e-3 * COLMAX[state])
            if state == 2 and abs(XT[row, state]) < 1.0:                        # a temperature at the floor would be excused: not this check's row
                continue
            assert verdict_mismatches(got, g, c).tolist() == [row], (c, row, state)
            assert np.flatnonzero(state_difference(got, ref, g["X"]) > 1e-11).tolist() == [row]
            assert verdicts(got, XT, 2e-4)[row] == REAL and not allowed(g, c)[row]      # the fp32 rule: an offender outside the allowed set


def state_difference(got, ref, X):
    """tests/test_gpu_fuzz.py's metric per row: max over the states of |got - ref| / max(|ref|, column max of |X|, 1e-3)."""
    scale = np.maximum(np.abs(X).max(axis=0), 1e-3)
    return np.max(np.abs(got - ref) / np.maximum(np.abs(ref), scale), axis=1)
