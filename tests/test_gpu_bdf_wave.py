"""GPU tests of the BDF integrator's wavefront team, piece by piece, through the tests-only module tests/bdfwave/libbdfwave.so (one
64-lane workgroup per problem, the product's own source): the butterfly sum and argmax, bdf_rms, bdf_lu_factor at width 64 with the
register solve, bdf_change_D, the lane layout of eval1 / jac on the model, and bdf_step on systems whose solution is known in closed
form, with the return code a product kernel reduces to NaN.  References: exact rational arithmetic, the a-priori bounds of Gaussian
elimination, closed forms in extended precision, scipy's BDF, and the host twin (tests/test_bdf_wave_host.py holds the twin and the
inputs to the same references on the CPU).  Inputs, references and checks: tests/bdf_wave_inputs.py.
GLGYM_BDF_WAVE_PROFILE=<file> writes every measured figure there (profiles/bdf_wave.txt)."""
import os

import numpy as np
import pytest

import bdf_wave_inputs as W

pytestmark = pytest.mark.gpu

REPORT = []


@pytest.fixture(scope="module")
def dev():
    yield W.device_wave()
    path = os.environ.get("GLGYM_BDF_WAVE_PROFILE")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(REPORT) + "\n")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return W.host_wave(tmp_path_factory.mktemp("bdfwave"))


def say(line):
    REPORT.append(line)
    print(line)


ONES = np.ones((1, W.NX))
LANE_IDX = np.arange(W.LANES, dtype=np.int32)


def test_sum_is_the_butterfly_in_every_lane(dev):
    cases = W.sum_cases()
    V = np.array(list(cases.values()))
    n = len(V)
    s = dev.reduce(V, np.tile(LANE_IDX, (n, 1)), np.tile(ONES, (n, 1)), np.tile(ONES, (n, 1)))[0]
    for k, name in enumerate(cases):
        err, bound = W.check_sum(s[k], V[k], name)
        say(f"sum {name}: |sum - fsum| {err:.3e} bound gamma_6 sum|v| {bound:.3e}")


def test_argmax_largest_value_smallest_index_in_every_lane(dev):
    cases = W.argmax_cases()
    V, I = np.array([c[0] for c in cases.values()]), np.array([c[1] for c in cases.values()])
    assert len(V) <= 64
    _, av, ai, _ = dev.reduce(V, I, np.tile(ONES, (len(V), 1)), np.tile(ONES, (len(V), 1)))
    for k, (name, (v, idx, want_v, want_i)) in enumerate(cases.items()):
        W.check_argmax(av[k], ai[k], v, idx, want_v, want_i, name)
    say(f"argmax: {len(cases)} cases, every lane the largest value and the smallest index among equal values")


def test_rms_norm(dev):
    rv, rs = W.rms_cases()
    r = dev.reduce(np.zeros((4, W.LANES)), np.zeros((4, W.LANES), dtype=np.int32), rv, rs)[3]
    for k in range(4):
        err, bound = W.check_rms(r[k], rv[k], rs[k], k)
        say(f"bdf_rms case {k}: error {err:.3e} bound {bound:.3e}")


def test_lu_on_exact_matrices_bit_for_bit(dev):
    cases = W.exact_lu_cases()
    A = np.array([W.frac_to_float(c["A"]) for c in cases.values()])
    b = np.array([[float(v) for v in c["b"]] for c in cases.values()])
    ok, LU, piv, perm, x = dev.lu(np.array([W.lu_inputs(a) for a in A]), np.ones(len(A)), b)
    for k, (name, c) in enumerate(cases.items()):
        W.check_exact_lu(c, ok[k], LU[k], piv[k], perm[k], x[k], name)
        swaps = int(np.sum((piv[k] != np.arange(W.NX)) & (piv[k] >= 0)))
        say(f"exact LU {name}: flag {ok[k]}, {swaps} swaps, " + ("piv, perm, L, U and the solution equal the rational reference bit for bit"
            if c["ref"]["ok"] else f"singular at column {c['ref']['k_fail']} as the reference, the pivots before it equal"))


def test_lu_with_nan_columns(dev, host):
    cases = W.nan_lu_cases()
    A = np.array([c[0] for c in cases.values()])
    J = np.array([W.lu_inputs(a) for a in A])
    ok, LU, piv, perm, x = dev.lu(J, np.ones(len(A)), np.tile(ONES, (len(A), 1)))
    okh, _, pivh, _, _ = host.lu(J, np.ones(len(A)), np.tile(ONES, (len(A), 1)))
    for k, (name, (a, row)) in enumerate(cases.items()):
        W.check_nan_lu(a, row, ok[k], piv[k], name)
        assert ok[k] == okh[k] and np.array_equal(piv[k], pivh[k]), name
        say(f"NaN LU {name}: flag {ok[k]}, pivots {piv[k].tolist()}")


@pytest.fixture(scope="module")
def model(dev, host, golden):
    x, u, d, p = W.model_rows(golden)
    return dict(x=x, u=u, d=d, p=p, dev=dev.model_jac(x, u, d, p, True), host=host.model_jac(x, u, d, p, True))


def test_model_eval1_and_jac_lane_layout(dev, golden, model):
    x, (f, f0, J), (fh, f0h, Jh) = model["x"], model["dev"], model["host"]
    sc = W.rhs_scale(golden)
    for k in range(len(x)):
        e = W.check_model_jac(x[k:k + 1], sc, f[k:k + 1], f0[k:k + 1], J[k:k + 1], fh[k:k + 1], Jh[k:k + 1], k)
        say(f"model row {k}: |f - host| / sc {e[0]:.2e} (eval1, lane 0), {e[1]:.2e} (need_f0, lane 28), bound 1e-11; "
            f"|J - host| dx / sc {e[2]:.2e}, bound 2e-11")
    _, f0b, Jb = dev.model_jac(x, model["u"], model["d"], model["p"], False, f0=f0)
    assert np.array_equal(f0b, f0) and np.array_equal(Jb, J)  # the columns come from one call site


def test_lu_on_general_matrices_within_the_a_priori_bounds(dev, model):
    names, J, c, b = W.general_lu_matrices(model["dev"][2])
    ok, LU, piv, perm, x = dev.lu(J, c, b)
    for k, name in enumerate(names):
        r1, r2 = W.check_general_lu(J[k], c[k], b[k], ok[k], LU[k], piv[k], perm[k], x[k], name)
        say(f"general LU {name}: |PA - LU| / (gamma_28 |L||U| + forming) {r1:.3f}, |b - Ax| / (gamma_84 P^T|L||U||x| + forming) {r2:.3f}, "
            f"{int(np.sum(piv[k] != np.arange(W.NX)))} swaps")


def test_change_D(dev):
    D, order, factor = W.change_D_cases()
    out = dev.change_D(D, order, factor)
    for k in range(len(D)):
        worst = W.check_change_D(D[k], order[k], factor[k], out[k], k)
        say(f"change_D order {order[k]} factor {factor[k]:.17g}: worst error / (gamma_{8 * order[k] + 2} (|R||U|)^T |D|) {worst:.3f}")


@pytest.fixture(scope="module")
def grid(dev, host):
    """Every step problem in ONE launch: the linear pairs, Van der Pol, the failing ones."""
    F = W.failure_problems()
    problems = W.linear_problems() + W.vdp_problems() + list(F.values())
    assert len(problems) <= 64
    pr = W.stack(problems)
    return dict(problems=problems, n_lin=len(W.linear_problems()), fail=list(F), dev=dev.step(pr), host=host.step(pr))


def test_step_on_linear_systems_against_closed_forms_and_scipy(grid):
    n = grid["n_lin"]
    (y, st, rc), (yh, sth, rch) = grid["dev"], grid["host"]
    _, hl = W.check_steps(yh[:n], sth[:n], rch[:n], None, match=0.95, label="host")
    share, lines = W.check_steps(y[:n], st[:n], rc[:n], yh[:n], match=0.90, label="device")
    for line in hl + lines:
        say(line)


def test_step_van_der_pol(grid):
    n = grid["n_lin"]
    (y, st, rc), (yh, sth, rch) = grid["dev"], grid["host"]
    tr = W.vdp_truth()
    for k, tol in enumerate(W.TOLS):
        e, eh = W.wrms(y[n + k], tr, tol), W.wrms(yh[n + k], tr, tol)
        say(f"van der pol mu 1000 tol {tol:g}: device rc {rc[n + k]} stats {st[n + k].tolist()} error vs Radau 1e-12 {e:.3e}; "
            f"host rc {rch[n + k]} stats {sth[n + k].tolist()} error {eh:.3e}")
        assert rc[n + k] == W.BDF_OK and st[n + k, 2] >= 2
        assert e <= 1.25 * eh


def test_step_failure_codes(grid):
    n = grid["n_lin"] + len(W.TOLS)
    (y, st, rc), (yh, sth, rch) = grid["dev"], grid["host"]
    res = {name: (y[n + k], st[n + k], rc[n + k], yh[n + k], rch[n + k]) for k, name in enumerate(grid["fail"])}
    for name, r in res.items():
        say(f"failure case {name}: device rc {r[2]} stats {r[1].tolist()}, host rc {r[4]}")
    y0 = W.SQUARE_Y0.astype(W.LD)
    truth = y0 / (1 - y0 * W.LD(0.4))
    from scipy.integrate import solve_ivp
    sol = solve_ivp(lambda t, v: v * v, (0.0, 0.4), W.SQUARE_Y0, method="BDF", rtol=1e-8, atol=1e-8)
    yk, _, r, yhk, _ = res["square_ok"]
    e, eh, es = W.wrms(yk, truth, 1e-8), W.wrms(yhk, truth, 1e-8), W.wrms(sol.y[:, -1], truth, 1e-8)
    say(f"y' = y^2 to t = 0.4 at 1e-8: error device {e:.3e} host {eh:.3e} scipy {es:.3e}")
    assert r == W.BDF_OK and e <= 1.25 * max(eh, es)          # the margin of the other step cases
    assert res["square_blowup"][4] == W.BDF_FAIL_UNDERFLOW and res["square_blowup"][2] == W.BDF_FAIL_UNDERFLOW
    assert res["square_step_limit"][2] == W.BDF_FAIL_STEPS and res["square_step_limit"][1][0] == 50
    assert res["square_nan_rhs"][2] in (W.BDF_FAIL_STEPS, W.BDF_FAIL_RHS, W.BDF_FAIL_UNDERFLOW, W.BDF_FAIL_NONFINITE, W.BDF_FAIL_SINGULAR)


def test_mixed_grid_equals_every_problem_alone(dev, grid):
    y, st, rc = grid["dev"]
    for k, p in enumerate(grid["problems"]):
        ya, sta, rca = dev.step(W.stack([p]))
        assert rca[0] == rc[k] and np.array_equal(sta[0], st[k]), k
        assert np.array_equal(ya[0].view(np.int64), y[k].view(np.int64)), k
    say(f"mixed grid: {len(grid['problems'])} problems in one launch, {int(np.sum(rc != 0))} of them failing, each equal bit for bit to "
        f"the same problem sent alone")
