"""CPU tests of the host twin of tests/bdfwave/ (gl_bdf.hpp on a team of one lane, tests/bdfwave/bdfwave_host.cpp) on every input of
tests/test_gpu_bdf_wave.py against the same references, so that a red GPU test points at the device code and not at the inputs: the
exact cases are exact, the twin takes scipy's path on at least 95 % of the step pairs, the blow-up returns UNDERFLOW.  And every check
of tests/bdf_wave_inputs.py fails on doctored data."""
import numpy as np
import pytest

import bdf_wave_inputs as W


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return W.host_wave(tmp_path_factory.mktemp("bdfwave"))


ONES = np.ones((1, W.NX))
LANE_IDX = np.arange(W.LANES, dtype=np.int32)


def test_reductions_of_the_twin_and_their_checks(host):
    for name, v in W.sum_cases().items():
        s = host.reduce(v[None], LANE_IDX[None], ONES, ONES)[0][0]
        W.check_sum(s, v, name)
    v = W.sum_cases()["cancelling"]
    assert abs(np.sum(np.abs(v)) / np.sum(v)) > 1e11
    serial = np.full(W.LANES, np.cumsum(v)[-1])               # another order of the additions: not the butterfly's bits
    with pytest.raises(AssertionError, match="butterfly"):
        W.check_sum(serial, v)
    good = W.butterfly_sum(v); good[37] = np.nextafter(good[37], 1.0)
    with pytest.raises(AssertionError, match="lanes differ"):
        W.check_sum(good, v)
    for name, (v, idx, want_v, want_i) in W.argmax_cases().items():
        _, av, ai, _ = host.reduce(v[None], idx[None], ONES, ONES)
        W.check_argmax(av[0], ai[0], v, idx, want_v, want_i, name)
    v, idx, want_v, want_i = W.argmax_cases()["tie2_5_37"]
    with pytest.raises(AssertionError):                       # the tie resolved to the larger index
        W.check_argmax(np.full(W.LANES, want_v), np.full(W.LANES, 37, dtype=np.int32), v, idx, want_v, want_i)
    rv, rs = W.rms_cases()
    r = host.reduce(np.zeros((4, W.LANES)), np.zeros((4, W.LANES), dtype=np.int32), rv, rs)[3]
    for k in range(4):
        W.check_rms(r[k], rv[k], rs[k], k)
    with pytest.raises(AssertionError):
        W.check_rms(r[0] * (1 + 1e-14), rv[0], rs[0])


@pytest.fixture(scope="module")
def exact_results(host):
    cases = W.exact_lu_cases()
    A = np.array([W.frac_to_float(c["A"]) for c in cases.values()])
    b = np.array([[float(v) for v in c["b"]] for c in cases.values()])
    out = host.lu(np.array([W.lu_inputs(a) for a in A]), np.ones(len(A)), b)
    return cases, {name: tuple(o[k].copy() for o in out) for k, name in enumerate(cases)}


def test_exact_lu_is_exact_on_the_twin(exact_results):
    cases, res = exact_results
    assert sum(not c["ref"]["ok"] for c in cases.values()) == 3
    for name, c in cases.items():
        W.check_exact_lu(c, *res[name], name)


def test_exact_lu_check_fails_on_doctored_data(exact_results):
    cases, res = exact_results
    ok, LU, piv, perm, x = res["cycle"]
    p2 = perm.copy(); p2[[3, 9]] = p2[[9, 3]]
    with pytest.raises(AssertionError, match="perm"):
        W.check_exact_lu(cases["cycle"], ok, LU, piv, p2, x)
    LU2 = LU.copy(); LU2[4, 11] += 1e-9
    with pytest.raises(AssertionError, match="LU"):
        W.check_exact_lu(cases["cycle"], ok, LU2, piv, perm, x)
    for name in ("tie_keeps_k_13", "tie_later_rows_13", "tie_plus_minus"):
        k, want = cases[name]["tie"]
        ok, LU, piv, perm, x = res[name]
        assert piv[k] == want
        col = np.abs(W.frac_to_float(cases[name]["ref"]["LU"])[:, k])       # the tie is there: a multiplier of magnitude one below k
        assert np.sum(col[k + 1:] == 1.0) == 1
        later = k + 1 + int(np.flatnonzero(col[k + 1:] == 1.0)[0])
        piv2 = piv.copy(); piv2[k] = later                                   # the tie resolved to the larger index
        with pytest.raises(AssertionError, match="piv"):
            W.check_exact_lu(cases[name], ok, LU, piv2, perm, x)
    ok, LU, piv, perm, x = res["singular_13"]
    with pytest.raises(AssertionError, match="flag"):
        W.check_exact_lu(cases["singular_13"], 1, LU, piv, perm, x)


def test_nan_columns_on_the_twin(host):
    for name, (A, row) in W.nan_lu_cases().items():
        ok, LU, piv, perm, x = host.lu(W.lu_inputs(A)[None], np.ones(1), ONES)
        W.check_nan_lu(A, row, ok[0], piv[0], name)
    A, row = W.nan_lu_cases()["one_nan_row_11"]
    piv2 = piv[0].copy(); piv2[:] = np.arange(W.NX)           # a factorisation that chose the NaN row at k = 11
    with pytest.raises(AssertionError, match="NaN row chosen"):
        W.check_nan_lu(A, row, 0, piv2)


@pytest.fixture(scope="module")
def model_host(host, golden):
    x, u, d, p = W.model_rows(golden)
    f, f0, J = host.model_jac(x, u, d, p, True)
    return x, u, d, p, f, f0, J


def test_model_jacobian_of_the_twin(host, hostmath, golden, model_host):
    x, u, d, p, f, f0, J = model_host
    sc = W.rhs_scale(golden)
    ref = np.array([hostmath.rhs(x[k], u[k], np.concatenate([d[k], np.zeros(3)]), p[k]) for k in range(len(x))])
    assert np.array_equal(f, f0)
    _, _, J2 = host.model_jac(x, u, d, p, False, f0=f0)
    assert np.array_equal(J, J2)
    W.check_model_jac(x, sc, f, f0, J, ref, J)
    Jd = J.copy(); Jd[3, 2, 15] += 3e-11 * sc[2] / (1.4901161193847656e-8 * max(abs(x[3, 15]), 1.0))
    with pytest.raises(AssertionError):
        W.check_model_jac(x, sc, f, f0, Jd, ref, J)
    with pytest.raises(AssertionError):
        W.check_model_jac(x, sc, f + 2e-11 * sc, f0, J, ref, J)


def test_general_lu_bounds_hold_on_the_twin_and_fail_on_doctored_data(host, model_host):
    names, J, c, b = W.general_lu_matrices(model_host[6])
    ok, LU, piv, perm, x = host.lu(J, c, b)
    swaps = 0
    for k, name in enumerate(names):
        W.check_general_lu(J[k], c[k], b[k], ok[k], LU[k], piv[k], perm[k], x[k], name)
        swaps += int(np.sum(piv[k] != np.arange(W.NX)))
    assert swaps > 100                                        # pivoting is live
    k = 1
    p2 = perm[k].copy(); p2[[3, 9]] = p2[[9, 3]]
    with pytest.raises(AssertionError, match="perm"):
        W.check_general_lu(J[k], c[k], b[k], ok[k], LU[k], piv[k], p2, x[k])
    i, j = np.unravel_index(np.argmax(np.abs(np.triu(LU[k]))), LU[k].shape)
    LU2 = LU[k].copy(); LU2[i, j] += 1e-9
    with pytest.raises(AssertionError, match="factorisation residual"):
        W.check_general_lu(J[k], c[k], b[k], ok[k], LU2, piv[k], perm[k], x[k])
    x2 = x[k].copy(); x2[5] += 1e-9 * max(1.0, abs(x2[5]))
    with pytest.raises(AssertionError, match="solve residual"):
        W.check_general_lu(J[k], c[k], b[k], ok[k], LU[k], piv[k], perm[k], x2)


def test_change_D_of_the_twin(host):
    D, order, factor = W.change_D_cases()
    assert len(D) <= 64 and sorted(set(order)) == [1, 2, 3, 4, 5]
    out = host.change_D(D, order, factor)
    for k in range(len(D)):
        W.check_change_D(D[k], order[k], factor[k], out[k], k)
    k = int(np.flatnonzero(order == 3)[1])                    # order 3, factor 0.5
    bad = out[k].copy(); bad[2, 7] += 1e-10 * np.abs(D[k, :4, 7]).max()
    with pytest.raises(AssertionError, match="row"):
        W.check_change_D(D[k], order[k], factor[k], bad)
    bad = out[k].copy(); bad[5, 7] = 0.0
    with pytest.raises(AssertionError, match="above the order"):
        W.check_change_D(D[k], order[k], factor[k], bad)


def test_the_twin_takes_scipys_path_on_the_linear_systems(host):
    names = [n for n, _ in W.step_pairs()]
    for family in W.FAMILIES:
        assert any(n.startswith(family) for n in names), family
    y, st, rc = host.step(W.stack(W.linear_problems()))
    share, lines = W.check_steps(y, st, rc, None, match=0.95, label="host")
    print("\n".join(lines))
    S = W.step_systems()
    for name in sorted(set(names)):                           # the pivot order of I - c A: off the diagonal at every step size for the
        if "triangular" in name:                              # pivoting family, at the late, large ones for A = P (Lam + 0.01 T) P^T
            for c in (1.0, 30.0, 300.0):
                piv = host.lu(S[name]["A"][None], np.array([c]), ONES)[2][0]
                assert np.any(piv != np.arange(W.NX)) or (c < 300.0 and name.startswith("permuted")), (name, c)
    y2 = y.copy(); y2[0] += 1e-3
    with pytest.raises(AssertionError):
        W.check_steps(y2, st, rc, y, label="doctored")
    st2 = st.copy(); st2[:4, 3] += 1
    with pytest.raises(AssertionError, match="pairs"):
        W.check_steps(y, st2, rc, y, label="doctored")


def test_van_der_pol_and_the_failure_codes_on_the_twin(host):
    y, st, rc = host.step(W.stack(W.vdp_problems()))
    tr = W.vdp_truth()
    for k, tol in enumerate(W.TOLS):
        print(f"host van der pol tol {tol:g}: rc {rc[k]} stats {st[k].tolist()} error vs Radau 1e-12 {W.wrms(y[k], tr, tol):.3e}")
        assert rc[k] == W.BDF_OK and st[k, 2] >= 2 and np.isfinite(W.wrms(y[k], tr, tol))
    F = W.failure_problems()
    y, st, rc = host.step(W.stack(list(F.values())))
    res = {name: (y[k], st[k], rc[k]) for k, name in enumerate(F)}
    y0, (yk, _, r) = W.SQUARE_Y0, res["square_ok"]
    truth = y0.astype(W.LD) / (1 - y0.astype(W.LD) * W.LD(0.4))
    from scipy.integrate import solve_ivp
    sol = solve_ivp(lambda t, v: v * v, (0.0, 0.4), y0, method="BDF", rtol=1e-8, atol=1e-8)
    print(f"host y' = y^2 to 0.4: error {W.wrms(yk, truth, 1e-8):.3e}, scipy {W.wrms(sol.y[:, -1], truth, 1e-8):.3e}")
    assert r == W.BDF_OK and W.wrms(yk, truth, 1e-8) <= 1.25 * W.wrms(sol.y[:, -1], truth, 1e-8)
    assert res["square_blowup"][2] == W.BDF_FAIL_UNDERFLOW
    assert res["square_step_limit"][2] == W.BDF_FAIL_STEPS and res["square_step_limit"][1][0] == 50
    assert res["square_nan_rhs"][2] not in (W.BDF_OK, -1)
