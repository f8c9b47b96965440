"""Inputs, references, checks and the Python side of tests/bdfwave/ (tests/test_gpu_bdf_wave.py on the device module,
tests/test_bdf_wave_host.py on its host twin).

The device module runs the pieces of the BDF integrator's wavefront team -- WaveTeam::sum / argmax / lu_solve / jac, bdf_lu_factor at
width 64, bdf_change_D, bdf_rms, bdf_step -- one 64-lane workgroup per problem; the host twin runs the same source on a team of one.
Every reference here is independent of both: exact rational arithmetic (fractions.Fraction), math.fsum, the a-priori bounds of
Gaussian elimination (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 9.3 / 9.4), closed-form solutions of linear
ODE systems in extended precision or mpmath, and scipy's BDF (the published implementation gl_bdf.hpp cites).
Each check is a function over plain arrays, so the CPU test can show on doctored data that it can fail."""
import ctypes as C
import functools
import math
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
WAVEDIR = ROOT / "tests" / "bdfwave"
NX, LANES, NROWD = 28, 64, 8
U_ROUND = 2.0 ** -53                                          # unit roundoff of double
BDF_OK, BDF_FAIL_STEPS, BDF_FAIL_RHS, BDF_FAIL_UNDERFLOW, BDF_FAIL_NONFINITE, BDF_FAIL_SINGULAR = range(6)
RHS_LINEAR, RHS_SQUARE, RHS_VDP, RHS_SQUARE_NAN = range(4)
LD = np.longdouble


def gamma(n):
    """gamma_n = n u / (1 - n u) in extended precision."""
    return LD(n) * LD(U_ROUND) / (LD(1) - LD(n) * LD(U_ROUND))


# ---------------------------------------------------------------------------------------------------------------------------------
# the two modules
class _HostPtr:
    def __init__(self, a):
        self.a = a


class Wave:
    """The five entry points over numpy arrays.  device=False: the host twin (host pointers); True: libbdfwave.so (device pointers of
    torch tensors and the current stream)."""

    def __init__(self, lib, device):
        self.lib, self.device = lib, device
        for name in ("reduce", "lu", "change_D", "step", "model_jac"):
            getattr(lib, "bdfwave_" + name).restype = C.c_int

    def _run(self, name, args, outs):
        fn = getattr(self.lib, "bdfwave_" + name)
        for a in args:
            assert not isinstance(a, np.ndarray) or a.flags.c_contiguous
        if not self.device:
            rc = fn(*[C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else C.c_void_p(a.a.ctypes.data) if isinstance(a, _HostPtr)
                      else a for a in args])
            assert rc == 0, (name, rc)
            return
        import torch
        ts = [torch.from_numpy(a).cuda() if isinstance(a, np.ndarray) else a for a in args]
        cargs = [C.c_void_p(t.data_ptr()) if torch.is_tensor(t) else C.c_void_p(t.a.ctypes.data) if isinstance(t, _HostPtr) else t
                 for t in ts]
        rc = fn(*cargs, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        for i in outs:
            args[i][...] = ts[i].cpu().numpy()

    @staticmethod
    def _f(a, shape):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.shape == shape, (a.shape, shape)
        return a

    @staticmethod
    def _i(a, shape):
        a = np.ascontiguousarray(a, dtype=np.int32)
        assert a.shape == shape, (a.shape, shape)
        return a

    def reduce(self, v, idx, rv, rs):
        """v, idx [n, 64]; rv, rs [n, 28] -> per lane sum [n, 64], argmax value and index [n, 64], bdf_rms [n, 64]"""
        n = len(v)
        v, idx, rv, rs = self._f(v, (n, LANES)), self._i(idx, (n, LANES)), self._f(rv, (n, NX)), self._f(rs, (n, NX))
        s, av, ai, r = np.empty((n, LANES)), np.empty((n, LANES)), np.empty((n, LANES), dtype=np.int32), np.empty((n, LANES))
        self._run("reduce", [v, idx, rv, rs, n, s, av, ai, r], [5, 6, 7, 8])
        return s, av, ai, r

    def lu(self, J, c, b):
        """J [n, 28, 28], c [n], b [n, 28] -> ok [n], LU [n, 28, 28], piv [n, 28], perm [n, 28], x [n, 28]"""
        n = len(J)
        J, c, b = self._f(J, (n, NX, NX)), self._f(c, (n,)), self._f(b, (n, NX))
        ok, LU = np.full(n, -1, dtype=np.int32), np.empty((n, NX, NX))
        piv, perm, x = np.empty((n, NX), dtype=np.int32), np.empty((n, NX), dtype=np.int32), np.empty((n, NX))
        self._run("lu", [J, c, b, n, ok, LU, piv, perm, x], [4, 5, 6, 7, 8])
        return ok, LU, piv, perm, x

    def change_D(self, D, order, factor):
        n = len(D)
        D, order, factor = self._f(D, (n, NROWD, NX)), self._i(order, (n,)), self._f(factor, (n,))
        assert order.min() >= 1 and order.max() <= 5
        out = np.empty((n, NROWD, NX))
        self._run("change_D", [D, order, factor, n, out], [4])
        return out

    def step(self, pr):
        """pr: dict of kind, y0, A, g, mu, dt, rtol, atol, max_steps over n problems -> y [n, 28], stats [n, 5], rc [n]"""
        n = len(pr["kind"])
        kind, ms = self._i(pr["kind"], (n,)), self._i(pr["max_steps"], (n,))
        y0, A, g = self._f(pr["y0"], (n, NX)), self._f(pr["A"], (n, NX, NX)), self._f(pr["g"], (n, NX))
        mu, dt, rtol, atol = (self._f(pr[k], (n,)) for k in ("mu", "dt", "rtol", "atol"))
        y, st, rc = np.empty((n, NX)), np.empty((n, 5), dtype=np.int32), np.full(n, -1, dtype=np.int32)
        self._run("step", [kind, y0, A, g, mu, dt, rtol, atol, ms, n, y, st, rc], [10, 11, 12])
        return y, st, rc

    def model_jac(self, x, u, d, p, need_f0, f0=None):
        """x [n, 28], u [n, 6], d [n, >= 7], p [n, 208] -> f (eval1), f0 (the Jacobian's base point; read when not need_f0), J"""
        n = len(x)
        x, u, d, p = self._f(x, (n, NX)), self._f(u, (n, 6)), self._f(np.asarray(d)[:, :7], (n, 7)), self._f(p, (n, 208))
        f0 = np.zeros((n, NX)) if f0 is None else self._f(f0, (n, NX)).copy()
        f, J = np.empty((n, NX)), np.empty((n, NX, NX))
        self._run("model_jac", [x, u, d, _HostPtr(p), int(bool(need_f0)), n, f, f0, J], [6, 7, 8])
        return f, f0, J


def host_wave(build_dir):
    """The host twin, compiled by g++ into build_dir."""
    so = Path(build_dir) / "libbdfwave_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(so), str(WAVEDIR / "bdfwave_host.cpp")])
    return Wave(C.CDLL(str(so)), device=False)


def device_wave():
    """tests/bdfwave/libbdfwave.so, which __graft_entry__.build() compiles after the product."""
    so = WAVEDIR / "libbdfwave.so"
    if not so.exists():
        import __graft_entry__ as g
        g.build()
    import torch                                              # its HIP runtime has to be the first one the process loads (_lib.load)
    assert torch.cuda.is_available()
    return Wave(C.CDLL(str(so)), device=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# reductions
def butterfly_sum(v):
    """The xor-butterfly tree (32, 16, ... 1) over 64 lane values in double: one addition per lane and level, so NumPy's elementwise
    IEEE additions restate it exactly.  Returns the 64 lane results."""
    s = np.array(v, dtype=np.float64)
    lanes = np.arange(LANES)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[lanes ^ o]
    return s


def sum_cases():
    rng = np.random.default_rng(11)
    cases = {"random": rng.normal(size=LANES) * 10.0 ** rng.integers(-3, 4, LANES)}
    big = rng.normal(size=LANES // 2) * 10.0 ** rng.integers(0, 7, LANES // 2)    # cancelling: sum |v| / |sum v| of about 1e12
    canc = np.concatenate([big, -big])[rng.permutation(LANES)]
    canc[5] += 1e-5 * rng.uniform(1, 2)
    cases["cancelling"] = canc
    for k in (0, 27, 28, 63):
        one = np.zeros(LANES); one[k] = math.pi * 1e3
        cases[f"one_lane_{k}"] = one
    return cases


def check_sum(lanes_out, v, name=""):
    """every lane the same bits; those of the butterfly tree; within gamma_6 sum |v| of the exact sum (a tree of depth 6)"""
    assert np.all(lanes_out.view(np.int64) == lanes_out.view(np.int64)[0]), (name, "lanes differ")
    assert np.array_equal(lanes_out.view(np.int64), butterfly_sum(v).view(np.int64)), (name, "not the butterfly's bits")
    exact = math.fsum(v)
    err, bound = abs(LD(lanes_out[0]) - LD(exact)), gamma(6) * LD(math.fsum(np.abs(v))) + LD(abs(exact)) * LD(U_ROUND)
    assert err <= bound, (name, float(err), float(bound))
    return float(err), float(bound)


def argmax_cases():
    """name -> (values [64], indices [64], expected value, expected index)"""
    rng = np.random.default_rng(12)
    lanes = np.arange(LANES, dtype=np.int32)
    cases = {}
    for k in (0, 27, 63):
        v = rng.uniform(0, 1, LANES); v[k] = 2.0
        cases[f"alone_{k}"] = (v, lanes, 2.0, k)
    for o in (1, 2, 4, 8, 16, 32):                            # two equal maxima at every butterfly distance, both orientations
        for a in (0, 5, 21):
            b = a ^ o
            v = rng.uniform(0, 1, LANES); v[a] = v[b] = 1.5
            cases[f"tie2_{a}_{b}"] = (v, lanes, 1.5, min(a, b))
    for quad in ((3, 2, 35, 34), (63, 31, 47, 15), (9, 10, 12, 17), (60, 61, 62, 59), (1, 33, 17, 49)):
        v = rng.uniform(0, 1, LANES); v[list(quad)] = 1.25
        cases["tie4_" + "_".join(map(str, quad))] = (v, lanes, 1.25, min(quad))
    v = np.full(LANES, -1.0); v[40] = -0.0; v[7] = 0.0        # +0.0 == -0.0: the smaller index wins, whichever sign it carries
    cases["zeros_pos_first"] = (v, lanes, 0.0, 7)
    v = np.full(LANES, -1.0); v[40] = 0.0; v[7] = -0.0
    cases["zeros_neg_first"] = (v, lanes, 0.0, 7)
    cases["sentinel"] = (np.full(LANES, -1.0), np.full(LANES, NX, dtype=np.int32), -1.0, NX)
    # the integrator's own use: lanes >= 28 bring the sentinel, lanes < 28 a column of |a_ik| (rows below k bring -1, index kept)
    v = np.full(LANES, -1.0); i = np.full(LANES, NX, dtype=np.int32)
    v[:NX] = rng.uniform(0, 1, NX); i[:NX] = np.arange(NX); v[:9] = -1.0; v[13] = v[22] = 3.0
    cases["column_use"] = (v, i, 3.0, 13)
    return cases


def check_argmax(av, ai, v, idx, want_v, want_i, name=""):
    assert np.all(av.view(np.int64) == av.view(np.int64)[0]) and np.all(ai == ai[0]), (name, "lanes differ")
    assert av[0] == want_v == np.max(v), (name, av[0], want_v)
    assert ai[0] == want_i == int(np.min(np.asarray(idx)[np.asarray(v) == np.max(v)])), (name, int(ai[0]), want_i)
    src = [l for l in range(LANES) if idx[l] == want_i and v[l] == want_v][0]         # the value travels with its index (-0.0 / +0.0)
    assert av[:1].view(np.int64)[0] == np.asarray(v, dtype=np.float64)[src:src + 1].view(np.int64)[0], (name, "value not the index's")


def rms_cases():
    rng = np.random.default_rng(13)
    v = rng.normal(size=(4, NX)) * 10.0 ** rng.integers(-6, 3, (4, NX))
    s = 1e-6 + 1e-6 * np.abs(rng.normal(size=(4, NX)) * 10.0 ** rng.integers(-2, 4, (4, NX)))
    v[3] = 0.0
    return v, s


def check_rms(r_lanes, v, s, name=""):
    """sqrt(sum (v_i / s_i)^2 / 28): division, square, a sum of 28 terms in any order (at most 27 additions on a path), division by
    28 and the square root: a relative error of at most gamma_2 + gamma_27 + 2 u in the radicand, half of it after the root, plus the
    root's own rounding -- gamma_17 covers it."""
    assert np.all(r_lanes.view(np.int64) == r_lanes.view(np.int64)[0]), (name, "lanes differ")
    import mpmath as mp
    q = [Fraction(float(a)) / Fraction(float(b)) for a, b in zip(v, s)]
    ssq = sum(x * x for x in q) / NX
    with mp.workdps(40):
        exact = LD(mp.nstr(mp.sqrt(mp.mpf(ssq.numerator) / mp.mpf(ssq.denominator)), 25))
    err = abs(LD(r_lanes[0]) - exact)
    assert err <= gamma(17) * exact, (name, float(err), float(exact))
    return float(err), float(gamma(17) * exact)


# ---------------------------------------------------------------------------------------------------------------------------------
# LU on matrices whose arithmetic is exact
def _dyadic_ok(v, max_den=2 ** 20, max_abs=2 ** 30):
    v = Fraction(v)
    return (v.denominator & (v.denominator - 1)) == 0 and v.denominator <= max_den and abs(v) < max_abs


def exact_lu(A, b=None):
    """Gaussian elimination with partial pivoting (the first largest |entry| of the column from the diagonal down; whole rows swap)
    in rational arithmetic.  A: 28 x 28 of Fractions.  -> dict(ok, k_fail, piv, perm, LU (multipliers below the diagonal), x) and
    `exact`: whether every intermediate is a dyadic fraction with a bounded numerator and denominator, so that double arithmetic in
    any order of operations, fused or not, commits no rounding error."""
    n = len(A)
    M = [[Fraction(v) for v in row] for row in A]
    piv, perm, exact = [-1] * n, list(range(n)), all(_dyadic_ok(v) for row in M for v in row)
    for k in range(n):
        best, m = Fraction(-1), n
        for i in range(k, n):
            if abs(M[i][k]) > best:
                best, m = abs(M[i][k]), i
        if not best > 0:
            return dict(ok=False, k_fail=k, piv=piv, perm=None, LU=M, x=None, exact=exact)
        piv[k] = m
        M[k], M[m] = M[m], M[k]
        perm[k], perm[m] = perm[m], perm[k]
        for i in range(k + 1, n):
            M[i][k] = M[i][k] / M[k][k]
            exact &= _dyadic_ok(M[i][k])
            for j in range(k + 1, n):
                t = M[i][k] * M[k][j]
                M[i][j] -= t
                exact &= _dyadic_ok(t) and _dyadic_ok(M[i][j])
    x = None
    if b is not None:
        w = [Fraction(b[perm[i]]) for i in range(n)]
        exact &= all(_dyadic_ok(v) for v in w)
        for i in range(n):
            terms = [M[i][k] * w[k] for k in range(i)]
            exact &= all(_dyadic_ok(t) for t in terms) and _dyadic_ok(abs(w[i]) + sum(abs(t) for t in terms))
            w[i] -= sum(terms)
        for i in reversed(range(n)):
            terms = [M[i][j] * w[j] for j in range(i + 1, n)]
            exact &= all(_dyadic_ok(t) for t in terms) and _dyadic_ok(abs(w[i]) + sum(abs(t) for t in terms))
            w[i] = (w[i] - sum(terms)) / M[i][i]
            exact &= _dyadic_ok(w[i])
        x = w
    return dict(ok=True, k_fail=None, piv=piv, perm=perm, LU=M, x=x, exact=exact)


def _factors(rng, ties=()):
    """Unit lower L with multipliers in {0, +-1/4, +-1/2, +-3/4}, upper U with diagonal +-2, +-4 and small integers above it: every
    entry of every Schur complement of L U is a short sum of such products.  ties: (k, i, sign) sets the multiplier l_ik = sign."""
    L = [[Fraction(0)] * NX for _ in range(NX)]
    Um = [[Fraction(0)] * NX for _ in range(NX)]
    for i in range(NX):
        L[i][i] = Fraction(1)
        for k in range(i):
            if rng.random() < 0.5:
                L[i][k] = Fraction(int(rng.integers(1, 4)) * int(rng.choice([-1, 1])), 4)
        Um[i][i] = Fraction(int(rng.choice([2, 4])) * int(rng.choice([-1, 1])))
        for j in range(i + 1, NX):
            if rng.random() < 0.5:
                Um[i][j] = Fraction(int(rng.integers(-3, 4)))
    for k, i, sign in ties:
        L[i][k] = Fraction(sign)
    return L, Um


def _matmul(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(NX)) for j in range(NX)] for i in range(NX)]


def _rows(A, order):
    """row i of the result is row order[i] of A"""
    return [list(A[r]) for r in order]


def exact_lu_cases():
    """name -> dict(A (Fractions), b, expected from exact_lu, and what the case is there to show).  c = 1 and J = I - A on the way in."""
    rng = np.random.default_rng(21)
    x0 = [Fraction(int(v)) for v in rng.integers(-3, 4, NX)]
    ident = [[Fraction(int(i == j)) for j in range(NX)] for i in range(NX)]
    cases = {}

    def add(name, A, **note):
        b = [sum(A[i][j] * x0[j] for j in range(NX)) for i in range(NX)]
        ref = exact_lu(A, b)
        assert ref["exact"], name
        if ref["ok"]:
            assert ref["x"] == x0, name
        cases[name] = dict(A=A, b=b, ref=ref, **note)

    add("identity", ident)
    L, Um = _factors(rng)
    add("no_swap", _matmul(L, Um))
    assert cases["no_swap"]["ref"]["piv"] == list(range(NX))
    T = [[Fraction(int(i == j)) if j <= i else Fraction(int(rng.integers(-2, 3))) for j in range(NX)] for i in range(NX)]
    add("cycle", _rows(T, [(i - 1) % NX for i in range(NX)]))             # row i of T sits in row i + 1: every column but the last swaps
    assert cases["cycle"]["ref"]["piv"] == [min(k + 1, NX - 1) for k in range(NX)]
    L, Um = _factors(rng)
    order = list(range(NX)); order[0], order[27] = 27, 0
    add("pivot_row_27_at_0", _rows(_matmul(L, Um), order))
    assert cases["pivot_row_27_at_0"]["ref"]["piv"][0] == 27
    for k in (0, 13, 26):                                                 # |a_kk| equal to a later row's: k stays
        L, Um = _factors(rng, ties=[(k, k + 1 + (k % 2), 1)])
        add(f"tie_keeps_k_{k}", _matmul(L, Um), tie=(k, k))
        assert cases[f"tie_keeps_k_{k}"]["ref"]["piv"][k] == k
    for k, (r1, r2) in ((0, (9, 20)), (13, (14, 27)), (24, (25, 26))):    # two later rows tie above row k: the smaller index
        L, Um = _factors(rng, ties=[(k, r2, 1)])
        order = list(range(NX)); order[k], order[r1] = r1, k              # the pivot row of L U goes to r1, its equal stays at r2
        add(f"tie_later_rows_{k}", _rows(_matmul(L, Um), order), tie=(k, r1))
        assert cases[f"tie_later_rows_{k}"]["ref"]["piv"][k] == r1
    L, Um = _factors(rng, ties=[(5, 17, -1)])                             # +a in row 5 against -a in row 17
    add("tie_plus_minus", _matmul(L, Um), tie=(5, 5))
    L, Um = _factors(rng, ties=[(26, 27, -1)])
    order = list(range(NX)); order[26], order[27] = 27, 26                # -a first (the last two rows: the factors stay dyadic)
    add("tie_minus_plus", _rows(_matmul(L, Um), order), tie=(26, 26))
    assert cases["tie_plus_minus"]["ref"]["piv"][5] == 5 and cases["tie_minus_plus"]["ref"]["piv"][26] == 26
    for k in (0, 13, 27):                                                 # the column is exactly zero from the diagonal down at step k
        L, Um = _factors(rng)
        Um[k][k] = Fraction(0)
        add(f"singular_{k}", _matmul(L, Um), singular=k)
        assert not cases[f"singular_{k}"]["ref"]["ok"] and cases[f"singular_{k}"]["ref"]["k_fail"] == k
    return cases


def frac_to_float(M):
    a = np.array([[float(v) for v in row] for row in M])
    assert all(Fraction(float(v)) == v for row in M for v in row)
    return a


def lu_inputs(A_float):
    """c = 1, J = I - A: the code's I - c J is A again (exact whenever 1 - a and 1 - (1 - a) are, as for the dyadic cases)"""
    J = np.eye(NX) - A_float
    return J


def check_exact_lu(case, ok, LU, piv, perm, x, name=""):
    """bit for bit against the rational reference: the flag, the pivots, the permutation, L and U, the solution"""
    ref = case["ref"]
    assert bool(ok) == ref["ok"], (name, "flag", int(ok))
    if not ref["ok"]:
        k = ref["k_fail"]
        assert list(piv[:k]) == ref["piv"][:k] and np.all(piv[k:] == -1), (name, "pivots before the singular column", list(piv))
        return
    assert list(piv) == ref["piv"], (name, "piv", list(piv), ref["piv"])
    assert list(perm) == ref["perm"], (name, "perm", list(perm), ref["perm"])
    want = frac_to_float(ref["LU"])
    bad = np.argwhere((LU != want) | (np.signbit(LU) != np.signbit(want)) & (want != 0))
    assert len(bad) == 0, (name, "LU", bad[:4].tolist())
    assert np.array_equal(x, np.array([float(v) for v in ref["x"]])), (name, "solution")


def nan_lu_cases():
    rng = np.random.default_rng(22)
    L, Um = _factors(rng)
    A = frac_to_float(_matmul(L, Um))
    one = A.copy(); one[11, 0] = np.nan
    col = A.copy(); col[:, 0] = np.nan
    late = A.copy(); late[20:, 20] = np.nan; late[:20, 20] = 1.0
    return {"one_nan_row_11": (one, 11), "nan_column_0": (col, None), "nan_from_diagonal_20": (late, None)}


def check_nan_lu(A, nan_row, ok, piv, name=""):
    """What the code defines: `a > best` is false for a NaN, so a row holding one is never the pivot; a column with nothing else from
    the diagonal down is singular.  One NaN row poisons its whole row of the trailing matrix, is left over as the last row and the
    factorisation ends there: false."""
    assert not ok, (name, "a factorisation through a NaN must not succeed")
    if nan_row is None:
        k = int(np.flatnonzero(np.isnan(A).any(axis=0))[0])
        assert np.all(piv[k:] == -1) and np.all(piv[:k] >= 0), (name, list(piv))
        return
    pos = nan_row
    for k in range(NX):
        if piv[k] < 0:
            assert pos == k == NX - 1, (name, "stopped at", k, "NaN row at", pos)
            break
        assert piv[k] != pos, (name, "NaN row chosen at", k)
        if pos == k:
            pos = int(piv[k])


# ---------------------------------------------------------------------------------------------------------------------------------
# LU on general matrices
def general_lu_matrices(model_J):
    """16 of (J, c): random dense, I - c J of model Jacobians (model_J [>= 3, 28, 28]) at c = 1, 30, 300, graded matrices of
    condition 1e8 and 1e12.  b random."""
    rng = np.random.default_rng(31)
    out = []
    for _ in range(4):
        out.append((f"dense_{len(out)}", rng.normal(size=(NX, NX)), float(rng.uniform(0.1, 10))))
    for r in range(3):
        for c in (1.0, 30.0, 300.0):
            if len(out) < 12:
                out.append((f"model_row{r}_c{c:g}", model_J[r], c))
    for cond in (1e8, 1e8, 1e12, 1e12):
        Q1, _ = np.linalg.qr(rng.normal(size=(NX, NX))); Q2, _ = np.linalg.qr(rng.normal(size=(NX, NX)))
        A = (Q1 * np.logspace(0, -math.log10(cond), NX)) @ Q2
        if len(out) % 2:                                      # every other one graded by rows and columns rather than by singular values
            g = np.logspace(0, -math.log10(cond) / 2, NX)
            A = g[:, None] * rng.normal(size=(NX, NX)) * g[None, :]
        out.append((f"graded_{cond:g}_{len(out)}", np.eye(NX) - A, 1.0))
    assert len(out) == 16
    b = rng.normal(size=(16, NX))
    return [o[0] for o in out], np.array([o[1] for o in out]), np.array([o[2] for o in out]), b


def check_general_lu(J, c, b, ok, LU, piv, perm, x, name=""):
    """Higham Thm 9.3 / 9.4, componentwise, valid for any order of the operations with or without fused multiply-add:
        |P A - L U| <= gamma_28 |L||U|,        |b - A x| <= gamma_84 P^T |L||U||x|
    for the A the code factorised.  That A is fl(I - c J), two roundings at most from the exact I - c J used here, so
    gamma_2 (|I| + |c J|) joins either bound (times |x| in the second).  And partial pivoting's own properties."""
    assert ok, name
    assert np.all(piv >= np.arange(NX)) and np.all(piv < NX), (name, "piv", list(piv))
    want = list(range(NX))
    for k in range(NX):
        want[k], want[piv[k]] = want[piv[k]], want[k]
    assert list(perm) == want, (name, "perm is not the composition of the swaps")
    L = np.tril(LU, -1).astype(LD) + np.eye(NX, dtype=LD)
    Uu = np.triu(LU).astype(LD)
    assert np.all(np.abs(np.tril(LU, -1)) <= 1.0), (name, "a multiplier above 1")
    A = np.eye(NX, dtype=LD) - LD(c) * J.astype(LD)
    form = gamma(2) * (np.eye(NX, dtype=LD) + abs(LD(c)) * np.abs(J).astype(LD))
    LaU = np.abs(L) @ np.abs(Uu)
    r1, b1 = np.abs(A[perm] - L @ Uu), gamma(NX) * LaU + form[perm]
    assert np.all(r1 <= b1), (name, "factorisation residual", float(np.max(r1 / np.where(b1 > 0, b1, gamma(1)))))
    xa = np.abs(x).astype(LD)
    PtLaU = np.empty_like(LaU); PtLaU[perm] = LaU
    r2, b2 = np.abs(b.astype(LD) - A @ x.astype(LD)), gamma(3 * NX) * (PtLaU @ xa) + form @ xa
    assert np.all(r2 <= b2), (name, "solve residual", float(np.max(r2 / np.where(b2 > 0, b2, gamma(1)))))
    return float(np.max(r1 / np.where(b1 > 0, b1, 1))), float(np.max(r2 / np.where(b2 > 0, b2, 1)))


# ---------------------------------------------------------------------------------------------------------------------------------
# bdf_change_D
def _R_exact(order, factor):
    f = Fraction(factor)
    R = [[Fraction(0)] * (order + 1) for _ in range(order + 1)]
    for j in range(order + 1):
        R[0][j] = Fraction(1)
        for i in range(1, order + 1):
            R[i][j] = R[i - 1][j] * (Fraction(i - 1) - f * j) / i if j >= 1 else Fraction(0)
    return R


def change_D_cases():
    """(D [n, 8, 28], order [n], factor [n]): every order with the factors of the integrator's call sites -- the floor 0.2, the
    halving 0.5, the cap 10, a safety x rate product and a landing ratio (dt - t) / h, the last two inexact doubles.  Rows above the
    order hold a sentinel."""
    rng = np.random.default_rng(41)
    t, h = 900.0 * 0.7312345678901234, 17.123456789012345
    factors = [0.2, 0.5, 10.0, 0.9 * 0.731, (900.0 - t) / h / 20.0]
    D, order, factor = [], [], []
    for o in range(1, 6):
        for f in factors:
            d = rng.normal(size=(NROWD, NX)) * 10.0 ** rng.integers(-4, 3, (NROWD, NX))
            d[o + 1:] = -7.25e77
            D.append(d); order.append(o); factor.append(f)
    return np.array(D), np.array(order, dtype=np.int32), np.array(factor)


def check_change_D(D, order, factor, out, name=""):
    """rows 0..order = (R(factor) R(1))^T D exactly, up to the componentwise gamma_m (|R||U|)^T |D|.  m counted from gl_bdf.hpp:
    an entry of R takes 4 roundings per level (factor * j, the difference, the product, the division), `order` levels: 4 order;
    an entry of U = R(1) takes 2 per level (the integer factors are exact): 2 order; an entry of R U is a sum of order + 1 products:
    order + 1; a new difference is a sum of order + 1 products of those with D: order + 1.  m = 8 order + 2 (42 at order 5).
    Rows above the order keep every bit."""
    o = int(order)
    assert np.array_equal(out[o + 1:].view(np.int64), D[o + 1:].view(np.int64)), (name, "a row above the order moved")
    R, Uu = _R_exact(o, float(factor)), _R_exact(o, 1.0)
    RU = [[sum(R[i][k] * Uu[k][j] for k in range(o + 1)) for j in range(o + 1)] for i in range(o + 1)]
    aRU = [[sum(abs(R[i][k]) * abs(Uu[k][j]) for k in range(o + 1)) for j in range(o + 1)] for i in range(o + 1)]
    g, worst = gamma(8 * o + 2), 0.0
    for col in range(NX):
        d = [Fraction(float(D[k, col])) for k in range(o + 1)]
        for i in range(o + 1):
            exact = sum(RU[k][i] * d[k] for k in range(o + 1))
            bound = g * LD(float(sum(aRU[k][i] * abs(d[k]) for k in range(o + 1))))
            err = LD(abs(float(Fraction(float(out[i, col])) - exact)))
            assert err <= bound, (name, "row", i, "state", col, float(err), float(bound))
            if bound > 0:
                worst = max(worst, float(err / bound))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# bdf_step on systems with a closed-form solution
RATES = np.logspace(-5, math.log10(15.0), NX)                 # the model's range of decay rates [1/s]
TOLS = (1e-6, 1e-8)


def _blocks_solution(blocks, z0, h, dt):
    """z' = B z + h for block-diagonal B in extended precision: a 1 x 1 block lam (z = e^{lam t} z0 + h (e^{lam t} - 1) / lam, h t at
    lam = 0) or a 2 x 2 block [[-a, b], [-b, -a]] (w = z1 + i z2 obeys w' = (-a - i b) w + h1 + i h2)."""
    z, i, dt = np.zeros(NX, dtype=LD), 0, LD(dt)
    for blk in blocks:
        if np.isscalar(blk):
            lam = LD(blk)
            z[i] = z0[i] + h[i] * dt if lam == 0 else np.exp(lam * dt) * z0[i] + h[i] * np.expm1(lam * dt) / lam
            i += 1
        else:
            a, bb = LD(blk[0]), LD(blk[1])
            lam = np.clongdouble(complex(0)) + (-a) + np.clongdouble(1j) * (-bb)
            w0, hh = z0[i] + np.clongdouble(1j) * z0[i + 1], h[i] + np.clongdouble(1j) * h[i + 1]
            e = np.exp(lam * dt)
            w = e * w0 + hh * (e - 1) / lam
            z[i], z[i + 1] = w.real, w.imag
            i += 2
    assert i == NX
    return z


def _blocks_matrix(blocks):
    B, i = np.zeros((NX, NX)), 0
    for blk in blocks:
        if np.isscalar(blk):
            B[i, i] = blk; i += 1
        else:
            a, bb = blk
            B[i:i + 2, i:i + 2] = [[-a, bb], [-bb, -a]]; i += 2
    return B


def _orthogonal_system(rng, blocks, Q, dt, y0=None, zero_g=False):
    """A = Q B Q^T, g = -A ys for a steady state ys of order one; the truth through z = Q^T y in extended precision"""
    B = _blocks_matrix(blocks)
    A = Q @ B @ Q.T if Q is not None else B
    y0 = rng.uniform(0.5, 2.0, NX) if y0 is None else y0
    g = np.zeros(NX) if zero_g else -A @ rng.uniform(0.5, 2.0, NX)
    Ql = np.eye(NX, dtype=LD) if Q is None else Q.astype(LD)
    z = _blocks_solution(blocks, Ql.T @ y0.astype(LD), Ql.T @ g.astype(LD), dt)
    return A, g, y0, (Ql @ z)


def _triangular_truth(M, y0, g, dt):
    """y' = M y + g, M upper triangular with distinct diagonal: eigenvectors by back substitution in mpmath (50 digits)"""
    import mpmath as mp
    with mp.workdps(50):
        n = NX
        lam = [mp.mpf(float(M[i, i])) for i in range(n)]
        V = [[mp.mpf(0)] * n for _ in range(n)]               # column k: eigenvector of lam_k, v_kk = 1
        for k in range(n):
            V[k][k] = mp.mpf(1)
            for i in reversed(range(k)):
                s = mp.fsum(mp.mpf(float(M[i, j])) * V[j][k] for j in range(i + 1, k + 1))
                V[i][k] = s / (lam[k] - lam[i])

        def solve(rhs):                                       # V c = rhs, V unit upper triangular
            c = [mp.mpf(0)] * n
            for i in reversed(range(n)):
                c[i] = mp.mpf(float(rhs[i])) - mp.fsum(V[i][j] * c[j] for j in range(i + 1, n))
            return c
        c0, h = solve(y0), solve(g)
        z = [mp.exp(lam[k] * dt) * c0[k] + h[k] * mp.expm1(lam[k] * dt) / lam[k] for k in range(n)]
        return np.array([LD(mp.nstr(mp.fsum(V[i][k] * z[k] for k in range(n)), 25)) for i in range(n)])


FAMILIES = ("diagonal", "dense", "permuted_triangular", "complex_pairs", "f_zero", "y0_zero", "dt_1e-7", "pivoting_triangular")
# (family, variant): variant 0 of a family has the rates RATES, the others random rates in the same range.  scipy's BDF keeps its
# factorisation after a step that the error test rejected and gl_bdf.hpp factorises again at the new step size, so a system on which
# such a step occurs differs from scipy in `nlu` (and then sometimes in a step) by the algorithm, not by rounding.  Of the 34
# (system, tolerance) pairs below the host twin differs from scipy on one (permuted_triangular_3 at 1e-8, one factorisation
# more), which stays in as the witness; tests/test_bdf_wave_host.py asserts the twin's share.
STEP_SYSTEMS = (tuple(("diagonal", k) for k in range(4)) + (("dense", 0), ("dense", 1))
                + tuple(("permuted_triangular", k) for k in range(4))
                + (("pivoting_triangular", 0), ("pivoting_triangular", 1))
                + (("complex_pairs", 0), ("complex_pairs", 1), ("f_zero", 0), ("y0_zero", 0), ("dt_1e-7", 0)))


def make_system(family, k):
    """dict(A, g, y0, dt, truth [28] in extended precision) of one linear system y' = A y + g"""
    rng = np.random.default_rng([51, FAMILIES.index(family), k])
    rates = RATES if k == 0 else np.sort(10.0 ** rng.uniform(-5, math.log10(15.0), NX))
    dt = 900.0
    if family == "diagonal":
        A, g, y0, tr = _orthogonal_system(rng, [-r for r in rates], None, dt)
    elif family == "dense":                                   # A = Q Lam Q^T
        Q, _ = np.linalg.qr(rng.normal(size=(NX, NX)))
        A, g, y0, tr = _orthogonal_system(rng, [-r for r in rates], Q, dt)
    elif family in ("permuted_triangular", "pivoting_triangular"):
        # A = P (Lam + 0.01 T) P^T: the largest entry of a slow column of I - c A leaves the diagonal once c passes 100 or so, late
        # in the run.  A = P (Lam + 0.4 Lam T) P^T, rates descending: a fast row i couples into the slower column j with
        # 0.4 t_ij rate_i, larger than 1 / c + rate_j from the first steps on, so that every factorisation pivots, while the
        # eigenvectors (entries of order 0.4 t_ij) and the solution stay of order one.
        if family == "permuted_triangular":
            M = np.diag(-rates) + 0.01 * np.triu(rng.uniform(-1, 1, (NX, NX)), 1)
        else:
            rates = rates[::-1]
            M = np.diag(-rates) + 0.4 * rates[:, None] * np.triu(rng.uniform(-1, 1, (NX, NX)), 1)
        p = rng.permutation(NX)
        y0_, ys = rng.uniform(0.5, 2.0, NX), rng.uniform(0.5, 2.0, NX)
        g_ = -M @ ys
        tr_ = _triangular_truth(M, y0_, g_, dt)
        A = np.zeros((NX, NX)); A[np.ix_(p, p)] = M           # exactly P M P^T
        g, y0, tr = np.zeros(NX), np.zeros(NX), np.zeros(NX, dtype=LD)
        g[p], y0[p], tr[p] = g_, y0_, tr_
    elif family == "complex_pairs":                           # three damped pairs, |Im lam| dt <= 30, mixed by Q in variant 1
        pairs = [(float(rng.uniform(1e-3, 5e-3)), float(rng.uniform(5, 30)) / dt) for _ in range(3)]
        Q, _ = np.linalg.qr(rng.normal(size=(NX, NX)))
        A, g, y0, tr = _orthogonal_system(rng, pairs + [-r for r in rates[:NX - 6]], Q if k % 2 else None, dt)
    elif family == "f_zero":
        y0 = rng.uniform(0.5, 2.0, NX)
        A, g, tr = np.zeros((NX, NX)), np.zeros(NX), y0.astype(LD)
    elif family == "y0_zero":
        A, g, y0, tr = _orthogonal_system(rng, [-r for r in rates], None, dt, y0=np.zeros(NX))
    else:                                                     # the first step lands on dt
        dt = 1e-7
        A, g, y0, tr = _orthogonal_system(rng, [-r for r in rates], None, dt)
    return dict(A=np.ascontiguousarray(A), g=g, y0=y0, dt=dt, truth=tr)


@functools.lru_cache(maxsize=None)
def step_systems():
    return {f"{family}_{k}": make_system(family, k) for family, k in STEP_SYSTEMS}


def step_pairs():
    return [(name, tol) for name in step_systems() for tol in TOLS]


def _problem(kind=RHS_LINEAR, y0=None, A=None, g=None, mu=0.0, dt=900.0, tol=1e-6, max_steps=100000):
    return dict(kind=kind, y0=np.zeros(NX) if y0 is None else y0, A=np.zeros((NX, NX)) if A is None else A,
                g=np.zeros(NX) if g is None else g, mu=mu, dt=dt, rtol=tol, atol=tol, max_steps=max_steps)


def stack(problems):
    return {k: np.array([p[k] for p in problems]) for k in problems[0]}


def linear_problems():
    S = step_systems()
    return [_problem(y0=S[n]["y0"], A=S[n]["A"], g=S[n]["g"], dt=S[n]["dt"], tol=tol) for n, tol in step_pairs()]


VDP_Y0 = np.concatenate([[2.0, 0.0], np.linspace(0.5, 2.0, NX - 2)])


def vdp_problems():
    return [_problem(kind=RHS_VDP, y0=VDP_Y0, mu=1000.0, dt=900.0, tol=tol) for tol in TOLS]


SQUARE_Y0 = np.linspace(0.5, 2.0, NX)


def failure_problems():
    """name -> problem.  y' = y^2 from y0 in [0.5, 2] blows up at t = 1 / y0, the first state at t = 0.5."""
    return {
        "square_ok": _problem(kind=RHS_SQUARE, y0=SQUARE_Y0, dt=0.4, tol=1e-8),
        "square_blowup": _problem(kind=RHS_SQUARE, y0=SQUARE_Y0, dt=2.5, tol=1e-6),
        "square_step_limit": _problem(kind=RHS_SQUARE, y0=SQUARE_Y0, dt=2.5, tol=1e-6, max_steps=50),
        "square_nan_rhs": _problem(kind=RHS_SQUARE_NAN, y0=SQUARE_Y0, dt=2.5, tol=1e-6),
    }


def wrms(y, truth, tol):
    """the solver's own weighted RMS norm of y - truth, scale = atol + rtol |truth|"""
    e = (np.asarray(y, dtype=LD) - truth) / (LD(tol) + LD(tol) * np.abs(truth))
    return float(np.sqrt(np.mean(e * e)))


def _rhs_numpy(p):
    A, g, kind, mu = p["A"], p["g"], p["kind"], p["mu"]
    if kind == RHS_LINEAR:
        return lambda t, y: A @ y + g
    if kind == RHS_VDP:
        i = np.arange(NX)

        def f(t, y):
            k = -0.01 * i * y
            k[0], k[1] = y[1], mu * (1.0 - y[0] * y[0]) * y[1] - y[0]
            return k
        return f
    return lambda t, y: y * y


@functools.lru_cache(maxsize=None)
def scipy_reference():
    """scipy.integrate.solve_ivp(method="BDF") on every (system, tolerance) pair: y(dt), [steps, njev, nlu]"""
    from scipy.integrate import solve_ivp
    out = {}
    for (name, tol), p in zip(step_pairs(), linear_problems()):
        sol = solve_ivp(_rhs_numpy(p), (0.0, p["dt"]), p["y0"], method="BDF", rtol=tol, atol=tol)
        assert sol.status == 0, (name, tol)
        out[(name, tol)] = (sol.y[:, -1].copy(), np.array([len(sol.t) - 1, sol.njev, sol.nlu]))
    return out


@functools.lru_cache(maxsize=None)
def vdp_truth():
    """Van der Pol mu = 1000 from (2, 0) over 900 s by Radau at 1e-12; the decoupled states in closed form"""
    from scipy.integrate import solve_ivp
    p = vdp_problems()[0]
    sol = solve_ivp(lambda t, y: np.array([y[1], p["mu"] * (1.0 - y[0] * y[0]) * y[1] - y[0]]), (0.0, 900.0), VDP_Y0[:2], method="Radau",
                    rtol=1e-12, atol=1e-12)
    assert sol.status == 0
    tr = VDP_Y0.astype(LD) * np.exp(LD(-0.01) * np.arange(NX).astype(LD) * LD(900.0))
    tr[:2] = sol.y[:, -1]
    return tr


def check_steps(y, st, rc, y_twin=None, match=0.90, label=""):
    """The linear systems, in the order of step_pairs().  y_twin: the host twin's states; None when the twin itself is under test
    (its error is then held to scipy's alone, on the pairs where it took scipy's path).
    -> (share of pairs whose steps / Jacobians / factorisations equal scipy's, report lines)."""
    ref, twin = scipy_reference(), y_twin is not None
    y_twin = y if y_twin is None else y_twin
    S = step_systems()
    same, lines = [], []
    for k, (name, tol) in enumerate(step_pairs()):
        truth, (ys, ss) = S[name]["truth"], ref[(name, tol)]
        e, e_twin, e_sp = wrms(y[k], truth, tol), wrms(y_twin[k], truth, tol), wrms(ys, truth, tol)
        eq = bool(np.array_equal(st[k, [0, 2, 3]], ss))
        same.append(eq)
        lines.append(f"{label} {name} tol {tol:g}: rc {rc[k]} error {e:.3e} twin {e_twin:.3e} scipy {e_sp:.3e} | steps/njev/nlu "
                     f"{st[k, 0]}/{st[k, 2]}/{st[k, 3]} scipy {ss[0]}/{ss[1]}/{ss[2]} {'same' if eq else 'DIFFERENT'}")
        assert rc[k] == BDF_OK, lines[-1]
        # 1.25 x the larger of the twin's and scipy's error: the margin of test_same_algorithm_as_the_cpu_port
        assert e <= 1.25 * (max(e_twin, e_sp) if twin else e_sp) or not (twin or eq), lines[-1]
        if eq:                                                # compare()'s same_tol on the pairs that took the reference's path
            sc = np.maximum(np.abs(y_twin[k]), 1e-3 * np.abs(y_twin[k]).max())
            d = float(np.max(np.abs(y[k] - y_twin[k]) / np.where(sc == 0.0, 1.0, sc)))
            assert d <= 1e-8, (lines[-1], "state against the twin", d)
    share = float(np.mean(same))
    lines.append(f"{label} statistics equal to scipy's on {sum(same)} of {len(same)} pairs ({share:.3f})")
    assert share >= match, lines[-1]
    return share, lines


# ---------------------------------------------------------------------------------------------------------------------------------
# the model's right-hand side through eval1 and jac
def model_rows(golden):
    """16 rows (x, u, d, p): 8 each of step_tight and step_tight_storm"""
    p0 = np.load(ROOT / "tests" / "golden" / "params_default.npz")["p"].astype(np.float64)
    X, U, D, P = [], [], [], []
    for name in ("step_tight", "step_tight_storm"):
        g = golden(name)
        n = len(g["X"])
        rows = np.linspace(0, n - 1, 8).astype(int)
        X.append(g["X"][rows]); U.append(g["U"][rows]); D.append(g["D"][rows][:, :7])
        P.append(g["P"][rows].astype(np.float64) if "P" in g.files else np.repeat(p0[None], 8, axis=0))
    return tuple(np.concatenate(v) for v in (X, U, D, P))


def rhs_scale(golden):
    """the scale of test_rhs_matches_reference_text_vectors: the column maximum of |DX| over the reference's vectors"""
    return np.maximum(np.abs(golden("rhs_kat")["DX"]).max(axis=0), 1e-30)


def check_model_jac(x, sc, f, f0, J, f_ref, J_ref, name=""):
    """f (eval1, lane 0) and f0 (the need_f0 path, lane 28) against the reference right-hand side within 1e-11 sc (the bound the suite
    holds the device right-hand side to); J within 2 x 1e-11 sc_i / dx_j: either side of the difference quotient may be off by
    1e-11 sc_i, the increment dx_j = sqrt(eps) max(|x_j|, 1) is the same double on both sides."""
    dx = 1.4901161193847656e-8 * np.maximum(np.abs(x), 1.0)
    e_f, e_f0 = np.max(np.abs(f - f_ref) / sc), np.max(np.abs(f0 - f_ref) / sc)
    e_J = np.max(np.abs(J - J_ref) / (sc[None, :, None] / dx[:, None, :]))
    assert e_f <= 1e-11 and e_f0 <= 1e-11, (name, float(e_f), float(e_f0))
    assert e_J <= 2e-11, (name, float(e_J))
    return float(e_f), float(e_f0), float(e_J)
