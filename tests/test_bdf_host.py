"""CPU tests of the BDF integrator of glgym_evalF (GLGYM_INTEGRATOR_BDF, ABI 7): the binding agrees with the header and the library,
GreenLight validates its integrator arguments without a device, and the host instantiation of csrc/gl_bdf.hpp (a team of one lane,
tests/bdfhost/bdfhost.cpp) takes the same decisions as the oracle's gl_oracle_bdf and lands on the same state."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from gl_gym_amd import _lib
    if not _lib.LIB_PATH.exists():
        g.build()
    return _lib


def test_integrator_abi_is_declared_bound_and_versioned(lib):
    hdr = (ROOT / "include" / "glgym.h").read_text()
    for name in ("glgym_set_integrator", "glgym_set_tolerances", "glgym_get_solver_stats"):
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in lib.PROTOTYPES
    L = lib.load()
    for name in ("glgym_set_integrator", "glgym_set_tolerances", "glgym_get_solver_stats"):
        assert getattr(L, name).argtypes == lib.PROTOTYPES[name][1]
    enum = dict((k.lower(), int(v)) for k, v in re.findall(r"GLGYM_INTEGRATOR_([A-Z]+) = (\d+)", hdr))
    assert enum == lib.INTEGRATORS == {"explicit": 0, "bdf": 1}
    assert int(re.search(r"#define GLGYM_NSOLVER_STAT (\d+)", hdr).group(1)) == lib.NSOLVER_STAT == len(lib.SOLVER_STAT_KEYS)
    assert lib.ABI_VERSION == 7 == L.glgym_abi_version()
    assert b"ABI 7" in L.glgym_version()
    # a null handle is refused by every new entry point (no device needed)
    assert L.glgym_set_integrator(None, 1) == lib.EINVAL
    assert L.glgym_set_tolerances(None, 1e-6, 1e-6, 10) == lib.EINVAL
    st = (C.c_int32 * 5)()
    assert L.glgym_get_solver_stats(None, 1, st) == lib.EINVAL


@pytest.mark.parametrize("kw", [dict(integrator="rk45"), dict(integrator="bdf", rtol=0.0), dict(integrator="bdf", atol=-1e-6),
                                dict(rtol=float("nan")), dict(integrator="bdf", max_steps=0), dict(max_steps=2.5),
                                dict(integrator="bdf", variant="ode_pipe")])
def test_greenlight_validates_integrator_arguments_before_the_device(lib, kw):
    from gl_gym_amd import GreenLight
    nd = 14 if kw.get("variant") == "ode_pipe" else 10
    with pytest.raises(ValueError):
        GreenLight(28, 6, nd, 208, 900.0, **kw)


@pytest.fixture(scope="module")
def bdfhost(tmp_path_factory):
    so = tmp_path_factory.mktemp("bdfhost") / "libbdfhost.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", "-o", str(so),
                           str(ROOT / "tests" / "bdfhost" / "bdfhost.cpp")])
    L = C.CDLL(str(so))
    dp = C.POINTER(C.c_double)
    L.bdfhost_step.argtypes = [dp] * 4 + [C.c_double] * 3 + [C.c_int, dp, C.POINTER(C.c_int)]

    def step(x, u, d, p, tol, max_steps=10000):
        x, u, d, p = [np.ascontiguousarray(v, dtype=np.float64) for v in (x, u, d, p)]
        out, st = np.empty(28), np.zeros(5, dtype=np.int32)
        rc = L.bdfhost_step(*(v.ctypes.data_as(dp) for v in (x, u, d, p)), 900.0, tol, tol, max_steps, out.ctypes.data_as(dp),
                            st.ctypes.data_as(C.POINTER(C.c_int)))
        return rc, out, st
    return step


def _against_oracle(bdfhost, oracle, X, U, D, P, tol):
    H, R, same = [], [], []
    for i in range(len(X)):
        rc, xh, sh = bdfhost(X[i], U[i], D[i], P[i], tol)
        xo, nfev, so = oracle.bdf(X[i], U[i], D[i], P[i], 900.0, tol, tol)
        assert rc == 0
        H.append(xh); R.append(xo)
        same.append(np.array_equal(sh, [so[0], nfev, so[1], so[2], so[3]]))
    return np.array(H), np.array(R), np.array(same)


@pytest.mark.parametrize("tol,bound", [(1e-6, 5e-5), (1e-8, 5e-7)])
@pytest.mark.parametrize("fixture", ["step_tight", "holdout_gl2010_random"])
def test_host_instantiation_takes_the_oracles_decisions(bdfhost, oracle, golden, fixture, tol, bound):
    g = golden(fixture)
    if fixture == "step_tight":
        X, U, D, P = g["X"], g["U"], g["D"], g["P"]
    else:
        n = 200                                               # one-step maps from the fixture's trajectory states, W row k with U row k
        X, U, D = g["X"][:n], g["U"][:n], g["weather"][:n]
        P = np.repeat(np.load(ROOT / "tests" / "golden" / "params_default.npz")["p"][None], n, axis=0)
    H, R, same = _against_oracle(bdfhost, oracle, X, U, D, P, tol)
    print(f"{fixture} tol {tol:g}: stats identical on {same.mean():.3f} of {len(X)} rows, "
          f"difference on those {oracle.scaled_rel_err(H[same], R[same]):.2e}, on all {oracle.scaled_rel_err(H, R):.2e}")
    assert same.mean() >= 0.95
    assert oracle.scaled_rel_err(H[same], R[same]) <= 1e-9
    assert oracle.scaled_rel_err(H, R) <= bound


def test_host_instantiation_step_limit_fails_the_row(bdfhost, golden):
    g = golden("step_tight")
    rc, _, st = bdfhost(g["X"][0], g["U"][0], g["D"][0], g["P"][0], 1e-6, max_steps=5)
    assert rc != 0 and st[0] == 5
