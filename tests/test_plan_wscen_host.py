"""CPU tests of the weather-forecast scenarios' scalar logic: csrc/gl_wscen.hpp (host instantiation, tests/wscenhost/wscenhost.cpp -- a
lane is a call, a grid a loop over the lanes) against a NumPy restatement written from include/glgym.h glgym_plan_weather.

Bounds.
* Windows and child offsets: EXACT (uint32 / uint64 views).  Every operation of the definition is a correctly rounded double operation or
  one rounding to T, and NumPy performs the same ones in the same order.
* Moments of x = e / sigma over N = 4 480 (ps, j) streams at lead h = 40 with phi = 0.8.  x_h = sum_k w_k eps_{h-k}, w_k = sqrt(1 - phi^2)
  phi^k: mean 0, variance V = 1 - phi^(2h).  eps is four centred uniforms scaled to unit variance, excess kurtosis -1.2 / 4 = -0.3; a
  weighted sum of independent terms has excess kurtosis kappa = -0.3 sum w^4 / (sum w^2)^2 = -0.3 (1 - phi^2) / (1 + phi^2) = -0.066 (the
  finite-h correction is of relative size phi^80).  So: |mean| <= 5 sqrt(V / N); |var - V| <= 5 sqrt((2 + kappa) V^2 / N); the sample
  lag-1 correlation of (x_39, x_40) across streams within 5 (1 - phi^2) / sqrt(N) of phi (the normal-theory standard error of a
  correlation coefficient; x is a sum of many bounded terms with |kappa| < 0.07).  The generator is deterministic and MOMENT_SEED was
  picked once so that the NumPy restatement itself passes."""
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
SRC = ROOT / "tests" / "wscenhost" / "wscenhost.cpp"
KEY_TAG = 0x5753434E
M32 = 0xFFFFFFFF
NCOL = 7
ADDITIVE = (1, 5, 6)
SQRT3 = 1.7320508075688772
MOMENT_SEED = 2026
SEED, DRAW = 0xDEADBEEF12345678, (7 << 32) | 41                # both with a nonzero high word
SIGMA = [0.2, 1.5, 0.1, 0.0, 0.3, 2.0, 0.0]                    # moderate; co2Out and tSoOut left alone
SHAPES = [(2, 5, 3), (3, 4, 7), (1, 1, 1)]                     # (P, S, H)


def build_host(path):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.wscenhost_sizeof.argtypes, lib.wscenhost_sizeof.restype = [], C.c_int
    lib.wscenhost_window.argtypes = ([C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_uint64, C.c_uint64,
                                                      C.c_void_p, C.c_void_p])
    lib.wscenhost_window.restype = None
    lib.wscenhost_error.argtypes = [C.c_uint32, C.c_int, C.c_int, C.c_double, C.c_double, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.wscenhost_error.restype = None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_wscen.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    return build_host(tmp_path_factory.mktemp("wscenhost") / "libwscenhost.so")


def ptr(a):
    return None if a is None else a.ctypes.data


# ---- restatement (from the header's text, not from gl_wscen.hpp) ----------------------------------------------------------------
def np_wscen_eps(n_ps, h, seed, D):
    """eps of every (ps, column j) at horizon step h: [n_ps, 7] float64."""
    ps = np.arange(n_ps, dtype=np.uint64)[:, None]
    j = np.arange(NCOL, dtype=np.uint64)[None, :]
    ps, ctr = np.broadcast_arrays(ps, np.uint64(8 * h) + j)
    r = np_philox(ps, D & M32, D >> 32, ctr, seed & M32, (seed >> 32) ^ KEY_TAG)            # [n_ps, 7, 4]
    c = (r.astype(np.float64) + 0.5) * 2.0 ** -32 - 0.5
    return (((c[..., 0] + c[..., 1]) + c[..., 2]) + c[..., 3]) * np.float64(SQRT3)


def np_wscen_errors(n_ps, H, sigma, phi, seed, D):
    """e [H, n_ps, 7] float64: e_0 = 0, e_h = phi*e_{h-1} + g*eps_h with g = sqrt(1 - phi*phi) * sigma."""
    phi = np.float64(phi)
    g = np.sqrt(np.float64(1.0) - phi * phi) * np.asarray(sigma, dtype=np.float64)
    e = np.zeros((H, n_ps, NCOL))
    for h in range(1, H):
        e[h] = phi * e[h - 1] + g[None, :] * np_wscen_eps(n_ps, h, seed, D)
    return e


def np_wscen(P, K, S, H, weather, w_off, ts, sigma, phi, seed, D):
    """-> (window [P*S*H, nd] of weather's dtype, w_off_child [P*K*S] int32)."""
    rows, nd = weather.shape
    T = weather.dtype
    e = np_wscen_errors(P * S, H, sigma, phi, seed, D)
    out = np.empty((P * S * H, nd), T)
    for ps in range(P * S):
        p = ps // S
        for h in range(H):
            src = weather[min(max(int(w_off[p]) + int(ts[p]) + h, 0), rows - 1)]
            row = src.copy()
            for j in range(NCOL):
                w = np.float64(src[j])
                if j in ADDITIVE:
                    row[j] = T.type(w + e[h, ps, j])
                else:
                    t = e[h, ps, j] * w
                    v0 = w + t
                    row[j] = T.type(0.0 if v0 < 0 else v0)
            out[ps * H + h] = row
    child = np.empty(P * K * S, np.int32)
    for c in range(P * K * S):
        p, s = c // (K * S), c % S
        child[c] = (p * S + s) * H - int(ts[p])
    return out, child


def table(dtype, rows=40, nd=10, seed=5):
    """A small weather table: iGlob zero at 'night' rows, temperatures of either sign, the rest positive."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 20.0, (rows, nd))
    w[:, 0] = np.where(np.arange(rows) % 4 < 2, 0.0, rng.uniform(50, 800, rows))
    w[:, 1] = rng.uniform(-8, 25, rows)
    w[:, 5] = w[:, 1] - rng.uniform(5, 20, rows)
    w[:, 3] = 7.3e-4
    return np.ascontiguousarray(w.astype(dtype))


def parents(P, rows, H):
    """w_off / timestep per parent; the last parent's source rows run past the end of the table (the clamp)."""
    w_off = np.arange(P, dtype=np.int32) * 3
    ts = np.arange(P, dtype=np.int32) + 2
    ts[-1] = rows - 1 - w_off[-1] - (H // 2)                   # rows-1-H//2, .., rows-1, rows-1, ...
    return w_off, ts


def run_window(host, P, K, S, H, weather, w_off, ts, sigma, phi, seed, D, offsets=True, pad=3):
    nd = weather.shape[1]
    out = np.full((P * S * H + pad, nd), -7, weather.dtype)
    child = np.full(P * K * S + pad, -7, np.int32) if offsets else None
    sg = np.asarray(sigma, dtype=np.float64)
    host.wscenhost_window(int(weather.dtype == np.float64), P, K, S, H, nd, ptr(weather), weather.shape[0], ptr(w_off), ptr(ts), ptr(sg), phi,
                          seed, D, ptr(out), ptr(child))
    return out, child


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def moment_checks(x39, x40, phi, h):
    """The five-standard-error checks of the module docstring on x = e / sigma over N streams; -> (|mean|, |var - V|, |corr - phi|)."""
    N = x40.size
    V = 1.0 - phi ** (2 * h)
    kappa = -0.3 * (1 - phi * phi) / (1 + phi * phi)
    corr = (x39 * x40).sum() / np.sqrt((x39 * x39).sum() * (x40 * x40).sum())
    worst = abs(x40.mean()), abs(x40.var() - V), abs(corr - phi)
    assert worst[0] <= 5 * np.sqrt(V / N), worst
    assert worst[1] <= 5 * np.sqrt((2 + kappa) * V * V / N), worst
    assert worst[2] <= 5 * (1 - phi * phi) / np.sqrt(N), worst
    return worst


# ---- tests -------------------------------------------------------------------------------------------------------------------
def test_args_struct_has_the_headers_size(host):
    from gl_gym_amd import _lib as L
    assert C.sizeof(L.PlanWeatherArgs) == host.wscenhost_sizeof()
    assert L.PlanWeatherArgs._fields_[0][0] == "struct_size"
    hdr = (ROOT / "include" / "glgym.h").read_text()
    assert "glgym_plan_weather" in L.PROTOTYPES and re.search(r"\bint glgym_plan_weather\s*\(", hdr)
    assert L.ABI_VERSION == 7 == int(re.search(r"#define GLGYM_ABI_VERSION (\d+)", hdr).group(1))
    assert L.WEATHER_COLUMNS == ("iGlob", "tOut", "vpOut", "co2Out", "wind", "tSky", "tSoOut")


def test_vectorised_words_are_the_scalar_definition():
    h, ps, j = 2, 7, 4
    r = philox4x32_10([ps, DRAW & M32, DRAW >> 32, 8 * h + j], [SEED & M32, (SEED >> 32) ^ KEY_TAG])
    c = [(float(v) + 0.5) * 2.0 ** -32 - 0.5 for v in r]
    assert np_wscen_eps(10, h, SEED, DRAW)[ps, j] == (((c[0] + c[1]) + c[2]) + c[3]) * SQRT3
    # apart from the crop-scenario stream (its tag, its counter layout) and the untagged key
    assert philox4x32_10([ps, DRAW & M32, DRAW >> 32, 8 * h + j], [SEED & M32, (SEED >> 32) ^ 0x5343454E]) != r
    assert philox4x32_10([ps, DRAW & M32, DRAW >> 32, 8 * h + j], [SEED & M32, SEED >> 32]) != r


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("P,S,H", SHAPES)
def test_windows_are_exact(host, P, S, H, phi, dtype):
    K = 3
    weather = table(dtype)
    rows, nd = weather.shape
    w_off, ts = parents(P, rows, H)
    got, child = run_window(host, P, K, S, H, weather, w_off, ts, SIGMA, phi, SEED, DRAW)
    exp, exp_child = np_wscen(P, K, S, H, weather, w_off, ts, SIGMA, phi, SEED, DRAW)
    n = P * S * H
    assert same_bits(got[:n], exp), np.abs(got[:n].astype(np.float64) - exp).max()
    assert (got[n:] == -7).all() and (child[P * K * S:] == -7).all()      # nothing past the end
    assert np.array_equal(child[:P * K * S], exp_child)
    # ---- properties
    win = got[:n].reshape(P, S, H, nd)
    src_rows = np.clip((w_off + ts)[:, None] + np.arange(H)[None, :], 0, rows - 1)          # [P, H]
    src = weather[src_rows]                                                                # [P, H, nd]
    if H >= 3:
        assert (w_off + ts)[-1] + H - 1 > rows - 1 == src_rows[-1].max()       # the last parent runs into the clamp
    for s in range(S):
        assert same_bits(win[:, s, 0], src[:, 0])                         # h = 0: a measurement
        for j in [j for j in range(NCOL) if SIGMA[j] == 0] + list(range(NCOL, nd)):
            assert same_bits(win[:, s, :, j], src[:, :, j]), j            # sigma_j = 0, and the columns past the seventh
    for j in (0, 2, 3, 4):
        assert (win[..., j] >= 0).all()
    assert (win[..., 0][np.broadcast_to(src[:, None, :, 0] == 0, win[..., 0].shape)] == 0).all()
    assert P == 1 or (src[..., 0] == 0).any()                              # iGlob at night is among the source rows
    if H > 1 and S > 1:
        assert not same_bits(win[:, 0, 1:, 1], win[:, 1, 1:, 1])           # the scenarios differ
    # the window does not depend on K, and every child's unchanged timestep indexes its own window
    got1, child1 = run_window(host, P, 1, S, H, weather, w_off, ts, SIGMA, phi, SEED, DRAW)
    assert same_bits(got1[:n], got[:n])
    ch = child[:P * K * S].reshape(P, K, S)
    assert (ch == ch[:, :1]).all() and np.array_equal(ch[:, 0].reshape(-1), child1[:P * S])
    for h in range(H):
        assert np.array_equal(ch.astype(np.int64) + ts[:, None, None] + h, np.broadcast_to((np.arange(P * S).reshape(P, 1, S) * H + h), ch.shape))
    # without the offsets only the window is written; another draw, another seed: other futures
    got2, none = run_window(host, P, K, S, H, weather, w_off, ts, SIGMA, phi, SEED, DRAW, offsets=False)
    assert none is None and same_bits(got2, got)
    if H > 1:
        assert not same_bits(run_window(host, P, K, S, H, weather, w_off, ts, SIGMA, phi, SEED, DRAW + 1)[0], got)
        assert not same_bits(run_window(host, P, K, S, H, weather, w_off, ts, SIGMA, phi, SEED + 1, DRAW)[0], got)


def test_zero_sigmas_give_the_source_rows(host):
    P, K, S, H = 2, 2, 3, 5
    weather = table(np.float32, nd=14)                                     # the measured-pipe variant's column count
    w_off, ts = parents(P, weather.shape[0], H)
    got, _ = run_window(host, P, K, S, H, weather, w_off, ts, [0.0] * 7, 0.7, SEED, DRAW)
    src = weather[np.clip((w_off + ts)[:, None] + np.arange(H)[None, :], 0, weather.shape[0] - 1)]
    assert same_bits(got[:P * S * H].reshape(P, S, H, 14), np.broadcast_to(src[:, None], (P, S, H, 14)).copy())


def test_moments_of_the_error_process(host):
    n_ps, H, phi = 640, 41, 0.8                                            # 4 480 (ps, j) streams, lead h = 40
    e = np_wscen_errors(n_ps, H, [1.0] * 7, phi, MOMENT_SEED, 0)
    w_ref = moment_checks(e[39].reshape(-1), e[40].reshape(-1), phi, 40)   # the seed's own NumPy restatement passes
    got = np.empty((n_ps, NCOL, H))
    for ps in range(n_ps):
        for j in range(NCOL):
            host.wscenhost_error(ps, j, H, 1.0, phi, MOMENT_SEED, 0, got[ps, j].ctypes.data)
    assert same_bits(got.transpose(2, 0, 1), e)
    w = moment_checks(got[:, :, 39].reshape(-1), got[:, :, 40].reshape(-1), phi, 40)
    N = n_ps * NCOL
    print(f"moments of e / sigma at h = 40, phi = 0.8 over N = {N} streams (seed {MOMENT_SEED}): |mean| {w[0]:.5f} (NumPy {w_ref[0]:.5f}, "
          f"bound {5 / np.sqrt(N):.5f}), |var - V| {w[1]:.5f} ({w_ref[1]:.5f}, {5 * np.sqrt(1.934 / N):.5f}), |corr - phi| {w[2]:.5f} "
          f"({w_ref[2]:.5f}, {5 * 0.36 / np.sqrt(N):.5f})")
    assert (got[:, :, 0] == 0).all() and np.abs(got).max() < 3.47 * 5.0    # |e| <= g |eps| / (1 - phi)


def test_entry_point_refuses_bad_arguments_without_a_device():
    """Every check happens before the handle is looked at: with good arguments and no handle the refusal names the handle, with a bad
    argument it names the argument list.  The output pointers are never followed: nothing is launched."""
    import __graft_entry__ as g
    from gl_gym_amd import _lib as L
    if not L.LIB_PATH.exists():
        g.build()
    lib = L.load()
    window, child = np.full(64, -7.0), np.full(64, -7, np.int32)
    P_ = 0x1000                                                            # a non-null pointer: never followed

    def args(**kw):
        a = L.make_plan_args(L.PlanWeatherArgs, 2, 3, 5, 4, 100, P_, P_, P_, (C.c_double * 7)(*SIGMA), 0.7, SEED, DRAW, None, window.ctypes.data,
                             child.ctypes.data)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def refused(a, null_handle):
        assert lib.glgym_plan_weather(None, C.byref(a), None) == L.EINVAL
        assert b"glgym_plan_weather" in lib.glgym_last_error()
        return (b"null handle" in lib.glgym_last_error()) == null_handle

    assert refused(args(), True)
    assert refused(args(w_off_child=None, draw_base=P_), True)             # the optional members
    for field, value in (("struct_size", 8), ("struct_size", C.sizeof(L.PlanWeatherArgs) + 8), ("S", 257), ("S", 0), ("H", 65537), ("H", 0),
                         ("P", 0), ("K", 0), ("phi", 1.0), ("phi", -0.1), ("phi", float("nan")), ("weather_rows", 0), ("weather", None),
                         ("w_off_parent", None), ("timestep_parent", None), ("window", None)):
        assert refused(args(**{field: value}), False), (field, value)
    for j, bad in ((0, -0.1), (3, float("nan")), (6, float("inf"))):
        a = args()
        a.sigma[j] = bad
        assert refused(a, False), (j, bad)
    assert refused(args(P=2 ** 20, S=256, H=65536), False)                 # P*S*H past INT32_MAX
    assert refused(args(P=2 ** 15, S=256, H=256), False)                   # = 2^31
    assert refused(args(P=2 ** 10, K=2 ** 15, S=64, H=1), False)           # P*K*S = 2^31
    assert refused(args(P=2 ** 15 - 1, S=256, H=256), True)                # just below
    assert (window == -7).all() and (child == -7).all()


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """tests/wscenhost/wscenhost.cpp with its own main, AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (nothing is
    loaded into Python): exactly sized heap buffers at the awkward shapes, so an index past a row end is reported."""
    exe = tmp_path / "wscenhost_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DWSCENHOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "wscenhost ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
