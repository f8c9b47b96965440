"""CPU tests of the evolution strategy's stages: csrc/gl_es.hpp (host instantiation, tests/eshost/eshost.cpp -- a lane is a call, a
block a loop over 4 x 64 thread slots, the wavefront an array of 64) against NumPy restatements written from include/glgym.h.

Bounds.
* Philox words, utilities, n_adm, kept rows: EXACT.  With mean = 0 the odd child is the negated even child bit for bit, and for even
  k >= 2 the even child is glgym_plan_sample's (beta = 0, carry = 0) bit for bit.
* Sampled theta: within np.spacing(np.float32(1)) = 1.19e-7 absolute of the float64 restatement, test_plan_cem_host's bound for its
  reason: ln / cos / sin of two libms differ by a few double ulps, which can move the float32 rounding of a value of magnitude <= 1 by
  at most one float32 ulp <= 1.19e-7.
* The double g and s: within M * 2^-53 * (the largest |term| of that sum, computed here) of NumPy's -- M terms summed in another order.
* The stored mean: within one float32 ulp of NumPy's rounded value.  The stored std: within TWO float32 ulps -- the same bound with one
  more ulp, because exp comes from another libm (a few double ulps apart, which can move the float32 rounding once more).
* The loop: ||mean - theta*|| after 30 iterations is less than HALF the initial distance (a NumPy prototype of exactly this update
  with default_rng noise gave ratios 0.03-0.05 (SGD) and 0.10-0.19 (Adam) on three seeds); the generator is deterministic and LOOP_SEED
  was picked once so that the NumPy restatement itself passes, as MOMENT_SEED was in test_plan_cem_host."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_plan_cem_host import F32_STEP, M32, KEY_TAG, build_host as build_cem_host, make_returns, np_noise, ptr
from test_controller_and_noise import philox4x32_10

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SRC = ROOT / "tests" / "eshost" / "eshost.cpp"
SGD, ADAM = 0, 1
LOOP_SEED = 2026
DEFAULTS = dict(lr=0.05, lr_std=0.1, std_decay=0.995, min_std=0.02, max_std=1.0, beta1=0.9, beta2=0.999, eps=1e-8)


def build_host(path):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.eshost_sizeof.argtypes, lib.eshost_sizeof.restype = [C.c_int], C.c_int
    lib.eshost_words.argtypes, lib.eshost_words.restype = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p], None
    lib.eshost_pow_t.argtypes, lib.eshost_pow_t.restype = [C.c_double, C.c_uint64], C.c_double
    lib.eshost_sample.argtypes, lib.eshost_sample.restype = [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_uint64] * 2 + [C.c_void_p], None
    lib.eshost_utilities.argtypes, lib.eshost_utilities.restype = [C.c_int] * 2 + [C.c_void_p] * 4, None
    lib.eshost_update.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_double] * 8 + [C.c_uint64] + [C.c_void_p] * 8
    lib.eshost_update.restype = None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_es.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    return build_host(tmp_path_factory.mktemp("eshost") / "libeshost.so")


# ---- NumPy restatements (from the header's text, not from gl_es.hpp) ---------------------------------------------------------------
def np_es_sample(P, K, H, mean, std, seed, D):
    """theta in float64 BEFORE the cast [H, P*K, 6]: the even child's normals e (np_noise at beta = 0 is e itself), +e and -e."""
    e = np_noise(P * K, H, 0.0, seed, D)[:, 0::2].reshape(H, P, K // 2, 6)
    m, s = mean.astype(np.float64)[:, :, None, :], std.astype(np.float64)[:, :, None, :]
    out = np.empty((H, P, K // 2, 2, 6))
    out[:, :, :, 0], out[:, :, :, 1] = np.clip(m + s * e, -1.0, 1.0), np.clip(m + s * -e, -1.0, 1.0)
    return out.reshape(H, P * K, 6)


def np_utilities(P, K, ret, failed):
    u, n_adm = np.zeros((P, K)), np.zeros(P, np.int32)
    for p in range(P):
        r, f = ret[p * K:(p + 1) * K], failed[p * K:(p + 1) * K]
        idx = np.nonzero((f == 0) & np.isfinite(r))[0]
        n = n_adm[p] = len(idx)
        if n < 2:
            continue
        u[p] = -0.5
        u[p, idx[np.argsort(-r[idx], kind="stable")]] = 0.5 - np.arange(n) / (n - 1)
    return u, n_adm


def np_pow_t(b, t):
    r, q = 1.0, float(b)
    while t:
        if t & 1:
            r = r * q
        t >>= 1
        if t:
            q = q * q
    return r


def np_gs(P, K, H, theta, u, std):
    """-> g, s [H, P, 6] and the largest |term| of each sum."""
    M = K // 2
    th = theta.astype(np.float64).reshape(H, P, M, 2, 6)
    d = (th[:, :, :, 0] - th[:, :, :, 1]) * 0.5
    uu = u.reshape(P, M, 2)
    du, su = (uu[:, :, 0] - uu[:, :, 1])[None, :, :, None], (uu[:, :, 0] + uu[:, :, 1])[None, :, :, None]
    sig = std.astype(np.float64)[:, :, None, :]
    tg = du * d
    with np.errstate(all="ignore"):
        z = d / sig
        ts = np.where(sig > 0, su * (z * z - 1.0), 0.0)
    return tg.sum(axis=2) / M, ts.sum(axis=2) / M, np.abs(tg).max(axis=2), np.abs(ts).max(axis=2)


def np_update(opt, g, s, n_adm, mean, std, m1, m2, t, lr, lr_std, std_decay, min_std, max_std, beta1, beta2, eps):
    """-> mean', std' in float64 BEFORE the cast, m1', m2', and the mask [H, P] of the (row, plane)s that are kept."""
    keep = (n_adm < 2)[None, :] | ~np.isfinite(g).all(axis=2) | ~np.isfinite(s).all(axis=2)
    sig = std.astype(np.float64)
    with np.errstate(all="ignore"):
        if opt == ADAM:
            n1, n2 = beta1 * m1 + (1.0 - beta1) * g, beta2 * m2 + (1.0 - beta2) * (g * g)
            step = (lr * (n1 / (1.0 - np_pow_t(beta1, t)))) / (np.sqrt(n2 / (1.0 - np_pow_t(beta2, t))) + eps)
        else:
            n1, n2, step = m1, m2, lr * g
        mo = mean.astype(np.float64) + step
        so = np.minimum(np.maximum((sig * std_decay) * np.exp((0.5 * lr_std) * s), min_std), max_std)
    k3 = keep[:, :, None]
    return (np.where(k3, mean.astype(np.float64), mo), np.where(k3, sig, so), np.where(k3, m1, n1) if m1 is not None else None,
            np.where(k3, m2, n2) if m2 is not None else None, keep)


def within_f32_ulps(got32, ref64, n):
    ref32 = ref64.astype(np.float32)
    return (np.abs(got32.astype(np.float64) - ref32) <= n * np.spacing(np.maximum(np.abs(ref32), np.float32(1e-30))).astype(np.float64)).all()


def run_sample(host, P, K, H, mean, std, seed, D):
    out = np.full((H, P * K, 6), 7, np.float32)
    host.eshost_sample(P, K, H, ptr(mean), ptr(std), seed, D, ptr(out))
    return out


def run_utilities(host, P, K, ret, failed):
    u, n_adm = np.full((P, K), 9.0), np.full(P, 99, np.int32)
    host.eshost_utilities(P, K, ptr(ret), ptr(failed), ptr(u), ptr(n_adm))
    return u, n_adm


def run_update(host, P, K, H, opt, theta, u, n_adm, mean, std, m1, m2, t, in_place=False, **hp):
    """-> mean', std', m1', m2' (copies unless in_place), g, s."""
    hp = {**DEFAULTS, **hp}
    mo, so = (mean, std) if in_place else (np.full_like(mean, 7), np.full_like(std, 7))
    m1, m2 = (None if m1 is None else m1.copy()), (None if m2 is None else m2.copy())
    g, s = np.zeros((H, P, 6)), np.zeros((H, P, 6))
    host.eshost_update(P, K, H, opt, ptr(theta), ptr(u), ptr(n_adm), hp["lr"], hp["lr_std"], hp["std_decay"], hp["min_std"], hp["max_std"],
                       hp["beta1"], hp["beta2"], hp["eps"], t, ptr(m1), ptr(m2), ptr(mean), ptr(std), ptr(mo), ptr(so), ptr(g), ptr(s))
    return mo, so, m1, m2, g, s


def check_update(host, P, K, H, opt, theta, u, n_adm, mean, std, m1, m2, t, report=True, **hp):
    """One update against the restatement to the module's bounds; -> the host's results and the kept mask."""
    hpv = {**DEFAULTS, **hp}
    mo, so, n1, n2, g, s = run_update(host, P, K, H, opt, theta, u, n_adm, mean, std, m1, m2, t, **hp)
    e_g, e_s, big_g, big_s = np_gs(P, K, H, theta, u, std)
    fin = np.isfinite(e_g) & np.isfinite(e_s)
    assert np.array_equal(np.isfinite(g) & np.isfinite(s), fin)
    M = K // 2
    with np.errstate(invalid="ignore"):
        err_g, err_s = np.where(fin, np.abs(g - e_g), 0.0), np.where(fin, np.abs(s - e_s), 0.0)
        assert (err_g <= np.where(fin, M * 2.0 ** -53 * big_g, 0.0)).all(), (err_g.max(), big_g[fin].max())
        assert (err_s <= np.where(fin, M * 2.0 ** -53 * big_s, 0.0)).all(), (err_s.max(), big_s[fin].max())
    # the step from the HOST's sums, so that only the update's own arithmetic is compared to its bound
    e_mo, e_so, e_m1, e_m2, keep = np_update(opt, g, s, n_adm, mean, std, m1, m2, t, **hpv)
    assert within_f32_ulps(mo, e_mo, 1), np.abs(mo - e_mo).max()
    assert within_f32_ulps(so, e_so, 2), np.abs(so - e_so).max()
    assert np.array_equal(mo[keep], mean[keep]) and np.array_equal(so[keep], std[keep])
    if opt == ADAM:
        assert np.array_equal(n1, e_m1) and np.array_equal(n2, e_m2)       # +, * only: the same doubles
        assert np.array_equal(n1[keep], m1[keep]) and np.array_equal(n2[keep], m2[keep])
    if report:
        print(f"update P={P} K={K} H={H} opt={opt} t={t}: max |g - NumPy| = {err_g.max():.2e}, max |s - NumPy| = {err_s.max():.2e}")
    return mo, so, n1, n2, keep


def update_case(rng, host, P, K, H, std_lo=0.05):
    mean = rng.uniform(-0.8, 0.8, (H, P, 6)).astype(np.float32)
    std = rng.uniform(std_lo, 0.6, (H, P, 6)).astype(np.float32)
    theta = run_sample(host, P, K, H, mean, std, 77, 3)
    ret, failed = make_returns(rng, P, K)
    if K < 6:
        ret, failed = rng.normal(size=P * K), np.zeros(P * K, np.uint8)
    u, n_adm = run_utilities(host, P, K, ret, failed)
    m1, m2 = rng.normal(0, 0.01, (H, P, 6)), rng.uniform(0, 1e-4, (H, P, 6))
    return theta, u.reshape(-1), n_adm, mean, std, m1, m2


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
def test_args_structs_have_the_headers_sizes(host):
    from gl_gym_amd import _lib as L
    for which, cls in enumerate((L.PlanEsSampleArgs, L.PlanEsUtilitiesArgs, L.PlanEsUpdateArgs)):
        assert C.sizeof(cls) == host.eshost_sizeof(which), cls.__name__
        assert cls._fields_[0][0] == "struct_size"
    for name in ("glgym_plan_es_sample", "glgym_plan_es_utilities", "glgym_plan_es_update"):
        assert name in L.PROTOTYPES
    assert L.ES_OPTIMIZERS == {"sgd": SGD, "adam": ADAM}


def test_philox_words_are_exact(host):
    seed, D = 0x0123456789ABCDEF, (5 << 32) | 77
    for c, h in ((0, 0), (2, 0), (68, 2), (4094, 47), (2 ** 31 - 2, 65534)):
        r = np.zeros(8, np.uint32)
        host.eshost_words(c, h, D, seed, ptr(r))
        exp = []
        for blk in (0, 1):
            exp += philox4x32_10([c, 2 * h + blk, D & M32, D >> 32], [seed & M32, (seed >> 32) ^ KEY_TAG])
        assert r.tolist() == exp, (c, h)


@pytest.mark.parametrize("P,K,H", [(3, 70, 3), (2, 258, 2), (1, 2, 1), (3, 6, 5), (1, 66, 1)])
def test_sample_matches_numpy(host, P, K, H):
    rng = np.random.default_rng(K)
    mean = rng.uniform(-1.2, 1.2, (H, P, 6)).astype(np.float32)            # some means outside the box
    std = rng.uniform(0.05, 0.6, (H, P, 6)).astype(np.float32)
    seed, D = 0xDEADBEEF12345678, 2 ** 40 + 3
    got = run_sample(host, P, K, H, mean, std, seed, D)
    exp = np_es_sample(P, K, H, mean, std, seed, D)
    err = np.abs(got.astype(np.float64) - exp).max()
    print(f"es sample P={P} K={K} H={H}: max |theta - float64 restatement| = {err:.2e} (bound {F32_STEP:.2e})")
    assert err <= F32_STEP and (np.abs(got) <= 1).all()
    assert not np.array_equal(run_sample(host, P, K, H, mean, std, seed, D + 1), got)
    assert not np.array_equal(run_sample(host, P, K, H, mean, std, seed + 1, D), got)
    assert np.array_equal(run_sample(host, P, K, H, mean, std, seed, D), got)


@pytest.mark.parametrize("P,K,H", [(2, 70, 3), (1, 2, 2), (3, 258, 1)])
def test_mirror_is_exact_around_a_zero_mean(host, P, K, H):
    mean, std = np.zeros((H, P, 6), np.float32), np.random.default_rng(1).uniform(0.05, 3.0, (H, P, 6)).astype(np.float32)
    got = run_sample(host, P, K, H, mean, std, 5, 9)
    plus, minus = got[:, 0::2], got[:, 1::2]
    assert np.array_equal(minus.view(np.uint32), (-plus).view(np.uint32))   # bit for bit, the clipped ones included
    assert (np.abs(got) == 1).any() and (np.abs(got) < 1).any()


@pytest.mark.parametrize("P,K,H", [(3, 70, 3), (2, 258, 2), (1, 2, 1)])
def test_even_children_are_the_cem_samples(host, tmp_path_factory, P, K, H):
    cem = build_cem_host(tmp_path_factory.mktemp("cemhost_es") / "libcemhost.so")
    rng = np.random.default_rng(3)
    mean, std = rng.uniform(-1.1, 1.1, (H, P, 6)).astype(np.float32), rng.uniform(0.05, 0.6, (H, P, 6)).astype(np.float32)
    seed, D = 0xABCDEF0123, 41
    got = run_sample(host, P, K, H, mean, std, seed, D).reshape(H, P, K, 6)
    ref = np.full((H, P * K, 6), 7, np.float32)
    cem.cemhost_sample(P, K, H, ptr(mean), ptr(std), 0.0, seed, D, 0, 0, None, None, None, ptr(ref))
    ref = ref.reshape(H, P, K, 6)
    assert np.array_equal(got[:, :, 2::2].view(np.uint32), ref[:, :, 2::2].view(np.uint32))   # k = 0 is the CEM's reserved mean
    if K > 2:
        assert not np.array_equal(got[:, :, 3::2], ref[:, :, 3::2])       # the odd children are mirrors, not draws of their own


@pytest.mark.parametrize("K", [2, 6, 66, 258])
def test_utilities_are_exact(host, K):
    P = 5
    rng = np.random.default_rng(300 + K)
    ret, failed = make_returns(rng, P, K)                                 # random returns, ties, NaN, +-inf, failed flags
    if K == 2:
        ret[:], failed[:] = rng.normal(size=P * K), 0
        ret[0:2] = 1.5                                                    # row 0: a tie -> the lower index is the better
    ret[K:2 * K] = 2.0                                                    # row 1: all equal -> ranks 0, 1, 2, ... by index
    failed[K:2 * K] = 0
    failed[2 * K:3 * K] = 1                                               # row 2: n = 0
    ret[3 * K:4 * K] = np.nan                                             # row 3: n = 1
    ret[3 * K + K - 1], failed[3 * K + K - 1] = -3.0, 0
    ret[4 * K:5 * K] = np.where(np.arange(K) % 2 == 0, np.inf, -np.inf)   # row 4: infinities only -> n = 0
    got = run_utilities(host, P, K, ret, failed)
    exp = np_utilities(P, K, ret, failed)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert got[1][1:].tolist() == [K, 0, 1, 0] and (got[0][2:] == 0).all()
    assert np.array_equal(got[0][1], 0.5 - np.arange(K) / (K - 1)) and got[0][1, 0] == 0.5 and got[0][1, -1] == -0.5
    if K == 2:
        assert got[0][0].tolist() == [0.5, -0.5]


def test_utilities_with_two_admissible_and_signed_zeros(host):
    K = 66
    ret, failed = np.full(K, np.nan), np.zeros(K, np.uint8)
    ret[[5, 65]] = [1.0, 4.0]                                             # n = 2: +0.5 and -0.5, everything else -0.5
    u, n = run_utilities(host, 1, K, ret, failed)
    assert n.tolist() == [2] and u[0, 65] == 0.5 and u[0, 5] == -0.5 and (np.delete(u[0], [65]) == -0.5).all()
    r2, f2 = np.array([0.0, -0.0, 0.0, 1.0]), np.zeros(4, np.uint8)       # -0.0 and 0.0 tie
    assert np.array_equal(run_utilities(host, 1, 4, r2, f2)[0], np_utilities(1, 4, r2, f2)[0])
    assert run_utilities(host, 1, 4, r2, f2)[0].tolist() == [[0.5 - 1 / 3, 0.5 - 2 / 3, -0.5, 0.5]]


def test_pow_t_is_the_documented_square_and_multiply(host):
    for b in (0.0, 0.5, 0.9, 0.999, 0.123456789):
        for t in (1, 2, 3, 5, 1000, 2 ** 40 + 12345):
            assert host.eshost_pow_t(b, t) == np_pow_t(b, t), (b, t)
    assert abs(np_pow_t(0.999, 1000) - 0.999 ** 1000) < 1e-12


@pytest.mark.parametrize("opt", [SGD, ADAM])
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("K", [2, 66, 130, 258])                         # M = 1, 33, 65, 129
def test_update_matches_numpy(host, opt, t, K):
    P, H = 3, 2
    rng = np.random.default_rng(1000 * K + t)
    theta, u, n_adm, mean, std, m1, m2 = update_case(rng, host, P, K, H)
    if t == 1:
        m1[:], m2[:] = 0.0, 0.0
    mo, so, n1, n2, keep = check_update(host, P, K, H, opt, theta, u, n_adm, mean, std, m1, m2, t)
    assert not keep.any() and not np.array_equal(mo, mean) and not np.array_equal(so, std)
    # in place equals out of place
    mi, si = mean.copy(), std.copy()
    ri = run_update(host, P, K, H, opt, theta, u, n_adm, mi, si, m1, m2, t, in_place=True)
    assert np.array_equal(mi, mo) and np.array_equal(si, so)
    if opt == ADAM:
        assert np.array_equal(ri[2], n1) and np.array_equal(ri[3], n2)


@pytest.mark.parametrize("opt", [SGD, ADAM])
def test_update_with_a_zero_std_and_a_mean_on_the_box(host, opt):
    P, K, H = 2, 66, 2
    rng = np.random.default_rng(8)
    mean = rng.uniform(-0.5, 0.5, (H, P, 6)).astype(np.float32)
    std = rng.uniform(0.1, 0.4, (H, P, 6)).astype(np.float32)
    std[0, 0, 2] = 0.0                                                    # a std component of 0: no spread term, std' = min_std
    mean[1, 1, 3], mean[1, 0, 4] = 1.0, -1.0                              # a mean on +-1: one member of every pair is clipped
    mean[0, 1, 5], std[0, 1, 5] = 1.0, 0.0                                # ... and both: d = 0
    theta = run_sample(host, P, K, H, mean, std, 4, 4)
    assert (theta[1].reshape(P, K, 6)[1, :, 3] == 1).sum() >= K // 2 and (theta[0].reshape(P, K, 6)[1, :, 5] == 1).all()
    u, n_adm = run_utilities(host, P, K, rng.normal(size=P * K), np.zeros(P * K, np.uint8))
    m1, m2 = np.zeros((H, P, 6)), np.zeros((H, P, 6))
    mo, so, _, _, keep = check_update(host, P, K, H, opt, theta, u.reshape(-1), n_adm, mean, std, m1, m2, 1, min_std=0.03)
    assert not keep.any() and so[0, 0, 2] == np.float32(0.03) and so[0, 1, 5] == np.float32(0.03)
    assert mo[0, 1, 5] == mean[0, 1, 5] and mo[0, 0, 2] == mean[0, 0, 2]  # no spread, no step
    assert (so >= np.float32(0.03)).all() and (so <= 1).all()


@pytest.mark.parametrize("opt", [SGD, ADAM])
def test_update_keeps_rows_without_two_admissible_candidates_or_with_a_nan(host, opt):
    P, K, H = 4, 66, 3
    rng = np.random.default_rng(9)
    theta, _, _, mean, std, m1, m2 = update_case(rng, host, P, K, H)
    ret, failed = rng.normal(size=P * K), np.zeros(P * K, np.uint8)
    failed[0:K] = 1                                                       # row 0: n = 0
    ret[K:2 * K] = np.nan
    ret[K + 7] = 1.0                                                      # row 1: n = 1
    u, n_adm = run_utilities(host, P, K, ret, failed)
    assert n_adm.tolist() == [0, 1, K, K]
    theta[1, 2 * K + 11, 4] = np.nan                                      # row 2, plane 1: a NaN in theta -> that plane is kept
    mo, so, n1, n2, keep = check_update(host, P, K, H, opt, theta, u.reshape(-1), n_adm, mean, std, m1, m2, 5)
    exp_keep = np.zeros((H, P), bool)
    exp_keep[:, :2], exp_keep[1, 2] = True, True
    assert np.array_equal(keep, exp_keep)
    assert np.array_equal(mo[keep].view(np.uint32), mean[keep].view(np.uint32)) and np.array_equal(so[keep].view(np.uint32), std[keep].view(np.uint32))
    assert np.array_equal(n1[keep], m1[keep]) and np.array_equal(n2[keep], m2[keep])
    assert not np.array_equal(mo[~keep], mean[~keep])
    # in place: the kept rows are rewritten with their own values
    mi, si = mean.copy(), std.copy()
    run_update(host, P, K, H, opt, theta, u.reshape(-1), n_adm, mi, si, m1, m2, 5, in_place=True)
    assert np.array_equal(mi, mo) and np.array_equal(si, so)


def es_loop(K, Ht, target, opt, n_iter, init_std, hp, sample, utilities, update):
    """n_iter x (sample -> score -> utilities -> update) with the three stages given; -> the means after every iteration."""
    mean, std = np.zeros((Ht, 1, 6), np.float32), np.full((Ht, 1, 6), init_std, np.float32)
    m1, m2 = np.zeros((Ht, 1, 6)), np.zeros((Ht, 1, 6))
    trace = []
    for it in range(n_iter):
        theta = sample(mean, std, it)
        ret = -((theta.astype(np.float64).transpose(1, 0, 2).reshape(K, Ht * 6) - target) ** 2).sum(axis=1)
        u, n_adm = utilities(ret)
        mean, std, m1, m2 = update(theta, u, n_adm, mean, std, m1, m2, it + 1)
        trace.append((theta, u, mean, std, m1, m2))
    return trace


@pytest.mark.parametrize("opt,hp", [(SGD, dict(lr=0.5, lr_std=0.2)), (ADAM, dict(lr=0.03, lr_std=0.0))])
def test_the_loop_optimises(host, opt, hp):
    """Score = -||theta_k - theta*||^2 with D = 12, K = 16, 30 iterations, init_std 0.3, min_std 0.01: the distance of the mean to
    theta* falls below half the initial one, in the NumPy restatement and in the host build, which equals the restatement's stages
    at every iteration to the module's bounds (each iteration compared from the host's own state)."""
    K, Ht, n_iter = 16, 2, 30
    target = np.random.default_rng(12).uniform(-0.6, 0.6, Ht * 6)
    hp = {**DEFAULTS, "std_decay": 1.0, "min_std": 0.01, **hp}
    zeros = np.zeros(K, np.uint8)

    def np_upd(theta, u, n_adm, mean, std, m1, m2, t):
        g, s, _, _ = np_gs(1, K, Ht, theta, u.reshape(-1), std)
        mo, so, n1, n2, _ = np_update(opt, g, s, n_adm, mean, std, m1, m2, t, **hp)
        return mo.astype(np.float32), so.astype(np.float32), n1, n2

    ref = es_loop(K, Ht, target, opt, n_iter, 0.3, hp, lambda m, s, it: np_es_sample(1, K, Ht, m, s, LOOP_SEED, it).astype(np.float32),
                  lambda ret: np_utilities(1, K, ret, zeros), np_upd)
    d0 = np.linalg.norm(target)
    d_ref = np.linalg.norm(ref[-1][2].reshape(-1) - target)
    assert d_ref < 0.5 * d0, (d_ref, d0)                                  # the seed's own NumPy restatement passes

    def host_upd(theta, u, n_adm, mean, std, m1, m2, t):
        # every stage of this iteration against the restatement FROM THE HOST'S STATE
        assert np.abs(theta.astype(np.float64) - np_es_sample(1, K, Ht, mean, std, LOOP_SEED, t - 1)).max() <= F32_STEP
        mo, so, n1, n2, keep = check_update(host, 1, K, Ht, opt, theta, u.reshape(-1), n_adm, mean, std, m1, m2, t, report=False, **hp)
        assert not keep.any()
        return mo, so, n1, n2

    def host_util(ret):
        got, exp = run_utilities(host, 1, K, ret, zeros), np_utilities(1, K, ret, zeros)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
        return got

    got = es_loop(K, Ht, target, opt, n_iter, 0.3, hp, lambda m, s, it: run_sample(host, 1, K, Ht, m, s, LOOP_SEED, it), host_util, host_upd)
    d_got = np.linalg.norm(got[-1][2].reshape(-1) - target)
    print(f"loop opt={opt}: ||mean - theta*|| {d0:.4f} -> host {d_got:.4f} (ratio {d_got / d0:.3f}), NumPy {d_ref:.4f} (ratio {d_ref / d0:.3f})")
    assert d_got < 0.5 * d0, (d_got, d0)


# ---- argument checking through libglgym.so: no device is needed, the refusals come before the handle is looked at ------------------
@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from gl_gym_amd import _lib as L
    if not L.LIB_PATH.exists():
        g.build()
    return L, L.load()


P_ = 0x1000                                                              # a non-null, 16-byte aligned pointer: never followed


def refused(lib, fn, a, word):
    from gl_gym_amd import _lib as L
    assert fn(None, C.byref(a), None) == L.EINVAL, word
    msg = lib.glgym_last_error()
    assert msg and word in msg, (word, msg)


SHAPE_REFUSALS = (("struct_size", 8, b"struct_size"), ("P", 0, b"P or H < 1"), ("K", 0, b"K < 2"), ("K", 1, b"K < 2"), ("K", 7, b"K is odd"),
                  ("K", -2, b"K < 2"), ("P", 2 ** 30, b"past INT32_MAX"))


def test_es_sample_refusals(capi):
    L, lib = capi
    good = lambda: L.make_plan_args(L.PlanEsSampleArgs, 3, 8, 5, P_, P_, 1, 2, None, P_)  # noqa: E731
    refused(lib, lib.glgym_plan_es_sample, good(), b"glgym_plan_es_sample: null handle")
    for field, value, word in SHAPE_REFUSALS + (("H", 0, b"P or H < 1"), ("H", 65536, b"H > 65 535"), ("mean", None, b"null mean"),
                                                ("std", None, b"null mean"), ("actions", None, b"null mean"),
                                                ("actions", P_ + 8, b"16-byte aligned")):
        a = good()
        setattr(a, field, value)
        refused(lib, lib.glgym_plan_es_sample, a, word)
        assert b"glgym_plan_es_sample" in lib.glgym_last_error()
    a = good()
    a.H, a.draw_base = 65535, P_
    refused(lib, lib.glgym_plan_es_sample, a, b"null handle")
    assert lib.glgym_plan_es_sample(None, None, None) == L.EINVAL


def test_es_utilities_refusals(capi):
    L, lib = capi
    good = lambda: L.make_plan_args(L.PlanEsUtilitiesArgs, 3, 8, P_, P_, P_, P_)  # noqa: E731
    refused(lib, lib.glgym_plan_es_utilities, good(), b"glgym_plan_es_utilities: null handle")
    for field, value, word in SHAPE_REFUSALS + tuple((f, None, b"null ret") for f in ("ret", "failed", "u", "n_adm")):
        a = good()
        setattr(a, field, value)
        refused(lib, lib.glgym_plan_es_utilities, a, word)
        assert b"glgym_plan_es_utilities" in lib.glgym_last_error()
    assert lib.glgym_plan_es_utilities(None, None, None) == L.EINVAL


def test_es_update_refusals(capi):
    L, lib = capi
    nan, inf = float("nan"), float("inf")

    def good(opt=ADAM):
        return L.make_plan_args(L.PlanEsUpdateArgs, 3, 8, 5, opt, P_, P_, P_, 0.05, 0.1, 1.0, 0.02, 1.0, 0.9, 0.999, 1e-8, 1, None, P_, P_,
                                P_, P_, P_, P_)

    for opt in (SGD, ADAM):
        refused(lib, lib.glgym_plan_es_update, good(opt), b"glgym_plan_es_update: null handle")
    cases = SHAPE_REFUSALS + (("H", 0, b"P or H < 1"), ("H", 65536, b"H > 65 535"), ("optimizer", 2, b"optimizer"), ("optimizer", -1, b"optimizer"),
                              ("actions", P_ + 8, b"16-byte aligned"), ("u", P_ + 8, b"16-byte aligned"),
                              ("lr", -1.0, b"lr negative"), ("lr", nan, b"lr negative"), ("lr", inf, b"lr negative"),
                              ("lr_std", -1.0, b"lr_std negative"), ("lr_std", nan, b"lr_std negative"), ("lr_std", inf, b"lr_std negative"),
                              ("std_decay", 0.0, b"std_decay"), ("std_decay", -0.5, b"std_decay"), ("std_decay", nan, b"std_decay"),
                              ("std_decay", inf, b"std_decay"), ("min_std", -0.1, b"min_std"), ("min_std", nan, b"min_std"),
                              ("min_std", 1.5, b"min_std > max_std"), ("max_std", inf, b"max_std not finite"), ("max_std", nan, b"max_std"),
                              ("max_std", 0.01, b"min_std > max_std"), ("t_index", 0, b"t_index = 0"))
    cases += tuple((f, None, b"null actions") for f in ("actions", "u", "n_adm", "mean", "std", "mean_out", "std_out"))
    adam_only = (("beta1", 1.0, b"outside [0, 1)"), ("beta1", -0.1, b"outside [0, 1)"), ("beta1", nan, b"outside [0, 1)"),
                 ("beta2", 1.0, b"outside [0, 1)"), ("beta2", -0.1, b"outside [0, 1)"), ("beta2", nan, b"outside [0, 1)"),
                 ("eps", 0.0, b"eps"), ("eps", -1e-8, b"eps"), ("eps", nan, b"eps"), ("eps", inf, b"eps"),
                 ("m1", None, b"without m1 or m2"), ("m2", None, b"without m1 or m2"))
    for opt in (SGD, ADAM):
        for field, value, word in cases:
            a = good(opt)
            setattr(a, field, value)
            refused(lib, lib.glgym_plan_es_update, a, word)
            assert b"glgym_plan_es_update" in lib.glgym_last_error()
    for field, value, word in adam_only:
        a = good(ADAM)
        setattr(a, field, value)
        refused(lib, lib.glgym_plan_es_update, a, word)
        a = good(SGD)                                                     # ... SGD does not look at them
        setattr(a, field, value)
        refused(lib, lib.glgym_plan_es_update, a, b"null handle")
    a = good()                                                           # the edges that are allowed
    a.beta1, a.beta2, a.lr, a.lr_std, a.min_std, a.max_std, a.t_base = 0.0, 0.0, 0.0, 0.0, 0.5, 0.5, P_
    refused(lib, lib.glgym_plan_es_update, a, b"null handle")
    assert lib.glgym_plan_es_update(None, None, None) == L.EINVAL


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """tests/eshost/eshost.cpp with its own main, AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (nothing is
    loaded into Python): exactly sized heap buffers at the awkward shapes, so an index past a row end is reported."""
    exe = tmp_path / "eshost_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DESHOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "eshost ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
