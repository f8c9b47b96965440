"""CPU tests of the cross-entropy method's stages: csrc/gl_cem.hpp (host instantiation, tests/cemhost/cemhost.cpp -- a lane is a
call, a block a loop over 4 x 64 thread slots, the wavefront an array of 64) against NumPy restatements written from include/glgym.h.

Bounds.
* Philox words, candidate 0, carried candidates, elite_k, n_elite: EXACT.
* Sampled actions: within np.spacing(np.float32(1)) = 1.19e-7 absolute of the float64 restatement.  ln / cos / sin of two libms differ
  by a few double ulps, which can move the float32 rounding of a value of magnitude <= 1 by at most one float32 ulp <= 1.19e-7.
* Moments (K = 4 096, H = 2, std 0.2, beta 0.9, N = K - 1 sampled candidates): mean within 5 / sqrt(N) of 0, variance within
  5 sqrt(2 / N) of 1, lag-1 correlation within 5 / sqrt(N) of 0.9 -- five standard errors; the generator is deterministic and
  MOMENT_SEED was picked once so that the NumPy restatement itself passes.
* Refit: the double moments within E * 2^-53 of NumPy's (E terms of magnitude <= 1 summed in another order), the stored float32 within
  one float32 ulp of NumPy's rounded value."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_controller_and_noise import philox4x32_10

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SRC = ROOT / "tests" / "cemhost" / "cemhost.cpp"
KEY_TAG = 0x43454D31
M32 = 0xFFFFFFFF
F32_STEP = float(np.spacing(np.float32(1)))
MOMENT_SEED = 2026


def build_host(path):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.cemhost_sizeof.argtypes, lib.cemhost_sizeof.restype = [C.c_int], C.c_int
    lib.cemhost_words.argtypes, lib.cemhost_words.restype = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p], None
    lib.cemhost_sample.argtypes = [C.c_int] * 3 + [C.c_void_p] * 2 + [C.c_double, C.c_uint64, C.c_uint64, C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.cemhost_sample.restype = None
    lib.cemhost_elites.argtypes, lib.cemhost_elites.restype = [C.c_int] * 3 + [C.c_void_p] * 4, None
    lib.cemhost_refit.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_double] * 2 + [C.c_void_p] * 6
    lib.cemhost_refit.restype = None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_cem.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    return build_host(tmp_path_factory.mktemp("cemhost") / "libcemhost.so")


def ptr(a):
    return None if a is None else a.ctypes.data


# ---- NumPy restatements (from the header's text, not from gl_cem.hpp) ------------------------------------------------------
def np_philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over arrays: the definition of tests/test_controller_and_noise.py, vectorised (checked against it below)."""
    c = [np.broadcast_to(np.asarray(v, dtype=np.uint64), np.shape(c0)).copy() for v in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & M32, int(k1) & M32
    m = np.uint64(M32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0)) & m, p1 & m, ((p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1)) & m, p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack(c, axis=-1)


def np_words(n_children, h, D, seed):
    """r0..r7 of every child at step h: [C, 8] uint64."""
    c = np.arange(n_children, dtype=np.uint64)
    return np.concatenate([np_philox(c, 2 * h + blk, D & M32, D >> 32, seed & M32, (seed >> 32) ^ KEY_TAG) for blk in (0, 1)], axis=-1)


def np_noise(n_children, H, beta, seed, D):
    """The coloured noise n [H, C, 6] in float64."""
    n = np.zeros((H, n_children, 6))
    for h in range(H):
        u = (np_words(n_children, h, D, seed).astype(np.float64) + 0.5) * 2.0 ** -32
        e = np.empty((n_children, 6))
        for m in range(3):
            rad, ang = np.sqrt(-2.0 * np.log(u[:, 2 * m])), 2.0 * np.pi * u[:, 2 * m + 1]
            e[:, 2 * m], e[:, 2 * m + 1] = rad * np.cos(ang), rad * np.sin(ang)
        n[h] = e if h == 0 else beta * n[h - 1] + np.sqrt(1.0 - beta * beta) * e
    return n


def np_sample(P, K, H, mean, std, beta, seed, D, carry=0, prev_actions=None, prev_elite_k=None, prev_n_elite=None):
    """-> the action block in float64 BEFORE the cast [H, P*K, 6], and a mask [P*K] of the candidates that are copies (exact)."""
    n = np_noise(P * K, H, beta, seed, D).reshape(H, P, K, 6)
    v = np.clip(mean.astype(np.float64)[:, :, None, :] + std.astype(np.float64)[:, :, None, :] * n, -1.0, 1.0)
    v[:, :, 0] = np.clip(mean.astype(np.float64), -1.0, 1.0)
    exact = np.zeros((P, K), bool)
    exact[:, 0] = True
    for p in range(P):
        for k in range(1, min(carry, K - 1) + 1):
            if k - 1 < prev_n_elite[p]:
                v[:, p, k] = prev_actions[:, p * K + prev_elite_k[p, k - 1]]
                exact[p, k] = True
    return v.reshape(H, P * K, 6), exact.reshape(-1)


def np_elites(P, K, E, ret, failed):
    elite, n_elite = np.full((P, E), -1, np.int32), np.zeros(P, np.int32)
    for p in range(P):
        r, f = ret[p * K:(p + 1) * K], failed[p * K:(p + 1) * K]
        idx = np.nonzero((f == 0) & np.isfinite(r))[0]
        order = idx[np.argsort(-r[idx], kind="stable")][:E]
        elite[p, :len(order)], n_elite[p] = order, len(order)
    return elite, n_elite


def np_refit(P, K, H, actions, elite, n_elite, alpha, min_std, mean, std):
    """-> mean', std' in float64 BEFORE the cast, and the moments m, s (NaN where a parent is kept)."""
    mo, so = mean.astype(np.float64), std.astype(np.float64)
    m, s = np.full((H, P, 6), np.nan), np.full((H, P, 6), np.nan)
    for p in range(P):
        n = int(n_elite[p])
        if n == 0:
            continue
        a = actions[:, p * K + elite[p, :n]].astype(np.float64)            # [H, n, 6]
        m[:, p] = a.sum(axis=1) / n
        s[:, p] = np.sqrt(((a - m[:, p][:, None, :]) ** 2).sum(axis=1) / n)
        mo[:, p] = alpha * mean[:, p].astype(np.float64) + (1.0 - alpha) * m[:, p]
        so[:, p] = np.maximum(alpha * std[:, p].astype(np.float64) + (1.0 - alpha) * s[:, p], min_std)
    return mo, so, m, s


def within_one_f32_ulp(got32, ref64):
    ref32 = ref64.astype(np.float32)
    return (np.abs(got32.astype(np.float64) - ref32) <= np.spacing(np.maximum(np.abs(ref32), np.float32(1e-30)))).all()


def run_sample(host, P, K, H, mean, std, beta, seed, D, carry=0, prev_E=0, prev_actions=None, prev_elite_k=None, prev_n_elite=None):
    out = np.full((H, P * K, 6), 7, np.float32)
    host.cemhost_sample(P, K, H, ptr(mean), ptr(std), beta, seed, D, carry, prev_E, ptr(prev_actions), ptr(prev_elite_k), ptr(prev_n_elite),
                        ptr(out))
    return out


def run_elites(host, P, K, E, ret, failed):
    elite, n_elite = np.full((P, E), 99, np.int32), np.full(P, 99, np.int32)
    host.cemhost_elites(P, K, E, ptr(ret), ptr(failed), ptr(elite), ptr(n_elite))
    return elite, n_elite


def make_returns(rng, P, K):
    """Returns with ties, failures, NaN and both infinities."""
    ret = np.round(rng.normal(size=P * K) * 3.0) / 2.0                     # half-integers: many exact ties
    ret[rng.random(P * K) < 0.3] += rng.normal()                           # ... among other values
    failed = (rng.random(P * K) < 0.1).astype(np.uint8)
    bad = rng.random(P * K)
    ret[bad < 0.05] = np.nan
    ret[(bad >= 0.05) & (bad < 0.08)] = np.inf
    ret[(bad >= 0.08) & (bad < 0.10)] = -np.inf
    return ret, failed


def moment_checks(n, beta):
    """n [2, N, 6]: the five-standard-error checks of the module docstring; -> the worst of each for the report."""
    N = n.shape[1]
    mean, var = n.mean(axis=1), n.var(axis=1)
    d0, d1 = n[0] - n[0].mean(axis=0), n[1] - n[1].mean(axis=0)
    corr = (d0 * d1).mean(axis=0) / np.sqrt((d0 * d0).mean(axis=0) * (d1 * d1).mean(axis=0))
    worst = np.abs(mean).max(), np.abs(var - 1.0).max(), np.abs(corr - beta).max()
    assert worst[0] <= 5 / np.sqrt(N), worst
    assert worst[1] <= 5 * np.sqrt(2 / N), worst
    assert worst[2] <= 5 / np.sqrt(N), worst
    return worst


# ---- tests -------------------------------------------------------------------------------------------------------------------
def test_args_structs_have_the_headers_sizes(host):
    from gl_gym_amd import _lib as L
    for which, cls in enumerate((L.PlanSampleArgs, L.PlanElitesArgs, L.PlanRefitArgs)):
        assert C.sizeof(cls) == host.cemhost_sizeof(which), cls.__name__
        assert cls._fields_[0][0] == "struct_size"
    a = L.make_plan_args(L.PlanElitesArgs, 3, 5, 2)
    assert (a.struct_size, a.P, a.K, a.E) == (C.sizeof(L.PlanElitesArgs), 3, 5, 2)
    for name in ("glgym_plan_sample", "glgym_plan_elites", "glgym_plan_refit"):
        assert name in L.PROTOTYPES


def test_philox_words_are_exact(host):
    seed, D = 0x0123456789ABCDEF, (5 << 32) | 77
    for c, h in ((0, 0), (1, 0), (69, 2), (4095, 47), (2 ** 31 - 1, 65535)):
        r = np.zeros(8, np.uint32)
        host.cemhost_words(c, h, D, seed, ptr(r))
        exp = []
        for blk in (0, 1):                                                 # the scalar definition the device generators are held to
            exp += philox4x32_10([c, 2 * h + blk, D & M32, D >> 32], [seed & M32, (seed >> 32) ^ KEY_TAG])
        assert r.tolist() == exp, (c, h)
    vec = np_words(70, 2, D, seed)                                         # ... and the vectorised restatement used below is that definition
    assert vec[69].tolist() == [int(x) for x in exp_words(69, 2, D, seed)]
    # apart from the crop-noise stream: the same counter under the untagged key gives other words
    assert philox4x32_10([0, 0, D & M32, D >> 32], [seed & M32, seed >> 32]) != exp_words(0, 0, D, seed)[:4]


def exp_words(c, h, D, seed):
    out = []
    for blk in (0, 1):
        out += philox4x32_10([c, 2 * h + blk, D & M32, D >> 32], [seed & M32, (seed >> 32) ^ KEY_TAG])
    return out


@pytest.mark.parametrize("P,K,H,beta", [(3, 70, 3, 0.5), (2, 300, 2, 0.0), (1, 1, 1, 0.9), (2, 257, 4, 0.95)])
def test_sample_matches_numpy(host, P, K, H, beta):
    rng = np.random.default_rng(K)
    mean = rng.uniform(-1.2, 1.2, (H, P, 6)).astype(np.float32)            # some means outside the box: candidate 0 is CLIPPED
    std = rng.uniform(0.05, 0.6, (H, P, 6)).astype(np.float32)
    seed, D = 0xDEADBEEF12345678, 2 ** 40 + 3
    got = run_sample(host, P, K, H, mean, std, beta, seed, D)
    exp, exact = np_sample(P, K, H, mean, std, beta, seed, D)
    err = np.abs(got.astype(np.float64) - exp).max()
    print(f"sample P={P} K={K} H={H} beta={beta}: max |action - float64 restatement| = {err:.2e} (bound {F32_STEP:.2e})")
    assert err <= F32_STEP
    assert np.array_equal(got[:, exact], exp[:, exact].astype(np.float32))  # candidate 0: the clipped mean, exactly
    assert np.array_equal(got.reshape(H, P, K, 6)[:, :, 0], np.clip(mean, -1, 1))
    assert (np.abs(got) <= 1).all()
    # another draw index, another seed: other noise (K = 1 has only the reserved candidate)
    if K > 1:
        assert not np.array_equal(run_sample(host, P, K, H, mean, std, beta, seed, D + 1), got)
        assert not np.array_equal(run_sample(host, P, K, H, mean, std, beta, seed + 1, D), got)
    assert np.array_equal(run_sample(host, P, K, H, mean, std, beta, seed, D), got)


def test_sample_carries_the_previous_elites_exactly(host):
    P, K, H, E, carry = 3, 70, 3, 7, 4
    rng = np.random.default_rng(5)
    mean, std = np.zeros((H, P, 6), np.float32), np.full((H, P, 6), 0.4, np.float32)
    prev = run_sample(host, P, K, H, mean, std, 0.3, 1, 10)
    ret, failed = make_returns(rng, P, K)
    failed[K:2 * K] = 1
    failed[K + 5], ret[K + 5], failed[K + 9], ret[K + 9] = 0, 1.0, 0, 2.0   # parent 1: two admissible candidates < carry
    failed[2 * K:] = 1                                                    # parent 2: none
    elite, n_elite = np_elites(P, K, E, ret, failed)
    assert n_elite.tolist() == [7, 2, 0] and elite[1].tolist() == [9, 5, -1, -1, -1, -1, -1]
    got = run_sample(host, P, K, H, mean, std, 0.3, 1, 11, carry, E, prev, elite, n_elite)
    exp, exact = np_sample(P, K, H, mean, std, 0.3, 1, 11, carry, prev, elite, n_elite)
    assert exact.reshape(P, K).sum(axis=1).tolist() == [5, 3, 1]
    assert np.array_equal(got[:, exact], exp[:, exact].astype(np.float32))
    for p in range(P):
        for k in range(1, carry + 1):
            if k - 1 < n_elite[p]:
                assert np.array_equal(got[:, p * K + k], prev[:, p * K + elite[p, k - 1]])
    assert np.abs(got.astype(np.float64) - exp).max() <= F32_STEP           # the others are sampled as without carry
    fresh = run_sample(host, P, K, H, mean, std, 0.3, 1, 11)
    assert np.array_equal(got[:, ~exact], fresh[:, ~exact])
    # carry beyond K - 1 stops at the last candidate
    P2, K2 = 1, 3
    m2, s2 = np.zeros((1, P2, 6), np.float32), np.ones((1, P2, 6), np.float32)
    prev2 = run_sample(host, P2, K2, 1, m2, s2, 0.0, 1, 0)
    el2, n2 = np.array([[2, 1, 0]], np.int32), np.array([3], np.int32)
    got2 = run_sample(host, P2, K2, 1, m2, s2, 0.0, 1, 1, 3, 3, prev2, el2, n2)
    assert np.array_equal(got2[0, 1], prev2[0, 2]) and np.array_equal(got2[0, 2], prev2[0, 1]) and (got2[0, 0] == 0).all()


def test_sample_clips_at_the_box(host):
    P, K, H = 2, 300, 2
    mean, std = np.zeros((H, P, 6), np.float32), np.full((H, P, 6), 10.0, np.float32)
    got = run_sample(host, P, K, H, mean, std, 0.0, 9, 0)
    exp, _ = np_sample(P, K, H, mean, std, 0.0, 9, 0)
    assert (np.abs(got) <= 1).all() and (got == 1).mean() > 0.3 and (got == -1).mean() > 0.3
    assert np.abs(got.astype(np.float64) - exp).max() <= F32_STEP


def test_beta_zero_gives_independent_steps(host):
    P, K, H = 1, 4096, 3
    mean, std = np.zeros((H, P, 6), np.float32), np.full((H, P, 6), 0.2, np.float32)
    seed, D = MOMENT_SEED, 1
    white = run_sample(host, P, K, H, mean, std, 0.0, seed, D)
    coloured = run_sample(host, P, K, H, mean, std, 0.5, seed, D)
    assert np.array_equal(white[0], coloured[0]) and not np.array_equal(white[1], coloured[1])     # n_0 = e_0 whatever beta is
    # every row is its own e_h: the restatement's n at beta = 0 is e itself
    e = np_noise(K, H, 0.0, seed, D)
    exp = np.clip(np.float64(np.float32(0.2)) * e, -1, 1)
    exp[:, 0] = 0.0
    assert np.abs(white.astype(np.float64) - exp).max() <= F32_STEP
    n = white[:, 1:].astype(np.float64) / 0.2
    for h in (0, 1):
        d0, d1 = n[h] - n[h].mean(axis=0), n[h + 1] - n[h + 1].mean(axis=0)
        corr = (d0 * d1).mean(axis=0) / np.sqrt((d0 * d0).mean(axis=0) * (d1 * d1).mean(axis=0))
        assert np.abs(corr).max() <= 5 / np.sqrt(K - 1), corr


def test_sample_moments(host):
    P, K, H, beta = 1, 4096, 2, 0.9
    mean, std = np.zeros((H, P, 6), np.float32), np.full((H, P, 6), 0.2, np.float32)
    ref = np_noise(K, H, beta, MOMENT_SEED, 0)[:, 1:]
    assert np.abs(ref).max() < 5.0                                          # clipping at 1 / 0.2 = 5 sigma never happens in this draw
    w_ref = moment_checks(ref, beta)                                        # the seed's own NumPy restatement passes
    got = run_sample(host, P, K, H, mean, std, beta, MOMENT_SEED, 0)
    n = got[:, 1:].astype(np.float64) / np.float64(np.float32(0.2))
    w = moment_checks(n, beta)
    print(f"moments over N = {K - 1}: |mean| {w[0]:.4f} (NumPy {w_ref[0]:.4f}, bound {5 / np.sqrt(K - 1):.4f}), |var - 1| {w[1]:.4f} "
          f"({w_ref[1]:.4f}, {5 * np.sqrt(2 / (K - 1)):.4f}), |corr - 0.9| {w[2]:.4f} ({w_ref[2]:.4f}, {5 / np.sqrt(K - 1):.4f})")


@pytest.mark.parametrize("P,K,E", [(3, 70, 7), (2, 300, 300), (1, 1, 1), (2, 257, 64)])
def test_elites_match_stable_argsort(host, P, K, E):
    rng = np.random.default_rng(100 + K)
    ret, failed = make_returns(rng, P, K)
    if K == 1:
        ret[:], failed[:] = 0.5, 0
    got = run_elites(host, P, K, E, ret, failed)
    exp = np_elites(P, K, E, ret, failed)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    if K > 1:
        assert len(np.unique(ret[np.isfinite(ret)])) < np.isfinite(ret).sum()          # the case really has ties
        assert np.isnan(ret).any() and np.isinf(ret).any() and failed.any()


def test_elites_with_few_or_no_admissible_candidates(host):
    P, K, E = 4, 70, 7
    rng = np.random.default_rng(7)
    ret, failed = make_returns(rng, P, K)
    failed[0:K] = 1                                                       # parent 0: every candidate failed
    ret[K:2 * K] = np.nan                                                 # parent 1: every return non-finite ...
    ret[K + 3], failed[K + 3], ret[K + 60], failed[K + 60], ret[K + 61], failed[K + 61] = -1.0, 0, 4.0, 0, 4.0, 0  # ... but three
    ret[2 * K:3 * K], failed[2 * K:3 * K] = 1.5, 0                        # parent 2: all equal -> 0, 1, 2, ...
    ret[3 * K:4 * K] = np.where(np.arange(K) % 2 == 0, np.inf, -np.inf)   # parent 3: infinities only
    got = run_elites(host, P, K, E, ret, failed)
    exp = np_elites(P, K, E, ret, failed)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert got[1].tolist() == [0, 3, 7, 0]
    assert (got[0][0] == -1).all() and got[0][1].tolist() == [60, 61, 3, -1, -1, -1, -1] and got[0][2].tolist() == list(range(7))
    # -0.0 and 0.0 tie
    r2, f2 = np.array([0.0, -0.0, 0.0, 1.0]), np.zeros(4, np.uint8)
    assert run_elites(host, 1, 4, 4, r2, f2)[0].tolist() == [[3, 0, 1, 2]] == np_elites(1, 4, 4, r2, f2)[0].tolist()


def refit_case(rng, P, K, H, E):
    actions = np.clip(rng.normal(0, 0.6, (H, P * K, 6)), -1, 1).astype(np.float32)
    ret, failed = make_returns(rng, P, K)
    elite, n_elite = np_elites(P, K, E, ret, failed)
    mean = rng.uniform(-1, 1, (H, P, 6)).astype(np.float32)
    std = rng.uniform(0.05, 0.6, (H, P, 6)).astype(np.float32)
    return actions, elite, n_elite, mean, std


def run_refit(host, P, K, H, E, actions, elite, n_elite, alpha, min_std, mean, std, in_place=False):
    mo, so = (mean, std) if in_place else (np.full_like(mean, 7), np.full_like(std, 7))
    m, s = np.zeros((H, P, 6)), np.zeros((H, P, 6))
    host.cemhost_refit(P, K, H, E, ptr(actions), ptr(elite), ptr(n_elite), alpha, min_std, ptr(mean), ptr(std), ptr(mo), ptr(so), ptr(m), ptr(s))
    return mo, so, m, s


@pytest.mark.parametrize("P,K,H,E,alpha", [(3, 70, 3, 7, 0.1), (2, 300, 2, 300, 0.5), (1, 1, 1, 1, 0.0), (2, 257, 3, 64, 0.0)])
def test_refit_matches_numpy(host, P, K, H, E, alpha):
    rng = np.random.default_rng(200 + K)
    actions, elite, n_elite, mean, std = refit_case(rng, P, K, H, E)
    if K == 1:
        elite[:], n_elite[:] = 0, 1
    min_std = 0.05
    mo, so, m, s = run_refit(host, P, K, H, E, actions, elite, n_elite, alpha, min_std, mean, std)
    e_mo, e_so, e_m, e_s = np_refit(P, K, H, actions, elite, n_elite, alpha, min_std, mean, std)
    err_m, err_s = np.abs(m - e_m).max(), np.abs(s - e_s).max()
    print(f"refit K={K} E={E}: max |m - NumPy| = {err_m:.2e}, max |s - NumPy| = {err_s:.2e} (bound {E * 2.0 ** -53:.2e})")
    assert err_m <= E * 2.0 ** -53 and err_s <= E * 2.0 ** -53
    assert within_one_f32_ulp(mo, e_mo) and within_one_f32_ulp(so, e_so)
    assert (so >= np.float32(min_std)).all()
    if alpha == 0.0:                                                      # the elites' own moments (std under the floor)
        assert np.array_equal(mo, m.astype(np.float32)) and np.array_equal(so, np.maximum(s, min_std).astype(np.float32))
    # in place equals out of place
    mi, si = mean.copy(), std.copy()
    run_refit(host, P, K, H, E, actions, elite, n_elite, alpha, min_std, mi, si, in_place=True)
    assert np.array_equal(mi, mo) and np.array_equal(si, so)


def test_refit_keeps_parents_without_elites_and_holds_the_floor(host):
    P, K, H, E = 3, 70, 3, 7
    rng = np.random.default_rng(9)
    actions, elite, n_elite, mean, std = refit_case(rng, P, K, H, E)
    elite[1], n_elite[1] = -1, 0                                          # parent 1: no elite
    k0 = elite[2, 0]
    actions[:, 2 * K + elite[2]] = actions[:, 2 * K + k0][:, None, :]     # parent 2: identical elites -> s = 0 exactly -> the floor
    mo, so, m, s = run_refit(host, P, K, H, E, actions, elite, n_elite, 0.0, 0.125, mean, std)
    assert np.array_equal(mo[:, 1], mean[:, 1]) and np.array_equal(so[:, 1], std[:, 1]) and np.isnan(m[:, 1]).all()
    assert (s[:, 2] == 0).all() and (so[:, 2] == np.float32(0.125)).all() and np.array_equal(mo[:, 2], actions[:, 2 * K + k0])
    assert (so[:, [0, 2]] >= np.float32(0.125)).all()
    e_mo, e_so, _, _ = np_refit(P, K, H, actions, elite, n_elite, 0.0, 0.125, mean, std)
    assert within_one_f32_ulp(mo, e_mo) and within_one_f32_ulp(so, e_so)
    # min_std = 0 is allowed: identical elites then give std 0
    so0 = run_refit(host, P, K, H, E, actions, elite, n_elite, 0.0, 0.0, mean, std)[1]
    assert (so0[:, 2] == 0).all()


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """tests/cemhost/cemhost.cpp with its own main, AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (nothing is
    loaded into Python): exactly sized heap buffers at the awkward shapes, so an index past a row end is reported."""
    exe = tmp_path / "cemhost_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DCEMHOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cemhost ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
