"""CPU tests of the CMA-ES stages: csrc/gl_cma.hpp (host instantiation, tests/cmahost/cmahost.cpp -- a lane is a call, the updating
block a loop with the kernel's tiles and owners) against NumPy restatements written from include/glgym.h.

Bounds.
* Philox words: EXACT (test_plan_cem_host / test_plan_es_host check the stream itself; here the rows with chol = I are the CEM host
  build's bit for bit, which carries it over).  Padding slots: exactly 0.
* Sampled theta: within np.spacing(np.float32(1)) = 1.19e-7 absolute of the float64 restatement, test_plan_cem_host's bound for its
  reason: ln / cos / sin of two libms differ by a few double ulps; with sigma <= 1 and rows of chol of norm <= 1 that difference is
  not amplified, and it can move the float32 rounding of a value of magnitude <= 1 by at most one float32 ulp <= 1.19e-7.
* yw, zw, p_sigma', p_c', cov', chol', mean', status: EXACT -- only +, -, *, /, sqrt in a stated order.
* sigma': within 4 * 2^-52 relative -- exp of two libms, at most 1 ulp each, and one product rounding each.
* The loop (rotated quadratic of condition 1e3, N = 6, K = 16, E = 8, 60 generations, Philox noise): the distance of the mean from
  the optimum ends below 0.1 of the initial one.  LOOP_SEED was picked once so that the NumPy restatement itself passes (as in
  test_plan_es_host); with it the restatement ends at 0.0066 of the initial distance, and the same loop with the off-diagonal of C
  zeroed after every generation at 0.178."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_plan_cem_host import F32_STEP, build_host as build_cem_host, np_elites, np_noise, ptr
from test_plan_es_host import np_pow_t

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SRC = ROOT / "tests" / "cmahost" / "cmahost.cpp"
LOOP_SEED = 2026
SIGMA_RTOL = 4 * 2.0 ** -52
UPDATED, FEW_ELITES, NOT_FINITE, NOT_POSITIVE, T_ZERO = 0, 1, 2, 3, 4
GUARD = 8                                                                # sentinel elements in front of and behind every buffer


def build_host(path):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.cmahost_sizeof.argtypes, lib.cmahost_sizeof.restype = [C.c_int], C.c_int
    lib.cmahost_sample.argtypes, lib.cmahost_sample.restype = [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_uint64] * 2 + [C.c_void_p], None
    lib.cmahost_update.argtypes = [C.c_int] * 4 + [C.c_void_p] * 5 + [C.c_uint64] + [C.c_void_p] * 9
    lib.cmahost_update.restype = None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_cma.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    return build_host(tmp_path_factory.mktemp("cmahost") / "libcmahost.so")


# ---- NumPy restatements (from the header's text, not from gl_cma.hpp) ----------------------------------------------------------------
def cma_defaults(N, K, E):
    """Hansen's defaults as RuleSearch.cma_defaults states them (restated here so that this file needs no device)."""
    w = np.log(E + 0.5) - np.log(np.arange(1, E + 1))
    w = w / w.sum()
    mu = 1.0 / float((w * w).sum())
    c_sigma = (mu + 2.0) / (N + mu + 5.0)
    c_1 = 2.0 / ((N + 1.3) ** 2 + mu)
    return dict(w=w, mu_eff=mu, c_sigma=c_sigma, d_sigma=1.0 + 2.0 * max(0.0, np.sqrt((mu - 1.0) / (N + 1.0)) - 1.0) + c_sigma,
                c_c=(4.0 + mu / N) / (N + 4.0 + 2.0 * mu / N), c_1=c_1,
                c_mu=min(1.0 - c_1, 2.0 * (mu - 2.0 + 1.0 / mu) / ((N + 2.0) ** 2 + mu)),
                chi_n=np.sqrt(N) * (1.0 - 1.0 / (4.0 * N) + 1.0 / (21.0 * N * N)))


HYPER = ("mu_eff", "c_sigma", "d_sigma", "c_c", "c_1", "c_mu", "chi_n", "min_sigma", "max_sigma")


def planes(N):
    return (N + 5) // 6


def flat(block, N):
    """[Ht, n, 6] -> [n, N]: component i of row r at [r, i]."""
    return block.transpose(1, 0, 2).reshape(block.shape[1], -1)[:, :N]


def np_cma_sample(P, K, N, mean, sigma, chol, seed, D):
    """theta in float64 BEFORE the cast [Ht, P*K, 6]."""
    Ht = planes(N)
    z = flat(np_noise(P * K, Ht, 0.0, seed, D), N).reshape(P, K, N)
    m = flat(mean.astype(np.float64), N)
    out = np.zeros((P, K, Ht * 6))
    for p in range(P):
        y = np.zeros((K, N))
        for j in range(N):                                               # j ascending: each product rounded, then added
            y[:, j:] = y[:, j:] + chol[p][j:, j][None, :] * z[p][:, j:j + 1]
        out[p, :, :N] = np.clip(m[p][None, :] + sigma[p] * y, -1.0, 1.0)
    return out.reshape(P * K, Ht, 6).transpose(1, 0, 2)


def np_cma_update(P, K, N, E, theta, elite_k, n_elite, hp, t, mean, sigma, cov, chol, p_sigma, p_c):
    """-> the new state (copies; mean as float32, everything else float64), status, yw, zw, h_sigma per row."""
    w = hp["w"]
    mean, sigma, cov, chol, p_sigma, p_c = (a.copy() for a in (mean, sigma, cov, chol, p_sigma, p_c))
    status, yws, zws, hss = np.zeros(P, np.int32), np.full((P, N), np.nan), np.full((P, N), np.nan), np.zeros(P, bool)
    x_all = flat(theta, N).astype(np.float64).reshape(P, K, N)
    m_all = flat(mean, N)                                                # a copy: [P, N] float32
    with np.errstate(all="ignore"):
        for p in range(P):
            el = elite_k[p]
            if t == 0:
                status[p] = T_ZERO
                continue
            if n_elite[p] < E or (el < 0).any() or (el >= K).any():
                status[p] = FEW_ELITES
                continue
            m, s, L = m_all[p].astype(np.float64), float(sigma[p]), chol[p]
            y = (x_all[p][el] - m[None, :]) / s
            yw, R = np.zeros(N), np.zeros((N, N))
            for e in range(E):
                wy = w[e] * y[e]
                yw = yw + wy
                R = R + wy[:, None] * y[e][None, :]
            zw = np.zeros(N)
            for i in range(N):
                acc = yw[i]
                for j in range(i):
                    acc = acc - L[i, j] * zw[j]
                zw[i] = acc / L[i, i]
            yws[p], zws[p] = yw, zw
            cs, cc, c1, cmu, mu = hp["c_sigma"], hp["c_c"], hp["c_1"], hp["c_mu"], hp["mu_eff"]
            ps = (1.0 - cs) * p_sigma[p] + np.sqrt((cs * (2.0 - cs)) * mu) * zw
            n2 = 0.0
            for d in range(N):
                n2 = n2 + ps[d] * ps[d]
            nrm = np.sqrt(n2)
            g = 1.0 - np_pow_t(1.0 - cs, 2 * t)
            hs = bool(nrm / np.sqrt(g) < (1.4 + 2.0 / (N + 1)) * hp["chi_n"])
            hss[p] = hs
            pc = (1.0 - cc) * p_c[p] + (np.sqrt((cc * (2.0 - cc)) * mu) * yw if hs else 0.0)
            a0 = ((1.0 - c1) - cmu) + (0.0 if hs else (c1 * cc) * (2.0 - cc))
            cv = (a0 * cov[p] + c1 * (pc[:, None] * pc[None, :])) + cmu * R
            cv = np.tril(cv) + np.tril(cv, -1).T                          # the upper triangle is a copy of the lower
            mn = np.clip(m + s * yw, -1.0, 1.0).astype(np.float32)
            sg = min(max(s * np.exp((cs / hp["d_sigma"]) * (nrm / hp["chi_n"] - 1.0)), hp["min_sigma"]), hp["max_sigma"])
            if not (np.isfinite(ps).all() and np.isfinite(pc).all() and np.isfinite(cv).all() and np.isfinite(mn).all() and np.isfinite(sg)):
                status[p] = NOT_FINITE
                continue
            Ln, pivots_ok = np.zeros((N, N)), True
            for j in range(N):
                v = cv[j:, j].copy()
                for k in range(j):
                    v = v - Ln[j:, k] * Ln[j, k]
                pivots_ok = pivots_ok and bool(v[0] > 0.0)
                Ln[j, j] = np.sqrt(v[0])
                Ln[j + 1:, j] = v[1:] / Ln[j, j]
            if not pivots_ok:
                status[p] = NOT_POSITIVE
                continue
            if not np.isfinite(Ln).all():
                status[p] = NOT_FINITE
                continue
            m_all[p] = mn
            sigma[p], cov[p], chol[p], p_sigma[p], p_c[p] = sg, cv, Ln, ps, pc
    Ht = planes(N)
    full = np.zeros((P, Ht * 6), np.float32)
    full[:, :N] = m_all
    pad = flat(mean, Ht * 6)[:, N:]
    full[:, N:] = pad                                                    # the padding slots of mean are nobody's: they keep their bits
    return dict(mean=np.ascontiguousarray(full.reshape(P, Ht, 6).transpose(1, 0, 2)), sigma=sigma, cov=cov, chol=chol, p_sigma=p_sigma,
                p_c=p_c, status=status, yw=yws, zw=zws, h_sigma=hss)


# ---- running the host build on guarded buffers ----------------------------------------------------------------------------------------
class Guarded:
    """A host array with GUARD sentinel elements in front and behind."""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        self.raw = np.empty(arr.size + 2 * GUARD, arr.dtype)
        self.raw.view(np.uint8)[:] = 0xA5
        self.a = self.raw[GUARD:GUARD + arr.size].reshape(arr.shape)
        self.a[...] = arr

    def whole(self):
        g = self.raw.view(np.uint8)
        n = GUARD * self.raw.itemsize
        return bool((g[:n] == 0xA5).all() and (g[-n:] == 0xA5).all())


def run_sample(host, P, K, N, mean, sigma, chol, seed, D):
    out = Guarded(np.full((planes(N), P * K, 6), 7, np.float32))
    ins = [Guarded(a) for a in (mean, sigma, chol)]
    host.cmahost_sample(P, K, N, ptr(ins[0].a), ptr(ins[1].a), ptr(ins[2].a), seed, D, ptr(out.a))
    assert out.whole() and all(g.whole() for g in ins)
    return out.a.copy()


STATE = ("mean", "sigma", "cov", "chol", "p_sigma", "p_c")


def run_update(host, P, K, N, E, theta, elite_k, n_elite, hp, t, mean, sigma, cov, chol, p_sigma, p_c):
    g = {k: Guarded(v) for k, v in dict(mean=mean, sigma=sigma, cov=cov, chol=chol, p_sigma=p_sigma, p_c=p_c).items()}
    ro = [Guarded(a) for a in (theta, elite_k, n_elite, hp["w"], np.array([hp[k] for k in HYPER]))]
    out = {k: Guarded(v) for k, v in dict(status=np.full(P, 99, np.int32), yw=np.full((P, N), np.nan), zw=np.full((P, N), np.nan)).items()}
    host.cmahost_update(P, K, N, E, *(ptr(r.a) for r in ro), t, *(ptr(g[k].a) for k in STATE), ptr(out["status"].a), ptr(out["yw"].a),
                        ptr(out["zw"].a))
    assert all(x.whole() for x in list(g.values()) + ro + list(out.values())), "a guard word was written"
    for r, src in zip(ro, (theta, elite_k, n_elite)):
        assert same(r.a, src), "an input was written"
    res = {k: v.a.copy() for k, v in g.items()}
    res.update({k: v.a.copy() for k, v in out.items()})
    return res


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    return a.shape == np.shape(b) and np.array_equal(bits(a), bits(np.ascontiguousarray(b, dtype=a.dtype)))


def check_update(got, exp, before, N):
    """The module's bounds for one update; rows whose status is not 0 keep every bit."""
    assert np.array_equal(got["status"], exp["status"]), (got["status"], exp["status"])
    keep = exp["status"] != UPDATED
    went = np.isin(exp["status"], (UPDATED, NOT_FINITE, NOT_POSITIVE))
    for k in ("yw", "zw"):
        assert same(got[k][went], exp[k][went]), k
    for k in ("cov", "chol", "p_sigma", "p_c", "mean"):
        assert same(got[k], exp[k]), (k, np.abs(got[k].astype(np.float64) - exp[k]).max())
    assert (np.abs(got["sigma"] - exp["sigma"]) <= SIGMA_RTOL * np.abs(exp["sigma"])).all(), (got["sigma"], exp["sigma"])
    for k in ("sigma", "cov", "chol", "p_sigma", "p_c"):
        assert same(got[k][keep], before[k][keep]), k
    assert same(got["mean"][:, keep], before["mean"][:, keep])
    ok = ~keep
    assert same(np.triu(got["chol"][ok], 1), np.zeros_like(got["chol"][ok])) and same(got["cov"][ok], got["cov"][ok].transpose(0, 2, 1))


def make_state(rng, P, N, spread=1.0):
    """A state whose chol has rows of norm <= 1 and whose cov is chol chol^T, symmetric to the bit."""
    L = np.tril(rng.normal(0, 0.3, (P, N, N)))
    i = np.arange(N)
    L[:, i, i] = rng.uniform(0.5, 1.0, (P, N))
    L /= np.maximum(1.0, np.linalg.norm(L, axis=2, keepdims=True))
    L *= spread
    cov = L @ L.transpose(0, 2, 1)
    cov = np.tril(cov) + np.tril(cov, -1).transpose(0, 2, 1)
    mean = np.zeros((planes(N), P, 6), np.float32)
    m = rng.uniform(-0.7, 0.7, (P, N)).astype(np.float32)
    for d in range(N):
        mean[d // 6, :, d % 6] = m[:, d]
    return dict(mean=mean, sigma=rng.uniform(0.05, 1.0, P), cov=cov, chol=L, p_sigma=rng.normal(0, 0.5, (P, N)), p_c=rng.normal(0, 0.5, (P, N)))


def elites_of(rng, P, K, E):
    elite = np.stack([rng.permutation(K)[:E] for _ in range(P)]).astype(np.int32)
    return elite, np.full(P, E, np.int32)


def hyper_of(N, K, E, **over):
    return {**cma_defaults(N, K, E), "min_sigma": 1e-6, "max_sigma": 1.0, **over}


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
def test_args_structs_have_the_headers_sizes(host):
    from gl_gym_amd import _lib as L
    for which, cls in enumerate((L.PlanCmaSampleArgs, L.PlanCmaUpdateArgs)):
        assert C.sizeof(cls) == host.cmahost_sizeof(which), cls.__name__
        assert cls._fields_[0][0] == "struct_size"
    for name in ("glgym_plan_cma_sample", "glgym_plan_cma_update"):
        assert name in L.PROTOTYPES
    assert L.CMA_NMAX == host.cmahost_sizeof(2) == 32


SHAPES = [(1, 2, 1), (3, 6, 5), (2, 66, 6), (3, 258, 7), (2, 6, 29), (1, 66, 32), (2, 258, 32)]


@pytest.mark.parametrize("P,K,N", SHAPES)
def test_sample_matches_numpy(host, P, K, N):
    rng = np.random.default_rng(100 * N + K)
    st = make_state(rng, P, N)
    st["mean"][0, 0, 0] = 1.0                                            # a mean on the box
    seed, D = 0xDEADBEEF12345678, 2 ** 40 + 3
    got = run_sample(host, P, K, N, st["mean"], st["sigma"], st["chol"], seed, D)
    exp = np_cma_sample(P, K, N, st["mean"], st["sigma"], st["chol"], seed, D)
    err = np.abs(got.astype(np.float64) - exp).max()
    print(f"cma sample P={P} K={K} N={N}: max |theta - float64 restatement| = {err:.2e} (bound {F32_STEP:.2e})")
    assert err <= F32_STEP and (np.abs(got) <= 1).all()
    assert same(flat(got, planes(N) * 6)[:, N:], np.zeros((P * K, planes(N) * 6 - N), np.float32))   # padding: +0.0 to the bit
    assert not np.array_equal(run_sample(host, P, K, N, st["mean"], st["sigma"], st["chol"], seed, D + 1), got)
    assert not np.array_equal(run_sample(host, P, K, N, st["mean"], st["sigma"], st["chol"], seed + 1, D), got)
    assert same(run_sample(host, P, K, N, st["mean"], st["sigma"], st["chol"], seed, D), got)
    if N > 1:                                                            # the factor does correlate: another chol, other rows
        assert not np.array_equal(run_sample(host, P, K, N, st["mean"], st["sigma"], np.stack([np.eye(N)] * P), seed, D), got)


@pytest.mark.parametrize("P,K,N", SHAPES)
def test_identity_factor_gives_the_cem_rows(host, tmp_path_factory, P, K, N):
    cem = build_cem_host(tmp_path_factory.mktemp("cemhost_cma") / "libcemhost.so")
    rng = np.random.default_rng(3)
    Ht = planes(N)
    mean = rng.uniform(-1.1, 1.1, (Ht, P, 6)).astype(np.float32)
    sig32 = rng.uniform(0.05, 0.6, P).astype(np.float32)
    std = np.ascontiguousarray(np.broadcast_to(sig32[None, :, None], (Ht, P, 6)))
    seed, D = 0xABCDEF0123, 41
    got = run_sample(host, P, K, N, mean, sig32.astype(np.float64), np.stack([np.eye(N)] * P), seed, D)
    ref = np.full((Ht, P * K, 6), 7, np.float32)
    cem.cemhost_sample(P, K, Ht, ptr(mean), ptr(std), 0.0, seed, D, 0, 0, None, None, None, ptr(ref))
    g, r = flat(got, N).reshape(P, K, N), flat(ref, N).reshape(P, K, N)
    assert same(g[:, 1:], r[:, 1:])                                      # k = 0 is the CEM's reserved mean
    assert not np.array_equal(g[:, 0], r[:, 0])


UPDATE_CASES = [(1, 2, 1, 1), (5, 6, 3, 2), (6, 66, 33, 1000), (7, 258, 258, 1), (29, 66, 2, 2), (32, 258, 129, 1000), (6, 6, 6, 1),
                (32, 66, 1, 2), (5, 258, 1, 1)]


@pytest.mark.parametrize("N,K,E,t", UPDATE_CASES)
def test_update_matches_numpy_exactly(host, N, K, E, t):
    P = 3
    rng = np.random.default_rng(1000 * N + K + E)
    st = make_state(rng, P, N)
    hp = hyper_of(N, K, E)
    theta = run_sample(host, P, K, N, st["mean"], st["sigma"], st["chol"], 77, 3)
    elite, n_elite = elites_of(rng, P, K, E)
    got = run_update(host, P, K, N, E, theta, elite, n_elite, hp, t, **st)
    exp = np_cma_update(P, K, N, E, theta, elite, n_elite, hp, t, **st)
    check_update(got, exp, st, N)
    assert (exp["status"] == UPDATED).all() and not same(got["mean"], st["mean"]) and not same(got["cov"], st["cov"])
    print(f"cma update N={N} K={K} E={E} t={t}: h_sigma {exp['h_sigma'].tolist()}, "
          f"max rel |sigma' - NumPy| = {(np.abs(got['sigma'] - exp['sigma']) / exp['sigma']).max():.2e}")


def test_h_sigma_false_and_a_population_on_the_bound(host):
    P, K, N, E = 3, 66, 7, 33
    rng = np.random.default_rng(5)
    st = make_state(rng, P, N)
    st["p_sigma"][0] = 50.0                                              # row 0: a long path -> h_sigma false
    st["mean"][0, 1, 2], st["mean"][1, 1, 0] = 1.0, -1.0                 # row 1: a mean on +1 and on -1
    hp = hyper_of(N, K, E)
    theta = run_sample(host, P, K, N, st["mean"], st["sigma"], st["chol"], 1, 2)
    theta[0, 2 * K:3 * K, 3] = 1.0                                        # row 2: the whole population on a bound in component 3
    st["mean"][0, 2, 3] = 1.0
    elite, n_elite = elites_of(rng, P, K, E)
    got = run_update(host, P, K, N, E, theta, elite, n_elite, hp, 5, **st)
    exp = np_cma_update(P, K, N, E, theta, elite, n_elite, hp, 5, **st)
    check_update(got, exp, st, N)
    assert exp["h_sigma"].tolist() == [False, True, True] and (exp["status"] == UPDATED).all()
    assert got["yw"][2, 3] == 0.0 and got["mean"][0, 2, 3] == 1.0
    assert (np.abs(got["mean"]) <= 1).all()


def test_rows_that_are_not_updated_keep_every_bit(host):
    P, K, N, E = 7, 66, 7, 33
    rng = np.random.default_rng(6)
    st = make_state(rng, P, N)
    hp = hyper_of(N, K, E)
    theta = run_sample(host, P, K, N, st["mean"], st["sigma"], st["chol"], 1, 2)
    elite, n_elite = elites_of(rng, P, K, E)
    n_elite[0] = E - 1                                                    # 1: too few elites
    elite[1, 5] = -1                                                      # 1: an index of -1
    elite[2, E - 1] = K                                                   # 1: an index of K
    theta[1, 3 * K + elite[3, 4], 0] = np.nan                             # 2: a NaN in an elite's theta (component 6)
    st["cov"][4] = -np.eye(N)                                             # 3: a cov made indefinite by hand
    st["cov"][5][2, 2] = -50.0                                            # 3: ... in one pivot only
    got = run_update(host, P, K, N, E, theta, elite, n_elite, hp, 3, **st)
    exp = np_cma_update(P, K, N, E, theta, elite, n_elite, hp, 3, **st)
    assert exp["status"].tolist() == [FEW_ELITES, FEW_ELITES, FEW_ELITES, NOT_FINITE, NOT_POSITIVE, NOT_POSITIVE, UPDATED]
    check_update(got, exp, st, N)
    got0 = run_update(host, P, K, N, E, theta, elite, n_elite, hp, 0, **st)
    assert got0["status"].tolist() == [T_ZERO] * P                       # 4: t = 0, every row
    check_update(got0, np_cma_update(P, K, N, E, theta, elite, n_elite, hp, 0, **st), st, N)


def quadratic(N, seed=12):
    """f(x) = (x - x*)^T Q^T diag(lambda) Q (x - x*) with condition 1e3 and the optimum inside the box."""
    rng = np.random.default_rng(seed)
    Q = np.linalg.qr(rng.normal(size=(N, N)))[0]
    A = Q.T @ np.diag(np.logspace(0, 3, N)) @ Q
    return A, rng.uniform(-0.6, 0.6, N)


def cma_loop(N, K, E, n_iter, hp, sample, update, diagonal=False):
    P = 1
    A, target = quadratic(N)
    st = dict(mean=np.zeros((planes(N), P, 6), np.float32), sigma=np.full(P, 0.3), cov=np.eye(N)[None].copy(), chol=np.eye(N)[None].copy(),
              p_sigma=np.zeros((P, N)), p_c=np.zeros((P, N)))
    for it in range(n_iter):
        theta = sample(st, it)
        d = flat(theta, N).astype(np.float64) - target
        ret = -np.einsum("ka,ab,kb->k", d, A, d)
        elite, n_elite = np_elites(P, K, E, ret, np.zeros(K, np.uint8))
        st = update(theta, elite, n_elite, it + 1, st)
        if diagonal:
            dg = np.diagonal(st["cov"], axis1=1, axis2=2)
            st["cov"] = np.stack([np.diag(v) for v in dg])
            st["chol"] = np.stack([np.diag(np.sqrt(v)) for v in dg])
    return np.linalg.norm(flat(st["mean"], N)[0] - target) / np.linalg.norm(target)


def test_the_loop_converges_on_an_ill_conditioned_quadratic(host):
    """The setting and the bars of the module docstring.  The host build's stages are fed the restatement's state at every generation
    and meet the per-stage bounds there; the restatement, the yardstick, meets the bar of 0.1, and the loop without the off-diagonal
    of C ends above it."""
    N, K, E, n_iter = 6, 16, 8, 60
    hp = hyper_of(N, K, E)

    def np_sample(st, it):
        return np_cma_sample(1, K, N, st["mean"], st["sigma"], st["chol"], LOOP_SEED, it).astype(np.float32)

    def np_update(theta, elite, n_elite, t, st):
        out = np_cma_update(1, K, N, E, theta, elite, n_elite, hp, t, **st)
        assert out["status"].tolist() == [UPDATED]
        return {k: out[k] for k in STATE}

    def checked_sample(st, it):
        ref = np_cma_sample(1, K, N, st["mean"], st["sigma"], st["chol"], LOOP_SEED, it)
        got = run_sample(host, 1, K, N, st["mean"], st["sigma"], st["chol"], LOOP_SEED, it)
        assert np.abs(got.astype(np.float64) - ref).max() <= F32_STEP
        return ref.astype(np.float32)

    def checked_update(theta, elite, n_elite, t, st):
        exp = np_cma_update(1, K, N, E, theta, elite, n_elite, hp, t, **st)
        check_update(run_update(host, 1, K, N, E, theta, elite, n_elite, hp, t, **st), exp, st, N)
        assert exp["status"].tolist() == [UPDATED]
        return {k: exp[k] for k in STATE}

    full = cma_loop(N, K, E, n_iter, hp, np_sample, np_update)
    diag = cma_loop(N, K, E, n_iter, hp, np_sample, np_update, diagonal=True)
    fed = cma_loop(N, K, E, n_iter, hp, checked_sample, checked_update)
    print(f"cma loop: distance / initial distance = {full:.4f} (full), {diag:.4f} (off-diagonal zeroed), {fed:.4f} (host build checked)")
    assert full < 0.1 and fed == full
    assert diag > full


# ---- argument checking through libglgym.so: no device is needed, the refusals come before the handle is looked at ------------------
@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    from gl_gym_amd import _lib as L
    if not L.LIB_PATH.exists():
        g.build()
    return L, L.load()


P_ = 0x1000                                                              # a non-null pointer: never followed


def refused(lib, fn, a, word):
    from gl_gym_amd import _lib as L
    assert fn(None, C.byref(a), None) == L.EINVAL, word
    msg = lib.glgym_last_error()
    assert msg and word in msg, (word, msg)


SHAPE_REFUSALS = (("struct_size", 8, b"struct_size"), ("P", 0, b"P or K < 1"), ("K", 0, b"P or K < 1"), ("N", 0, b"N outside"),
                  ("N", 33, b"N outside"), ("N", -1, b"N outside"), ("P", 2 ** 30, b"past INT32_MAX"))


def test_cma_sample_refusals(capi):
    L, lib = capi
    good = lambda: L.make_plan_args(L.PlanCmaSampleArgs, 3, 8, 5, P_, P_, P_, 1, 2, None, P_)  # noqa: E731
    refused(lib, lib.glgym_plan_cma_sample, good(), b"glgym_plan_cma_sample: null handle")
    for field, value, word in SHAPE_REFUSALS + tuple((f, None, b"null mean") for f in ("mean", "sigma", "chol", "theta")):
        a = good()
        setattr(a, field, value)
        refused(lib, lib.glgym_plan_cma_sample, a, word)
        assert b"glgym_plan_cma_sample" in lib.glgym_last_error()
    a = good()
    a.N, a.K, a.draw_base = 32, 1, P_                                    # the edges that are allowed
    refused(lib, lib.glgym_plan_cma_sample, a, b"null handle")
    assert lib.glgym_plan_cma_sample(None, None, None) == L.EINVAL


def test_cma_update_refusals(capi):
    L, lib = capi
    nan, inf = float("nan"), float("inf")
    hp = hyper_of(5, 8, 4)
    w = np.ascontiguousarray(hp["w"])                                    # the weights are read on the host: a real array

    def good():
        return L.make_plan_args(L.PlanCmaUpdateArgs, 3, 8, 5, 4, P_, P_, P_, w.ctypes.data, P_, *(hp[k] for k in HYPER), 1, None,
                                P_, P_, P_, P_, P_, P_, P_)

    refused(lib, lib.glgym_plan_cma_update, good(), b"glgym_plan_cma_update: null handle")
    cases = SHAPE_REFUSALS + (("E", 0, b"E outside 1..K"), ("E", 9, b"E outside 1..K"), ("t_index", 0, b"t_index = 0"),
                              ("c_sigma", -0.1, b"c_sigma outside"), ("c_sigma", 1.1, b"c_sigma outside"), ("c_c", -0.1, b"c_c outside"),
                              ("c_c", 1.5, b"c_c outside"), ("c_1", -0.1, b"c_1 outside"), ("c_1", 1.5, b"c_1 outside"),
                              ("c_mu", -0.1, b"c_mu outside"), ("c_mu", 1.5, b"c_mu outside"), ("c_mu", 0.999, b"c_1 + c_mu > 1"),
                              ("d_sigma", 0.0, b"d_sigma not > 0"), ("d_sigma", -1.0, b"d_sigma not > 0"), ("chi_n", 0.0, b"chi_n not > 0"),
                              ("mu_eff", 0.0, b"mu_eff not > 0"), ("mu_eff", -2.0, b"mu_eff not > 0"), ("min_sigma", -1e-3, b"min_sigma negative"),
                              ("min_sigma", 2.0, b"> max_sigma"), ("max_sigma", 1e-9, b"> max_sigma"))
    cases += tuple((k, v, k.encode() + b" is not finite") for k in HYPER for v in (nan, inf, -inf))
    cases += tuple((f, None, b"null theta") for f in ("theta", "elite_k", "n_elite", "w", "w_dev", "mean", "sigma", "cov", "chol", "p_sigma",
                                                       "p_c", "status"))
    for field, value, word in cases:
        a = good()
        setattr(a, field, value)
        refused(lib, lib.glgym_plan_cma_update, a, word)
        assert b"glgym_plan_cma_update" in lib.glgym_last_error()
    for value, word in ((-1e-9, b"weight 2 is negative"), (nan, b"weight 2 is not finite"), (inf, b"weight 2 is not finite")):
        w[2] = value
        refused(lib, lib.glgym_plan_cma_update, good(), word)
        w[2] = hp["w"][2]
    a = good()                                                           # the edges that are allowed
    a.c_sigma, a.c_c, a.c_1, a.c_mu, a.min_sigma, a.max_sigma, a.t_base, a.E, a.N = 1.0, 0.0, 0.0, 1.0, 0.5, 0.5, P_, 1, 32
    refused(lib, lib.glgym_plan_cma_update, a, b"null handle")
    assert lib.glgym_plan_cma_update(None, None, None) == L.EINVAL


def test_defaults_are_the_restatement_here():
    """RuleSearch.cma_defaults (a static method: no device) against this file's restatement of the formulas of the issue."""
    from gl_gym_amd.planner import RuleSearch
    for N, K, E in ((1, 2, 1), (5, 16, 8), (29, 64, 32), (32, 258, 129)):
        got, exp = RuleSearch.cma_defaults(N, K, E), cma_defaults(N, K, E)
        assert set(got) == set(exp)
        for k in exp:
            assert np.allclose(got[k], exp[k], rtol=1e-14, atol=0), k
        assert abs(got["w"].sum() - 1) < 1e-15 and (np.diff(got["w"]) < 0).all() and 0 <= got["c_1"] + got["c_mu"] <= 1


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """tests/cmahost/cmahost.cpp with its own main, AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (nothing is
    loaded into Python): exactly sized heap buffers at the awkward shapes, so an index past a row end is reported."""
    exe = tmp_path / "cmahost_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DCMAHOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cmahost ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
