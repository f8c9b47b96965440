"""CPU tests of rollout collection: csrc/gl_actor.hpp (host instantiation, tests/achost/achost.cpp -- a lane is a pass of a loop) against
NumPy restatements written from the text of include/glgym.h; the refusals of glgym_ac_rows / glgym_gae through libglgym.so (no device:
every check precedes the handle).  The helpers below are also what tests/test_gpu_collect.py compares the kernels with.

Bounds.
* the sample, the log-probability and GAE: EXACT (uint32 view).  Every step is a single correctly rounded float32 operation in a fixed
  order, which NumPy performs in the same order.
* eps: within one float32 ulp of the float64 Box-Muller restatement (the host's libm and NumPy's differ in the last bits of a double).
* GAE against float64: one step of adv_t = delta_t + c_t adv_(t+1), c_t = gamma lambda nnt <= 1, is seven float32 operations (two
  products and two sums for delta, two products and one sum for adv), each with a relative error of at most u on an intermediate no
  larger than A = max |r| + 2 max |v| + max |adv|; casting gamma and lambda and rounding their product perturbs the two coefficients
  by at most 3 u relative, again on terms no larger than A.  A step therefore adds at most (7 + 3) u A to the error it inherits
  (times c_t <= 1), and after T steps |adv32 - adv64| <= 11 T u A, the eleventh u covering the second-order terms (gae_bound); returns
  has one more sum: + 2 u |returns|."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_plan_cem_host import KEY_TAG as CEM_TAG, moment_checks, np_philox, within_one_f32_ulp

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SRC = ROOT / "tests" / "achost" / "achost.cpp"
NU = 6
AC_TAG = 0x41435431
M32 = 0xFFFFFFFF
HALF_LOG_2PI = np.float32(0.9189385)
IN_DIMS = [1, 23, 64, 65, 130]
SENTINEL = np.float32(7.25)
GUARD = 3                                                     # sentinel rows behind row B-1 of every output
U = 2.0 ** -24


def build_host(path):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.achost_sizeof.argtypes, lib.achost_sizeof.restype = [C.c_int], C.c_int
    lib.achost_key_tag.argtypes, lib.achost_key_tag.restype = [], C.c_uint
    lib.achost_noise.argtypes, lib.achost_noise.restype = [C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_void_p], None
    lib.achost_rows.argtypes, lib.achost_rows.restype = [C.c_void_p], None
    lib.achost_gae.argtypes, lib.achost_gae.restype = [C.c_void_p], None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_actor.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    return build_host(tmp_path_factory.mktemp("achost") / "libachost.so")


def same_u32(a, b):
    """Bit for bit; a NaN equals a NaN (which payload an operation hands on is the processor's business, not the arithmetic's)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a.view(np.uint32)[ok], b.view(np.uint32)[ok])


# ---- noise, sample, GAE: the restatements ------------------------------------------------------------------------------------------------
def np_eps64(B, step, D, seed, tag=AC_TAG):
    """e [B, 6] in float64: counter (b, 2 step + blk, lo32(D), hi32(D)), key (lo32(seed), hi32(seed) ^ tag), Box-Muller on r0..r5."""
    b = np.arange(B, dtype=np.uint64)
    r = np.concatenate([np_philox(b, 2 * step + blk, D & M32, D >> 32, seed & M32, ((seed >> 32) ^ tag) & M32) for blk in (0, 1)], axis=-1)
    u = (r.astype(np.float64) + 0.5) * 2.0 ** -32
    e = np.empty((B, NU))
    for m in range(3):
        rad, ang = np.sqrt(-2.0 * np.log(u[:, 2 * m])), 2.0 * np.pi * u[:, 2 * m + 1]
        e[:, 2 * m], e[:, 2 * m + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return e


def np_sample(mean, std, log_std, eps):
    """-> action, action_env [B, 6], logp [B], float32, every operation on its own."""
    f = np.float32
    mean, std, log_std, eps = (np.asarray(v, dtype=f) for v in (mean, std, log_std, eps))
    with np.errstate(all="ignore"):
        a = mean + std * eps
        env = np.fmin(np.fmax(a, f(-1)), f(1))
        s = np.zeros(len(mean), dtype=f)
        for j in range(NU):
            s = s + (((f(-0.5) * eps[:, j]) * eps[:, j] - log_std[j]) - HALF_LOG_2PI)
    return a.astype(f), env.astype(f), s.astype(f)


def np_gae(reward, done, value, last_value, gamma, lam, T=np.float32):
    """advantage, returns [T, B] in dtype T by the header's text (float32: exact restatement; float64: SB3's formula as truth)."""
    r, v, last = reward.astype(T), value.astype(T), last_value.astype(T)
    g, lm = T(np.float32(gamma)) if T is np.float32 else T(gamma), T(np.float32(lam)) if T is np.float32 else T(lam)
    gl = g * lm
    n_t = len(r)
    adv, ret = np.empty_like(r), np.empty_like(r)
    run = np.zeros(r.shape[1], dtype=T)
    with np.errstate(all="ignore"):
        for t in range(n_t - 1, -1, -1):
            nnt = T(1) - (done[t] != 0).astype(T)
            nv = last if t == n_t - 1 else v[t + 1]
            delta = (r[t] + (g * nv) * nnt) - v[t]
            run = delta + (gl * nnt) * run
            adv[t] = run
            ret[t] = run + v[t]
    return adv, ret


def gae_bound(reward, value, last_value, adv64):
    n_t = len(reward)
    A = np.abs(reward).max() + 2 * max(np.abs(value).max(), np.abs(last_value).max()) + np.abs(adv64).max()
    return 11 * n_t * U * A


def make_gae_case(T, B, pattern, seed=0):
    rng = np.random.default_rng([seed, T, B])
    reward = rng.normal(size=(T, B)).astype(np.float32)
    value = rng.normal(size=(T, B)).astype(np.float32) * 3
    last = rng.normal(size=B).astype(np.float32) * 3
    done = np.zeros((T, B), dtype=np.uint8)
    if pattern == "first":
        done[0] = 1
    elif pattern == "last":
        done[T - 1] = 1
    elif pattern == "all":
        done[:] = 1
    elif pattern == "random":
        done[:] = rng.random((T, B)) < 0.3
        done[done != 0] = rng.integers(1, 256, int((done != 0).sum()))       # any non-zero byte is a done
    else:
        assert pattern == "none"
    return reward, done, value, last


def guarded(shape, dtype=np.float32):
    """An output array with GUARD sentinel rows behind the last one, all sentinel to begin with."""
    return np.full((shape[0] + GUARD,) + tuple(shape[1:]), SENTINEL, dtype=dtype)


def gae_args(T, B, reward, done, value, last, gamma, lam, adv, ret):
    from gl_gym_amd import _lib as L
    p = lambda v: v if isinstance(v, int) or v is None else v.ctypes.data  # noqa: E731
    return L.make_plan_args(L.GaeArgs, T, B, p(reward), p(done), p(value), p(last), gamma, lam, p(adv), p(ret))


def host_gae(host, reward, done, value, last, gamma, lam):
    T, B = reward.shape
    # [T][B] blocks with a guard behind the last row (t = T); no guard column, the rows are contiguous
    adv, ret = guarded((T, B)), guarded((T, B))
    a = gae_args(T, B, reward, done, value, last, gamma, lam, adv, ret)
    host.achost_gae(C.addressof(a))
    assert (adv[T:] == SENTINEL).all() and (ret[T:] == SENTINEL).all()
    return adv[:T], ret[:T]


# ---- a whole glgym_ac_rows call ------------------------------------------------------------------------------------------------------
class AcCase:
    """Inputs of one call in NumPy: obs [B, in_dim], the heads' outputs mean_in [B, 6] and value_in [B], log_std / std."""

    def __init__(self, in_dim, B, seed=0):
        rng = np.random.default_rng([seed, B, in_dim, 99])
        self.B, self.in_dim = B, in_dim
        self.obs = rng.uniform(-2.0, 2.0, (B, in_dim)).astype(np.float32)
        self.log_std = rng.uniform(-1.0, 0.5, NU).astype(np.float32)
        self.std = np.exp(self.log_std).astype(np.float32)
        self.mean_in = rng.normal(size=(B, NU)).astype(np.float32)
        self.value_in = rng.normal(size=B).astype(np.float32)


def ac_args(case, ptr, out, step=0, seed=1, draw_index=0, draw_base=None, deterministic=0, value_only=0, want_obs_out=True, want_eps=True):
    """The glgym_ac_rows_args of `case`.  ptr(name) -> the address of the input array `name` (host or device copies of the case's
    arrays), out: {name: address} of the outputs."""
    from gl_gym_amd import _lib as L
    return L.make_plan_args(L.AcRowsArgs, case.B, case.in_dim, step, deterministic, value_only, ptr("mean_in"), ptr("value_in"), ptr("log_std"),
                            ptr("std"), seed, draw_index, draw_base, ptr("obs"), out["obs_out"] if want_obs_out else None, out["action"],
                            out["action_env"], out["eps"] if want_eps else None, out["logp"], out["value"])


def case_arrays(case):
    return dict(obs=case.obs, log_std=case.log_std, std=case.std, mean_in=case.mean_in, value_in=case.value_in)


def output_shapes(case):
    B = case.B
    return dict(obs_out=(B, case.in_dim), action=(B, NU), action_env=(B, NU), eps=(B, NU), logp=(B,), value=(B,))


def host_rows(host, case, draw_base=None, **kw):
    """achost_rows on the case -> {name: array with its GUARD rows}."""
    arrays = case_arrays(case)
    outs = {k: guarded(s) for k, s in output_shapes(case).items()}
    base = None if draw_base is None else np.array([draw_base], dtype=np.uint64)
    a = ac_args(case, lambda k: arrays[k].ctypes.data, {k: v.ctypes.data for k, v in outs.items()},
                draw_base=None if base is None else base.ctypes.data, **kw)
    host.achost_rows(C.addressof(a))
    return outs


def np_rows(case, eps, deterministic=0):
    """The outputs of a call from the restatements, given its eps [B, 6] float32 (ignored with deterministic)."""
    e = np.zeros((case.B, NU), dtype=np.float32) if deterministic else eps
    action, env, logp = np_sample(case.mean_in, case.std, case.log_std, e)
    return dict(obs_out=case.obs, action=action, action_env=env, eps=e, logp=logp, value=case.value_in)


def check_outputs(got, want, B, written):
    """got: guarded outputs; every name in `written` equals want bit for bit in rows < B, everything else is sentinel."""
    for k, v in got.items():
        if k in written:
            assert same_u32(v[:B], want[k]), (k, np.abs(v[:B] - want[k]).max())
            assert (v[B:] == SENTINEL).all(), k
        else:
            assert (v == SENTINEL).all(), k


ALL_OUT = ("obs_out", "action", "action_env", "eps", "logp", "value")


# ---- 0. the feature is there ----------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_bound_and_declared(host):
    from gl_gym_amd import _lib as L
    header = (ROOT / "include" / "glgym.h").read_text()
    for name in ("glgym_ac_rows", "glgym_gae"):
        assert name in L.PROTOTYPES and f"int {name}(glgym_handle h" in header
    assert "#define GLGYM_ABI_VERSION 7" in header and L.ABI_VERSION == 7
    assert [host.achost_sizeof(i) for i in range(2)] == [C.sizeof(L.AcRowsArgs), C.sizeof(L.GaeArgs)]
    assert host.achost_key_tag() == AC_TAG == L.AC_KEY_TAG and "0x41435431" in header
    import gl_gym_amd
    assert {"TorchHeads", "RolloutCollector"} <= set(gl_gym_amd.__all__)


# ---- 1. noise -----------------------------------------------------------------------------------------------------------------------------
def host_eps(host, B, step, D, seed):
    e = np.full((B, NU), np.nan, dtype=np.float32)
    host.achost_noise(B, step, D, seed, e.ctypes.data)
    return e


def test_eps_matches_the_float64_box_muller(host):
    for step, D, seed in ((0, 0, 0), (5, 3, 1), (63, 2 ** 40 + 17, 0xFEDCBA9876543210), (2 ** 30, 2 ** 64 - 1, 2 ** 64 - 1)):
        got = host_eps(host, 130, step, D, seed)
        assert within_one_f32_ulp(got, np_eps64(130, step, D, seed)), (step, D, seed)
        assert same_u32(got[:64], host_eps(host, 64, step, D, seed))                # env b's noise does not depend on B


def test_step_draw_and_seed_each_change_the_draw_and_the_tag_separates_the_stream(host):
    ref = host_eps(host, 64, 3, 10, 7)
    for step, D, seed in ((4, 10, 7), (3, 11, 7), (3, 10, 8), (3, 10, 7 + 2 ** 32), (3, 10 + 2 ** 32, 7)):
        other = host_eps(host, 64, step, D, seed)
        assert not (other == ref).any(), (step, D, seed)
    # consecutive steps do not share a Philox block: step s uses counters 2s and 2s + 1
    assert not (host_eps(host, 64, 4, 10, 7)[:, :4] == ref[:, 4:6].repeat(2, axis=1)).any()
    cem = np_eps64(64, 3, 10, 7, tag=CEM_TAG).astype(np.float32)                     # glgym_plan_sample's stream at the same counter
    assert AC_TAG != CEM_TAG and not (cem == ref).any()
    assert within_one_f32_ulp(ref, np_eps64(64, 3, 10, 7))


def test_eps_moments(host):
    N = 65536
    n = np.stack([host_eps(host, N, s, 1, 2026) for s in (0, 1)]).astype(np.float64)       # [2, N, 6]: two consecutive steps
    worst = moment_checks(n, 0.0)
    print("mean, variance, step-to-step correlation: worst deviations", worst)


# ---- 2. the whole stage -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim", IN_DIMS)
def test_rows_match_numpy(host, in_dim):
    case = AcCase(in_dim, 67)
    kw = dict(step=4, seed=0xABCDEF0123, draw_index=5, draw_base=9)
    got = host_rows(host, case, **kw)
    eps = got["eps"][:case.B]
    assert within_one_f32_ulp(eps, np_eps64(case.B, 4, 14, 0xABCDEF0123))             # D = draw_index + *draw_base
    check_outputs(got, np_rows(case, eps), case.B, ALL_OUT)
    assert (np.abs(got["action"][:case.B]) > 1).any() and (np.abs(got["action_env"][:case.B]) <= 1).all()       # the clip is at work
    # optional outputs not asked for are not written; the others do not change
    lean = host_rows(host, case, want_obs_out=False, want_eps=False, **kw)
    check_outputs(lean, np_rows(case, eps), case.B, ("action", "action_env", "logp", "value"))
    # deterministic: no noise; value_only: the value alone
    check_outputs(host_rows(host, case, deterministic=1, **kw), np_rows(case, None, deterministic=1), case.B, ALL_OUT)
    check_outputs(host_rows(host, case, value_only=1, **kw), np_rows(case, eps), case.B, ("value",))


def test_nan_means_never_reach_the_env(host):
    case = AcCase(23, 9)
    case.mean_in[::2] = np.nan
    got = host_rows(host, case)
    assert np.isnan(got["action"][:9:2]).all() and (got["action_env"][:9:2] == -1).all() and np.isfinite(got["action"][1:9:2]).all()
    check_outputs(got, np_rows(case, got["eps"][:9]), 9, ALL_OUT)


def test_deterministic_action_is_the_mean_and_zero_std_gives_it_too(host):
    case = AcCase(23, 11)
    det = host_rows(host, case, deterministic=1)
    assert same_u32(det["action"][:11], case.mean_in + np.float32(0))
    case.std = np.zeros(NU, dtype=np.float32)                                        # a stochastic call with std = 0: a = mean + 0 * e
    assert same_u32(host_rows(host, case)["action"][:11], det["action"][:11])


# ---- 3. GAE -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["first", "last", "all", "none", "random"])
@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_gae_matches_numpy_and_the_float64_formula(host, T, B, pattern):
    reward, done, value, last = make_gae_case(T, B, pattern)
    for gamma, lam in ((0.99, 0.95), (0.9631, 0.95), (1.0, 1.0), (0.0, 0.5), (0.7, 0.0)):
        adv, ret = host_gae(host, reward, done, value, last, gamma, lam)
        adv32, ret32 = np_gae(reward, done, value, last, gamma, lam)
        assert same_u32(adv, adv32) and same_u32(ret, ret32), (gamma, lam)
        adv64, ret64 = np_gae(reward, done, value, last, gamma, lam, np.float64)
        bound = gae_bound(reward, value, last, adv64)
        assert np.abs(adv - adv64).max() <= bound and np.abs(ret - ret64).max() <= bound + 2 * U * np.abs(ret64).max() and bound < 1e-3
    if pattern == "all":                                                            # every step ends an episode: adv = r - v
        assert same_u32(adv, reward - value)


def test_gae_is_sb3s_recurrence(host):
    """stable_baselines3's RolloutBuffer.compute_returns_and_advantage, written out in float64 with episode_starts: the host build is
    within gae_bound of it, and the float64 helper the other tests take as truth IS it."""
    reward, done, value, last = make_gae_case(5, 7, "random", seed=3)
    starts = np.concatenate([np.zeros((1, 7)), (done[:-1] != 0).astype(np.float64)])           # episode_starts[t+1] == done[t]
    dones_last = (done[-1] != 0).astype(np.float64)
    r, v = reward.astype(np.float64), value.astype(np.float64)
    last_gae, adv = 0.0, np.zeros((5, 7))
    for step in reversed(range(5)):
        if step == 4:
            next_non_terminal, next_values = 1.0 - dones_last, last.astype(np.float64)
        else:
            next_non_terminal, next_values = 1.0 - starts[step + 1], v[step + 1]
        delta = r[step] + 0.99 * next_values * next_non_terminal - v[step]
        last_gae = delta + 0.99 * 0.95 * next_non_terminal * last_gae
        adv[step] = last_gae
    got_adv, got_ret = host_gae(host, reward, done, value, last, 0.99, 0.95)
    bound = gae_bound(reward, value, last, adv)
    assert np.abs(got_adv - adv).max() <= bound and np.abs(got_ret - (adv + v)).max() <= bound + 2 * U * np.abs(adv + v).max()
    assert np.abs(got_adv - adv).max() > 0                                          # float32 against float64: not vacuous
    a64, r64 = np_gae(reward, done, value, last, 0.99, 0.95, np.float64)
    assert np.array_equal(a64, adv) and np.array_equal(r64, adv + v)


# ---- 4. refusals without a device ---------------------------------------------------------------------------------------------------
P_ = 0x10000                                                  # a non-null pointer: never followed, nothing is launched


def good_ac_args():
    from gl_gym_amd import _lib as L
    M = 0x100000
    return L.make_plan_args(L.AcRowsArgs, 130, 23, 3, 0, 0, P_, P_ + M, P_ + 2 * M, P_ + 3 * M, 1, 0, None, P_ + 4 * M, P_ + 5 * M, P_ + 6 * M,
                            P_ + 7 * M, P_ + 8 * M, P_ + 9 * M, P_ + 10 * M)


def good_gae_args():
    from gl_gym_amd import _lib as L
    M = 0x100000                                              # 5 x 65 x 4 bytes fit many times between two of these
    return L.make_plan_args(L.GaeArgs, 5, 65, P_, P_ + M, P_ + 2 * M, P_ + 3 * M, 0.99, 0.95, P_ + 4 * M, P_ + 5 * M)


from test_plan_policy_host import NET_REFUSALS, set_path  # noqa: E402

from test_plan_policy_host import set_path  # noqa: E402

AC_REFUSALS = [("struct_size", 8, b"struct_size"), ("B", 0, b"B < 1"), ("B", -5, b"B < 1"), ("B", 2 ** 31 - 255, b"2^31 - 256 rows"),
               ("step", -1, b"step < 0"), ("deterministic", 2, b"must be 0 or 1"), ("value_only", -1, b"must be 0 or 1"),
               ("value_in", None, b"null value_in"), ("value", None, b"null value_in"), ("mean_in", None, b"null mean_in"),
               ("log_std", None, b"null mean_in"), ("std", None, b"null mean_in"), ("action", None, b"null mean_in"),
               ("action_env", None, b"null mean_in"), ("logp", None, b"null mean_in"), ("in_dim", 0, b"in_dim outside"),
               ("in_dim", 1025, b"in_dim outside"), ("obs", None, b"null obs"), ("obs_out", P_ + 0x400000, b"obs_out == obs"),
               ("obs_out", P_ + 0x400000 + 130 * 23 * 4 - 4, b"obs_out == obs")]
GAE_REFUSALS = [("struct_size", 4, b"struct_size"), ("T", 0, b"T < 1"), ("B", 0, b"B < 1"), ("gamma", -0.1, b"gamma"), ("gamma", 1.5, b"gamma"),
                ("gamma", float("nan"), b"gamma"), ("gamma", float("inf"), b"gamma"), ("lambda_", -0.1, b"lambda"), ("lambda_", 1.01, b"lambda"),
                ("lambda_", float("nan"), b"lambda"), ("reward", None, b"null reward"), ("done", None, b"null reward"),
                ("value", None, b"null reward"), ("last_value", None, b"null reward"), ("advantage", None, b"null reward"),
                ("returns", None, b"null reward"), ("advantage", P_, b"overlaps an input"), ("returns", P_ + 0x100000, b"overlaps an input"),
                ("advantage", P_ + 2 * 0x100000 + 5 * 65 * 4 - 4, b"overlaps an input"), ("returns", P_ + 3 * 0x100000, b"overlaps an input"),
                ("returns", P_ + 4 * 0x100000, b"advantage overlaps returns")]


def refused(lib, fn, h, a, word):
    from gl_gym_amd import _lib as L
    assert fn(h, C.byref(a), None) == L.EINVAL
    msg = lib.glgym_last_error()
    assert msg and word in msg, (word, msg)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every check happens before the handle is looked at: with good arguments and no handle the refusal names the handle, with a bad
    argument it names the argument."""
    import __graft_entry__ as g
    from gl_gym_amd import _lib as L
    if not L.LIB_PATH.exists():
        g.build()
    lib = L.load()
    refused(lib, lib.glgym_ac_rows, None, good_ac_args(), b"glgym_ac_rows: null handle")
    for path, value, word in AC_REFUSALS:
        a = good_ac_args()
        set_path(a, path, value)
        refused(lib, lib.glgym_ac_rows, None, a, word)
        assert b"glgym_ac_rows" in lib.glgym_last_error()
    a = good_ac_args()                                            # value_only: nothing but value_in and value is looked at
    a.value_only, a.mean_in, a.log_std, a.std, a.action, a.action_env, a.logp, a.obs_out, a.in_dim = 1, None, None, None, None, None, None, a.obs, 0
    refused(lib, lib.glgym_ac_rows, None, a, b"null handle")
    a = good_ac_args()                                            # without obs_out neither obs nor in_dim is looked at
    a.obs, a.obs_out, a.in_dim = None, None, -3
    refused(lib, lib.glgym_ac_rows, None, a, b"null handle")
    assert lib.glgym_ac_rows(None, None, None) == L.EINVAL
    refused(lib, lib.glgym_gae, None, good_gae_args(), b"glgym_gae: null handle")
    for path, value, word in GAE_REFUSALS:
        a = good_gae_args()
        set_path(a, path, value)
        refused(lib, lib.glgym_gae, None, a, word)
        assert b"glgym_gae" in lib.glgym_last_error()
    assert lib.glgym_gae(None, None, None) == L.EINVAL


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """tests/achost/achost.cpp with its own main, AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (nothing is
    loaded into Python): exactly sized heap buffers, so an index past an observation row, a head's output or a [T][B] block is
    reported."""
    exe = tmp_path / "achost_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DACHOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "achost ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
