"""CPU tests of device-side planning: csrc/gl_plan.hpp (host instantiation, tests/planhost/planhost.cpp -- the wavefront is an
array of 64 lanes, the butterfly exchanges are loops) against NumPy restatements written from include/glgym.h.

Bounds.  Returns, step counts, latches, best_k and best_return: EXACT (sums and products are rounded separately on both sides; the
argmax is a comparison).  MPPI mean: the double accumulators within 1e-12 absolute of NumPy's -- K <= 4 096 terms of magnitude <= 1
(weights <= 1, actions in [-1, 1]) summed in another order differ by at most 4 096 * 2^-53 = 4.5e-13 -- and the stored float32
values within one float32 ulp of NumPy's rounded mean."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SF_FAILED = 128


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_plan.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    so = tmp_path_factory.mktemp("planhost") / "libplanhost.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(so), str(ROOT / "tests" / "planhost" / "planhost.cpp")])
    lib = C.CDLL(str(so))
    lib.planhost_sizeof.argtypes, lib.planhost_sizeof.restype = [C.c_int], C.c_int
    lib.planhost_accumulate.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 10
    lib.planhost_accumulate.restype = None
    lib.planhost_select.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7 + [C.c_double, C.c_void_p, C.c_void_p]
    lib.planhost_select.restype = None
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


# ---- NumPy restatements (from the header's text, not from gl_plan.hpp) -----------------------------------------------------
def np_accumulate(w, reward, info, done, flags):
    n, B = reward.shape
    ret, viol = np.zeros(B), np.zeros((3, B))
    n_steps, alive, failed = np.zeros(B, np.int32), np.ones(B, bool), np.zeros(B, bool)
    for s in range(n):
        m = alive.copy()                                  # alive BEFORE the step
        ret[m] = ret[m] + w[s] * reward[s][m]
        viol[:, m] = viol[:, m] + info[s][:, m]
        n_steps[m] += 1
        failed[m] |= (flags[s][m] & SF_FAILED) != 0
        alive[m & (done[s] != 0)] = False
    return ret, viol, n_steps, alive, failed


def np_select(P, K, ret, failed, actions, temperature=None):
    H = actions.shape[0]
    best_k, best_ret = np.full(P, -1, np.int32), np.full(P, np.nan)
    best_action, best_seq = np.zeros((P, 6), np.float32), np.zeros((H, P, 6), np.float32)
    mean = np.zeros((H, P, 6))
    for p in range(P):
        r, f = ret[p * K:(p + 1) * K], failed[p * K:(p + 1) * K]
        adm = (f == 0) & np.isfinite(r)
        if not adm.any():
            continue
        k = int(np.argmax(np.where(adm, r, -np.inf)))     # first occurrence = lowest k
        best_k[p], best_ret[p] = k, r[k]
        best_action[p] = actions[0, p * K + k]
        best_seq[:, p] = actions[:, p * K + k]
        if temperature is not None:
            idx = np.nonzero(adm)[0]
            w = np.exp((r[idx] - r[k]) / temperature)
            w = w / w.sum()
            mean[:, p] = (w[None, :, None] * actions[:, p * K + idx].astype(np.float64)).sum(axis=1)
    return best_k, best_ret, best_action, best_seq, mean


def run_select(host, P, K, ret, failed, actions, temperature=None):
    H = actions.shape[0]
    best_k, best_ret = np.zeros(P, np.int32), np.zeros(P)
    best_action, best_seq = np.full((P, 6), 7, np.float32), np.full((H, P, 6), 7, np.float32)
    mean32 = np.full((H, P, 6), 7, np.float32) if temperature is not None else None
    mean64 = np.full((H, P, 6), 7.0) if temperature is not None else None
    host.planhost_select(P, K, H, ptr(ret), ptr(failed), ptr(actions), ptr(best_k), ptr(best_ret), ptr(best_action), ptr(best_seq),
                         float(temperature or 0.0), ptr(mean32), ptr(mean64))
    return best_k, best_ret, best_action, best_seq, mean32, mean64


def make_case(rng, P, K, H):
    ret = rng.normal(size=P * K)
    failed = (rng.random(P * K) < 0.1).astype(np.uint8)
    bad = rng.random(P * K)
    ret[bad < 0.05] = np.nan
    ret[(bad >= 0.05) & (bad < 0.08)] = np.inf
    ret[(bad >= 0.08) & (bad < 0.10)] = -np.inf
    actions = rng.uniform(-1, 1, (H, P * K, 6)).astype(np.float32)
    return ret, failed, actions


# ---- tests -------------------------------------------------------------------------------------------------------------------
def test_args_structs_have_the_headers_sizes(host):
    from gl_gym_amd import _lib as L
    for which, cls in enumerate((L.PlanForkArgs, L.PlanAccumulateArgs, L.PlanRolloutArgs, L.PlanSelectArgs, L.StepArgs)):
        assert C.sizeof(cls) == host.planhost_sizeof(which), cls.__name__
        assert cls._fields_[0][0] == "struct_size"
    a = L.make_plan_args(L.PlanSelectArgs, 3, 5, 7)
    assert (a.struct_size, a.P, a.K, a.H) == (C.sizeof(L.PlanSelectArgs), 3, 5, 7)
    r = L.make_plan_args(L.PlanRolloutArgs, 4, 0.99, L.make_step_args(8, 64))
    assert (r.H, r.gamma, r.step.struct_size, r.step.B, r.step.ld) == (4, 0.99, C.sizeof(L.StepArgs), 8, 64)


@pytest.mark.parametrize("gamma", [1.0, 0.99, 0.5])
def test_accumulate_and_latch_are_bit_exact(host, gamma):
    rng = np.random.default_rng(int(gamma * 100))
    n, B = 40, 257
    reward = rng.normal(size=(n, B)) * 10.0 ** rng.integers(-3, 3, (n, B))
    info = rng.random((n, 3, B))
    done = (rng.random((n, B)) < 0.04).astype(np.uint8)
    done[0, 0] = 1                                        # a child that ends with its first step: counted once
    done[:, 1] = 0                                        # ... and one that never ends
    flags = np.where(rng.random((n, B)) < 0.03, SF_FAILED | 3, rng.integers(0, 127, (n, B)) | (5 << 16)).astype(np.int32)
    w = np.empty(n)
    acc = 1.0
    for s in range(n):                                    # the running product of the header
        w[s] = acc
        acc = acc * gamma
    ret, viol = np.zeros(B), np.zeros((3, B))
    n_steps, alive, failed = np.zeros(B, np.int32), np.ones(B, np.uint8), np.zeros(B, np.uint8)
    host.planhost_accumulate(n, B, ptr(w), ptr(reward), ptr(info), ptr(done), ptr(flags), ptr(ret), ptr(viol), ptr(n_steps), ptr(alive),
                             ptr(failed))
    e_ret, e_viol, e_n, e_alive, e_failed = np_accumulate(w, reward, info, done, flags)
    assert np.array_equal(ret.view(np.uint64), e_ret.view(np.uint64))
    assert np.array_equal(viol.view(np.uint64), e_viol.view(np.uint64))
    assert np.array_equal(n_steps, e_n) and np.array_equal(alive.astype(bool), e_alive) and np.array_equal(failed.astype(bool), e_failed)
    assert n_steps[0] == 1 and not alive[0] and n_steps[1] == n and alive[1]
    first_done = np.where(done.any(axis=0), done.argmax(axis=0) + 1, n)        # the step that reports done is the last one counted
    assert np.array_equal(n_steps, first_done)
    assert 0 < alive.sum() < B and 0 < failed.sum() < B


@pytest.mark.parametrize("K", [1, 2, 37, 64, 65, 100, 200, 1000])
def test_select_matches_numpy_exactly(host, K):
    rng = np.random.default_rng(K)
    P, H = 9, 3
    ret, failed, actions = make_case(rng, P, K, H)
    if K >= 2:
        ret[0:K] = np.round(ret[0:K])                     # parent 0: exact ties (and whatever NaN / inf fell on it)
        failed[K:2 * K] = 1                               # parent 1: every candidate failed
        ret[2 * K:3 * K] = np.nan                         # parent 2: every return non-finite
        ret[3 * K:4 * K], failed[3 * K:4 * K] = 1.5, 0    # parent 3: all equal -> k = 0
        failed[4 * K] = 1                                 # parent 4: all equal but candidate 0 failed -> k = 1
        ret[4 * K:5 * K], failed[4 * K + 1:5 * K] = -2.0, 0
    got = run_select(host, P, K, ret, failed, actions)
    exp = np_select(P, K, ret, failed, actions)
    assert np.array_equal(got[0], exp[0])
    assert np.array_equal(got[1].view(np.uint64)[exp[0] >= 0], exp[1].view(np.uint64)[exp[0] >= 0])
    assert np.isnan(got[1][exp[0] < 0]).all()
    assert np.array_equal(got[2], exp[2]) and np.array_equal(got[3], exp[3])
    if K >= 2:
        assert got[0][1] == -1 and got[0][2] == -1 and got[0][3] == 0 and got[0][4] == 1
        assert (got[2][1] == 0).all() and (got[3][:, 2] == 0).all()


@pytest.mark.parametrize("K,temperature", [(1, 1.0), (37, 0.5), (64, 0.05), (200, 2.0), (1000, 0.3), (4096, 1.0)])
def test_mppi_mean_matches_numpy(host, K, temperature):
    rng = np.random.default_rng(1000 + K)
    P, H = 5, 4
    ret, failed, actions = make_case(rng, P, K, H)
    if K >= 2:
        failed[K:2 * K] = 1                               # an all-failed parent: zeros
    bad = (failed != 0) | ~np.isfinite(ret)
    actions[:, bad] = np.nan                              # the rows of inadmissible candidates must not be read into the mean
    got = run_select(host, P, K, ret, failed, actions, temperature)
    exp = np_select(P, K, ret, failed, np.nan_to_num(actions), temperature)
    assert np.array_equal(got[0], exp[0])
    err = np.abs(got[5] - exp[4]).max()
    print(f"MPPI mean K={K} T={temperature}: max |double accumulator - NumPy| = {err:.2e}")
    assert err <= 1e-12
    ref32 = exp[4].astype(np.float32)
    ulp = np.spacing(np.maximum(np.abs(ref32), np.float32(1e-30)))
    assert (np.abs(got[4].astype(np.float64) - ref32) <= ulp).all()
    assert np.array_equal(got[4], got[5].astype(np.float32))                  # stored = the accumulator rounded once
    if K >= 2:
        assert (got[4][:, 1] == 0).all() and got[0][1] == -1
    # the weights are a convex combination: every mean lies inside the actions' range
    assert (np.abs(got[5]) <= 1.0 + 1e-12).all()
