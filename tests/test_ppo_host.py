"""CPU tests of the PPO update: csrc/gl_ppo.hpp (host instantiation, tests/ppohost/ppohost.cpp -- a lane is a pass of a loop, a butterfly a
loop over 64) against NumPy restatements written from the text of include/glgym.h; the loss against torch's autograd in float64; the
refusals of glgym_ppo_batch / glgym_ppo_loss through libglgym.so (no device: every check precedes the handle).  The helpers below are also
what tests/test_gpu_ppo.py compares the kernels with.

Bounds.
* the permutation, the gathered rows, and -- given the ratio -- every per-row output and every sum of the loss: EXACT.  Every step is a
  single correctly rounded operation in a fixed order, which NumPy performs in the same order (np_reduce: lane, butterfly, wavefronts,
  blocks).
* ratio: within one float32 ulp of np.exp in double rounded to float (the host's libm and NumPy's differ in the last bits of a double).
* a sum of M terms in double against math.fsum: M additions, each with a relative error of at most 2^-53 on a partial sum no larger than
  sum |term|: |S - fsum| <= M 2^-52 sum |term| (sum_bound; twice what the argument gives).
* the advantage statistics against np.mean / np.std(ddof=1): from the sums' bounds e1 (on S1) and e2 (on S2) and u = 2^-52 for each further
  operation: |mean| off by at most e1 / M + u |mean|; var = (S2 - S1 S1 / M) / (M - 1) off by at most
  (e2 + 2 |S1| e1 / M + 4 u S1^2 / M + 2 u S2) / (M - 1) + 4 u var =: dv (the cancellation is in it: the terms are of the size of S2, not of
  var), and the deviation by dv / (2 sd) + u sd.
* float32 restatement against float64 autograd: the log-probability is 24 float32 operations on terms below about 10 for |z| <= 4, so
  |delta d| <= 24 * 10 * 2^-24 = 1.4e-5, and so is the ratio's relative error; 1e-4 of the largest |gradient| of a tensor is about six
  times that.  Rows whose ratio lies within 1e-4 of 1 - c or 1 + c, or whose |s1 - s2| lies within 1e-4 of zero outside the clip range,
  are left out (the gate can flip there); they must be at most 1 % of the rows."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_collect_host import AC_TAG, same_u32
from test_plan_cem_host import KEY_TAG as CEM_TAG, np_philox, within_one_f32_ulp
from test_plan_policy_host import set_path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SRC = ROOT / "tests" / "ppohost" / "ppohost.cpp"
NU = 6
PPO_TAG = 0x50524D31
M32 = 0xFFFFFFFF
BLOCK, MAX_BLOCKS, N_SUM, N_ADV = 256, 1024, 11, 2
S_SURR, S_VALUE, S_KL, S_CLIP, S_MAXRATIO, S_LS0 = 0, 1, 2, 3, 4, 5
HALF_LOG_2PI = np.float32(0.9189385)
SENTINEL = np.float32(7.25)
GUARD = 3
IN_DIMS = [1, 23, 24]
PERM_NS = [1, 2, 3, 4, 5, 15, 16, 17, 255, 256, 257, 1000, 4097, 65537]
f = np.float32


def build_host(path):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.ppohost_sizeof.argtypes, lib.ppohost_sizeof.restype = [C.c_int], C.c_int
    lib.ppohost_key_tag.argtypes, lib.ppohost_key_tag.restype = [], C.c_uint
    lib.ppohost_n_blocks.argtypes, lib.ppohost_n_blocks.restype = [C.c_longlong], C.c_int
    lib.ppohost_ws_bytes.argtypes, lib.ppohost_ws_bytes.restype = [C.c_int], C.c_longlong
    lib.ppohost_perm.argtypes = [C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_uint, C.c_void_p]
    lib.ppohost_perm.restype = None
    lib.ppohost_batch.argtypes, lib.ppohost_batch.restype = [C.c_void_p], None
    lib.ppohost_loss.argtypes, lib.ppohost_loss.restype = [C.c_void_p, C.c_void_p], None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_ppo.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    return build_host(tmp_path_factory.mktemp("ppohost") / "libppohost.so")


def guarded(shape, dtype=np.float32):
    """An output array with GUARD sentinel rows behind the last one, all sentinel to begin with."""
    return np.full((shape[0] + GUARD,) + tuple(shape[1:]), SENTINEL, dtype=dtype)


def same_f64(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return np.array_equal(a.view(np.uint64)[ok], b.view(np.uint64)[ok])


# ---- the restatements --------------------------------------------------------------------------------------------------------------------
def np_perm(N, D, seed, tag=PPO_TAG, p=None):
    """perm(p) for p = 0 .. N-1 (or the given positions): the balanced Feistel network over Philox words, cycle-walked into [0, N)."""
    w = 2
    while (1 << w) < N:
        w += 2
    half = w // 2
    mask = np.uint64((1 << half) - 1)

    def P(x):
        L, R = x >> np.uint64(half), x & mask
        for r in range(4):
            F = np_philox(R, r, D & M32, D >> 32, seed & M32, ((seed >> 32) ^ tag) & M32)[..., 0]
            L, R = R, L ^ (F & mask)
        return (L << np.uint64(half)) | R

    y = P(np.arange(N, dtype=np.uint64) if p is None else np.asarray(p, dtype=np.uint64))
    while True:
        bad = y >= N
        if not bad.any():
            return y.astype(np.int64)
        y[bad] = P(y[bad])


def n_blocks(M):
    return min(-(-M // BLOCK), MAX_BLOCKS)


def np_reduce(terms, kind="sum"):
    """terms [M] float64 -> the total in the header's order: block b takes chunks b, b + nb, ...; a lane its rows ascending from 0; the 64
    lanes by butterfly (xor 32 .. 1); the four wavefronts in index order; the blocks in block order."""
    terms = np.asarray(terms, dtype=np.float64)
    M, nb = len(terms), n_blocks(len(terms))
    n_chunk = -(-M // BLOCK)
    rounds = -(-n_chunk // nb)
    pad = -np.inf if kind == "max" else 0.0
    t = np.full(rounds * nb * BLOCK, pad)
    t[:M] = terms
    t = t.reshape(rounds, nb, BLOCK)
    op = (lambda a, b: np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.maximum(a, b)))) if kind == "max" else (lambda a, b: a + b)
    with np.errstate(all="ignore"):
        lane = np.full((nb, BLOCK), pad)
        for i in range(rounds):
            lane = op(lane, t[i])
        v = lane.reshape(nb, BLOCK // 64, 64)
        idx = np.arange(64)
        for m in (32, 16, 8, 4, 2, 1):
            v = op(v, v[..., idx ^ m])
        part = v[..., 0]
        blk = part[:, 0]
        for wv in range(1, BLOCK // 64):
            blk = op(blk, part[:, wv])
        total = blk[0]
        for b in range(1, nb):
            total = op(total, blk[b])
    return np.float64(total)


def sum_bound(terms):
    return len(terms) * 2.0 ** -52 * float(np.abs(np.asarray(terms, dtype=np.float64)).sum())


def np_adv_stats(adv):
    """-> [mean, unbiased standard deviation] of float32 advantages, the header's operations in its order."""
    a = adv.astype(np.float64)
    M = np.float64(len(a))
    S1, S2 = np_reduce(a), np_reduce(a * a)
    with np.errstate(all="ignore"):
        var = (S2 - (S1 * S1) / M) / (M - np.float64(1))
        return np.array([S1 / M, np.sqrt(var if var > 0 else np.float64(0))])


class LossCase:
    """Inputs of one glgym_ppo_loss call in NumPy: the heads' outputs mean [M, 6] and value [M], log_std / inv_std, the minibatch, adv_stats."""

    def __init__(self, M, seed=0, spread=0.3):
        rng = np.random.default_rng([seed, M, 77])
        self.M = M
        self.log_std = rng.uniform(-1.0, 0.5, NU).astype(f)
        self.inv_std = np.exp(-self.log_std.astype(np.float64)).astype(f)
        self.mean = rng.normal(size=(M, NU)).astype(f)
        e = np.clip(rng.normal(size=(M, NU)), -4, 4)
        self.mb_action = (self.mean + np.exp(self.log_std.astype(np.float64)) * e).astype(f)
        self.value = rng.normal(size=M).astype(f)
        self.mb_adv = (rng.normal(size=M) * 2 + 0.3).astype(f)
        self.mb_ret = rng.normal(size=M).astype(f)
        self.mb_value = (self.value + rng.normal(size=M) * 0.3).astype(f)
        self.mb_logp = (np_logp(self)[0] + rng.normal(size=M) * spread).astype(f)
        self.adv_stats = np_adv_stats(self.mb_adv) if M > 1 else np.array([0.0, 1.0])

    def arrays(self):
        return {k: getattr(self, k) for k in ("mean", "value", "log_std", "inv_std", "mb_action", "mb_logp", "mb_adv", "mb_ret", "mb_value", "adv_stats")}


def np_logp(c):
    """-> logp [M], z [M, 6], float32, every operation on its own."""
    with np.errstate(all="ignore"):
        z = (c.mb_action - c.mean) * c.inv_std
        s = np.zeros(c.M, dtype=f)
        for j in range(NU):
            s = s + (((f(-0.5) * z[:, j]) * z[:, j] - c.log_std[j]) - HALF_LOG_2PI)
    return s, z


def np_ratio64(c):
    """The ratio in double: exp of the float32 difference d."""
    with np.errstate(all="ignore"):
        return np.exp((np_logp(c)[0] - c.mb_logp).astype(np.float64))


def np_loss(c, ratio, clip_range=0.2, clip_range_vf=0.0, vf_coef=0.5, ent_coef=0.0, normalize=True):
    """Every output of the call given its ratio [M] float32, from the header's text."""
    M = c.M
    ratio = np.asarray(ratio, dtype=f)
    with np.errstate(all="ignore"):
        w = f(1.0 / M)
        cr, vf, ent = f(clip_range), f(vf_coef), f(ent_coef)
        lo, hi = f(1) - cr, f(1) + cr
        logp, z = np_logp(c)
        d = logp - c.mb_logp
        A = c.mb_adv
        if normalize:
            A = (c.mb_adv - f(c.adv_stats[0])) / (f(c.adv_stats[1]) + f(1e-8))
        s1 = ratio * A
        rc = np.fmin(np.fmax(ratio, lo), hi)
        s2 = rc * A
        surr = np.fmin(s1, s2)
        q = np.where(s1 <= s2, (-w) * s1, f(0)).astype(f)
        grad_mean = q[:, None] * (z * c.inv_std)
        ls_term = q[:, None] * (z * z - f(1))
        if clip_range_vf > 0:
            cv = f(clip_range_vf)
            dv = c.value - c.mb_value
            vp = c.mb_value + np.fmin(np.fmax(dv, -cv), cv)
            passes = (dv >= -cv) & (dv <= cv)
        else:
            vp, passes = c.value, np.ones(M, dtype=bool)
        vterm = (c.mb_ret - vp) * (c.mb_ret - vp)
        grad_value = np.where(passes, ((vf * f(2)) * w) * (vp - c.mb_ret), f(0)).astype(f)
        r1 = ratio - f(1)
        kl = r1 - d
        clipped = (np.abs(r1) > cr).astype(f)
        S = np.empty(N_SUM)
        S[S_SURR], S[S_VALUE], S[S_KL], S[S_CLIP] = np_reduce(surr), np_reduce(vterm), np_reduce(kl), np_reduce(clipped)
        S[S_MAXRATIO] = np_reduce(ratio, "max")
        for j in range(NU):
            S[S_LS0 + j] = np_reduce(ls_term[:, j])
        m = np.float64(M)
        policy, value_loss = -(S[S_SURR] / m), S[S_VALUE] / m
        e = f(0)
        for j in range(NU):
            e = e + ((f(0.5) + HALF_LOG_2PI) + c.log_std[j])
        entropy_loss = np.float64(-e)
        stats = np.array([(policy + np.float64(ent) * entropy_loss) + np.float64(vf) * value_loss, policy, value_loss, entropy_loss,
                          S[S_KL] / m, S[S_CLIP] / m, S[S_MAXRATIO], m])
        grad_log_std = S[S_LS0:].astype(f) - ent
    return dict(grad_mean=grad_mean.astype(f), grad_value=grad_value, grad_log_std=grad_log_std.astype(f), stats=stats, ratio_out=ratio,
                logp_out=logp, terms=dict(surr=surr, vterm=vterm, kl=kl, clipped=clipped, ls_term=ls_term), A=A, s1=s1, s2=s2)


LOSS_OUT = ("grad_mean", "grad_value", "grad_log_std", "stats", "ratio_out", "logp_out")
LOSS_CONFIGS = [dict(), dict(normalize=False), dict(clip_range_vf=0.15), dict(ent_coef=0.01, vf_coef=0.7), dict(clip_range=0.1, clip_range_vf=0.3, ent_coef=0.003, vf_coef=0.25, normalize=False)]


def loss_output_shapes(M):
    return dict(grad_mean=((M, NU), np.float32), grad_value=((M,), np.float32), grad_log_std=((NU,), np.float32), stats=((8,), np.float64),
                ratio_out=((M,), np.float32), logp_out=((M,), np.float32))


def loss_args(M, ptr, out, workspace, clip_range=0.2, clip_range_vf=0.0, vf_coef=0.5, ent_coef=0.0, normalize=True, workspace_bytes=None):
    """The glgym_ppo_loss_args of a case: ptr(name) -> the address of the input array `name`, out: {name: address}."""
    from gl_gym_amd import _lib as L
    return L.make_plan_args(L.PpoLossArgs, M, ptr("mean"), ptr("value"), ptr("log_std"), ptr("inv_std"), ptr("mb_action"), ptr("mb_logp"),
                            ptr("mb_adv"), ptr("mb_ret"), ptr("mb_value") if clip_range_vf > 0 else None, ptr("adv_stats") if normalize else None,
                            clip_range, clip_range_vf, vf_coef, ent_coef, out["grad_mean"], out["grad_value"], out["grad_log_std"], out["stats"],
                            out.get("ratio_out"), out.get("logp_out"), workspace,
                            L.PPO_LOSS_WS_BYTES if workspace_bytes is None else workspace_bytes)


def host_loss(host, c, ratio_in=None, **kw):
    """ppohost_loss on the case -> {name: array with its GUARD rows}; the workspace is exactly the stated size."""
    from gl_gym_amd import _lib as L
    arrays = c.arrays()
    outs = {k: guarded(s, dt) for k, (s, dt) in loss_output_shapes(c.M).items()}
    ws = np.zeros(L.PPO_LOSS_WS_BYTES // 8)
    a = loss_args(c.M, lambda k: arrays[k].ctypes.data, {k: v.ctypes.data for k, v in outs.items()}, ws.ctypes.data, **kw)
    r = None if ratio_in is None else np.ascontiguousarray(ratio_in, dtype=f)
    host.ppohost_loss(C.addressof(a), None if r is None else r.ctypes.data)
    return outs


def check_loss(got, want, M):
    """got: guarded outputs; rows < M (or the whole vector) equal want bit for bit, the guard rows hold their sentinel."""
    for k in LOSS_OUT:
        n = {"grad_log_std": NU, "stats": 8}.get(k, M)
        same = same_f64 if k == "stats" else same_u32
        assert same(got[k][:n], want[k]), (k, got[k][:n], want[k])
        assert (got[k][n:] == SENTINEL).all(), k


class BatchCase:
    """The flat [N] sources of a glgym_ppo_batch call in NumPy."""

    def __init__(self, N, in_dim, seed=0):
        rng = np.random.default_rng([seed, N, in_dim, 5])
        self.N, self.in_dim = N, in_dim
        self.obs = rng.uniform(-2, 2, (N, in_dim)).astype(f)
        self.action = rng.normal(size=(N, NU)).astype(f)
        self.logp, self.advantage, self.returns, self.value = (rng.normal(size=N).astype(f) * s for s in (3, 2, 1, 1.5))

    def arrays(self):
        return {k: getattr(self, k) for k in ("obs", "action", "logp", "advantage", "returns", "value")}


BATCH_PAIRS = dict(mb_obs="obs", mb_action="action", mb_logp="logp", mb_adv="advantage", mb_ret="returns", mb_value="value")


def batch_output_shapes(M, in_dim):
    return dict(mb_obs=((M, in_dim), np.float32), mb_action=((M, NU), np.float32), mb_logp=((M,), np.float32), mb_adv=((M,), np.float32),
                mb_ret=((M,), np.float32), mb_value=((M,), np.float32), mb_index=((M,), np.int32), adv_stats=((2,), np.float64))


def batch_args(c, M, offset, ptr, out, workspace, seed=1, draw_index=0, draw_base=None, want_index=True, want_stats=True, workspace_bytes=None):
    from gl_gym_amd import _lib as L
    return L.make_plan_args(L.PpoBatchArgs, c.N, M, offset, c.in_dim, seed, draw_index, draw_base, ptr("obs"), ptr("action"), ptr("logp"),
                            ptr("advantage"), ptr("returns"), ptr("value"), out["mb_obs"], out["mb_action"], out["mb_logp"], out["mb_adv"],
                            out["mb_ret"], out["mb_value"], out["mb_index"] if want_index else None, out["adv_stats"] if want_stats else None,
                            workspace if want_stats else None, L.PPO_BATCH_WS_BYTES if workspace_bytes is None else workspace_bytes)


def host_batch(host, c, M, offset, draw_base=None, **kw):
    from gl_gym_amd import _lib as L
    arrays = c.arrays()
    outs = {k: guarded(s, dt) for k, (s, dt) in batch_output_shapes(M, c.in_dim).items()}
    ws = np.zeros(L.PPO_BATCH_WS_BYTES // 8)
    base = None if draw_base is None else np.array([draw_base], dtype=np.uint64)
    a = batch_args(c, M, offset, lambda k: arrays[k].ctypes.data, {k: v.ctypes.data for k, v in outs.items()}, ws.ctypes.data,
                   draw_base=None if base is None else base.ctypes.data, **kw)
    host.ppohost_batch(C.addressof(a))
    return outs


def np_batch(c, M, offset, D, seed, want_stats=True):
    idx = np_perm(c.N, D, seed)[offset:offset + M]
    out = {k: getattr(c, src)[idx] for k, src in BATCH_PAIRS.items()}
    out["mb_index"] = idx.astype(np.int32)
    if want_stats:
        out["adv_stats"] = np_adv_stats(out["mb_adv"])
    return out


def check_batch(got, want, M):
    """got: guarded outputs.  Every name in want equals it bit for bit in rows < M with its guard intact; every other output is untouched."""
    for k, v in got.items():
        if k in want:
            n = 2 if k == "adv_stats" else M
            if k == "mb_index":
                assert np.array_equal(v[:n], want[k]), k
                assert (v[n:] == np.int32(SENTINEL)).all(), k
            else:
                assert (same_f64 if k == "adv_stats" else same_u32)(v[:n], want[k]), (k, v[:n], want[k])
                assert (v[n:] == SENTINEL).all(), k
        else:
            assert (v == v.dtype.type(SENTINEL)).all(), k


def host_perm(host, N, D, seed, tag=PPO_TAG, p0=0, n=None):
    n = N - p0 if n is None else n
    out = np.full(n, -7, dtype=np.int32)
    host.ppohost_perm(N, p0, n, D, seed, tag, out.ctypes.data)
    return out


# ---- 0. the feature is there -----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_bound_and_declared(host):
    from gl_gym_amd import _lib as L
    header = (ROOT / "include" / "glgym.h").read_text()
    for name in ("glgym_ppo_batch", "glgym_ppo_loss"):
        assert name in L.PROTOTYPES and f"int {name}(glgym_handle h" in header
    assert "#define GLGYM_ABI_VERSION 7" in header and L.ABI_VERSION == 7
    assert [host.ppohost_sizeof(i) for i in range(2)] == [C.sizeof(L.PpoBatchArgs), C.sizeof(L.PpoLossArgs)]
    assert host.ppohost_key_tag() == PPO_TAG == L.PPO_KEY_TAG and "0x50524d31" in header
    assert PPO_TAG not in (AC_TAG, CEM_TAG, 0x5343454E, 0x5753434E)
    assert [host.ppohost_ws_bytes(i) for i in range(2)] == [L.PPO_BATCH_WS_BYTES, L.PPO_LOSS_WS_BYTES] == [16384, 90112]
    assert "16 384 bytes" in header and "90 112 bytes" in header
    for M in (1, 255, 256, 257, BLOCK * MAX_BLOCKS, BLOCK * MAX_BLOCKS + 1, 2 ** 31 - 256):
        assert host.ppohost_n_blocks(M) == n_blocks(M)
    import gl_gym_amd
    assert {"PPO", "ppo_loss"} <= set(gl_gym_amd.__all__)


# ---- 1. the permutation ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", PERM_NS)
def test_perm_is_a_permutation_and_matches_numpy(host, N):
    for D, seed in ((0, 0), (3, 0xFEDCBA9876543210), (2 ** 40 + 17, 2 ** 64 - 1)):
        p = host_perm(host, N, D, seed)
        assert np.array_equal(np.sort(p), np.arange(N)), (N, D, seed)
        assert np.array_equal(p, np_perm(N, D, seed)), (N, D, seed)


def test_perm_changes_with_seed_draw_and_tag(host):
    N = 4097
    ref = host_perm(host, N, 10, 7)
    for D, seed, tag in ((11, 7, PPO_TAG), (10, 8, PPO_TAG), (10, 7 + 2 ** 32, PPO_TAG), (10 + 2 ** 32, 7, PPO_TAG), (10, 7, AC_TAG), (10, 7, CEM_TAG)):
        other = host_perm(host, N, D, seed, tag)
        assert np.array_equal(np.sort(other), np.arange(N))
        # two independent uniform permutations agree in one place on average: 40 of 4097 would be 39 standard deviations
        assert (other == ref).sum() < 40, (D, seed, tag)
        assert np.array_equal(other, np_perm(N, D, seed, tag))


@pytest.mark.parametrize("N", [5, 257, 1000])
def test_perm_does_not_depend_on_the_split(host, N):
    whole = host_perm(host, N, 4, 99)
    for M in (1, 7, N):
        parts = [host_perm(host, N, 4, 99, p0=o, n=min(M, N - o)) for o in range(0, N, M)]
        assert np.array_equal(np.concatenate(parts), whole), M


def test_perm_fixed_points_average_one(host):
    """A uniform permutation has one fixed point on average, with variance one: the mean over 256 draws has standard deviation 1/16, and
    [0.5, 1.5] is eight of them.  The seeds are fixed: the value printed is the value."""
    N = 1000
    counts = [int((host_perm(host, N, D, 2026) == np.arange(N)).sum()) for D in range(256)]
    avg = float(np.mean(counts))
    print(f"fixed points of perm at N = {N}, mean over 256 draws: {avg:.4f}")
    assert 0.5 <= avg <= 1.5, avg


# ---- 2. the batch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim", IN_DIMS)
def test_batch_rows_are_the_permuted_source_rows(host, in_dim):
    c = BatchCase(1000, in_dim)
    seed, draw_index, base = 0xABCDEF0123, 5, 9
    for M, offset in ((257, 300), (1, 999), (1000, 0), (65, 0)):
        got = host_batch(host, c, M, offset, seed=seed, draw_index=draw_index, draw_base=base, want_stats=M > 1)
        check_batch(got, np_batch(c, M, offset, draw_index + base, seed, want_stats=M > 1), M)
    # optional outputs not asked for are not written; the others do not change
    lean = host_batch(host, c, 257, 300, seed=seed, draw_index=draw_index, draw_base=base, want_index=False, want_stats=False)
    want = np_batch(c, 257, 300, draw_index + base, seed, want_stats=False)
    del want["mb_index"]
    check_batch(lean, want, 257)


def test_batch_ragged_epoch_covers_every_transition_once(host):
    c = BatchCase(1000, 23)
    M = 384                                                     # 384 + 384 + 232
    idx = []
    for o in range(0, c.N, M):
        m = min(M, c.N - o)
        got = host_batch(host, c, m, o, seed=3, draw_index=1)
        check_batch(got, np_batch(c, m, o, 1, 3), m)
        idx.append(got["mb_index"][:m])
    assert [len(i) for i in idx] == [384, 384, 232] and np.array_equal(np.sort(np.concatenate(idx)), np.arange(c.N))


@pytest.mark.parametrize("M", [2, 65, 257, 1000])
def test_adv_stats_against_float64_numpy(host, M):
    c = BatchCase(1000, 1, seed=M)
    got = host_batch(host, c, M, 0, seed=8)
    adv = got["mb_adv"][:M].astype(np.float64)
    mean, sd = got["adv_stats"][:2]
    assert same_f64(got["adv_stats"][:2], np_adv_stats(got["mb_adv"][:M]))
    u = 2.0 ** -52
    S1, S2 = math.fsum(adv), math.fsum(adv * adv)
    e1, e2 = sum_bound(adv), sum_bound(adv * adv)
    assert abs(np_reduce(adv) - S1) <= e1 and abs(np_reduce(adv * adv) - S2) <= e2
    assert abs(mean - np.mean(adv)) <= e1 / M + 2 * u * abs(mean)
    var = np.var(adv, ddof=1)
    dv = (e2 + 2 * abs(S1) * e1 / M + 4 * u * S1 * S1 / M + 2 * u * S2) / (M - 1) + 4 * u * var
    true_sd = np.std(adv, ddof=1)
    print(f"M = {M}: |mean - np.mean| = {abs(mean - np.mean(adv)):.2e}, |sd - np.std| = {abs(sd - true_sd):.2e} (bound {dv / (2 * true_sd) + u * true_sd:.2e})")
    assert abs(sd - true_sd) <= dv / (2 * true_sd) + 2 * u * true_sd


def test_adv_stats_of_equal_advantages_is_clamped_at_zero(host):
    c = BatchCase(300, 1)
    c.advantage[:] = f(0.1)                                     # S2 - S1 S1 / M is a rounding residue of either sign
    got = host_batch(host, c, 300, 0)
    assert got["adv_stats"][1] >= 0 and got["adv_stats"][1] < 1e-7 and same_f64(got["adv_stats"][:2], np_adv_stats(got["mb_adv"][:300]))


# ---- 3. the loss -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 4096])
def test_loss_matches_numpy(host, M):
    c = LossCase(M, seed=1)
    for cfg in LOSS_CONFIGS:
        if M == 1 and cfg.get("normalize", True):
            continue
        got = host_loss(host, c, **cfg)
        ratio = got["ratio_out"][:M]
        assert within_one_f32_ulp(ratio, np_ratio64(c)), cfg
        check_loss(got, np_loss(c, ratio, **cfg), M)
        # the ratio handed in gives the same call
        check_loss(host_loss(host, c, ratio_in=ratio, **cfg), np_loss(c, ratio, **cfg), M)


def test_loss_sums_against_fsum(host):
    M = 4096
    c = LossCase(M, seed=2)
    cfg = dict(clip_range_vf=0.15, ent_coef=0.01, vf_coef=0.7)
    got = host_loss(host, c, **cfg)
    want = np_loss(c, got["ratio_out"][:M], **cfg)
    t = want["terms"]
    st = got["stats"][:8]
    for name, k, scale in (("surr", 1, -1.0), ("vterm", 2, 1.0), ("kl", 4, 1.0), ("clipped", 5, 1.0)):
        terms = t[name].astype(np.float64)
        assert abs(st[k] * M * scale - math.fsum(terms)) <= sum_bound(terms) + 2.0 ** -52 * abs(st[k] * M), name
    assert st[6] == got["ratio_out"][:M].max() and st[7] == M
    assert 0.2 < st[5] < 0.8 and st[4] > 0                      # the clip is at work on this case
    for j in range(NU):
        terms = t["ls_term"][:, j].astype(np.float64)
        g = float(got["grad_log_std"][j]) + float(f(0.01))
        assert abs(g - math.fsum(terms)) <= sum_bound(terms) + 2.0 ** -23 * (abs(g) + 0.01)   # two float32 roundings behind the sum


def test_a_nan_mean_poisons_its_own_row_and_the_sums_it_enters(host):
    M = 300
    c = LossCase(M, seed=3)
    clean = host_loss(host, c)
    c.mean[70, 2] = np.nan
    got = host_loss(host, c)
    check_loss(got, np_loss(c, got["ratio_out"][:M]), M)
    # q = 0 (NaN <= x is false) times a NaN z is NaN, times a finite z is 0: the NaN column of the row, and the row's ratio and logp
    assert np.isnan(got["grad_mean"][70, 2]) and np.isnan(got["ratio_out"][70]) and np.isnan(got["logp_out"][70])
    assert not got["grad_mean"][70, [0, 1, 3, 4, 5]].any()
    others = np.arange(M) != 70
    for k in ("grad_mean", "grad_value", "ratio_out", "logp_out"):
        assert same_u32(got[k][:M][others], clean[k][:M][others]), k
    st = got["stats"][:8]
    assert np.isnan(st[4]) and np.isnan(st[6]) and np.isnan(got["grad_log_std"][2]) and st[7] == M
    assert np.isfinite(got["grad_log_std"][[0, 1, 3, 4, 5]]).all() and np.isfinite(st[2])


# ---- 4. against autograd ---------------------------------------------------------------------------------------------------------------
AUTOGRAD_SEED = 0


def test_float32_restatement_against_float64_autograd(host):
    import torch
    M, cr, vf_coef, ent_coef = 4096, 0.2, 0.5, 0.01
    c = LossCase(M, seed=AUTOGRAD_SEED)
    got = host_loss(host, c, ent_coef=ent_coef, vf_coef=vf_coef)
    want = np_loss(c, got["ratio_out"][:M], ent_coef=ent_coef, vf_coef=vf_coef)
    check_loss(got, want, M)
    ratio, A = got["ratio_out"][:M].astype(np.float64), want["A"].astype(np.float64)
    # the four cells: sign of A x ratio beyond a clip bound
    cells = [(s, b, float(((A > 0 if s else A < 0) & (ratio > 1 + cr if b else ratio < 1 - cr)).mean())) for s in (0, 1) for b in (0, 1)]
    print("share of rows per cell (A > 0, ratio > 1 + c):", cells)
    assert min(x[2] for x in cells) >= 0.05, cells
    outside = (ratio < 1 - cr) | (ratio > 1 + cr)
    doubtful = (np.abs(ratio - (1 - cr)) < 1e-4) | (np.abs(ratio - (1 + cr)) < 1e-4) | (outside & (np.abs(want["s1"].astype(np.float64) - want["s2"]) < 1e-4))
    print(f"rows left out: {int(doubtful.sum())} of {M}")
    assert doubtful.mean() <= 0.01
    keep = torch.as_tensor(~doubtful)

    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    mean, value, log_std = T(c.mean).requires_grad_(), T(c.value).requires_grad_(), T(c.log_std).requires_grad_()
    adv = T(c.mb_adv)
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    logp = (-0.5 * ((T(c.mb_action) - mean) / log_std.exp()) ** 2 - log_std - 0.5 * math.log(2 * math.pi)).sum(-1)
    r = (logp - T(c.mb_logp)).exp()
    surr = torch.min(r * adv, torch.clamp(r, 1 - cr, 1 + cr) * adv)
    # the rows left out contribute nothing on either side; with none left out this is PPO.train's loss, -surr.mean() + ...
    policy = -(surr * keep).sum() / M
    value_loss = torch.nn.functional.mse_loss(T(c.mb_ret), value)
    entropy_loss = -(0.5 + 0.5 * math.log(2 * math.pi) + log_std).sum()
    loss = policy + ent_coef * entropy_loss + vf_coef * value_loss
    loss.backward()
    if not doubtful.any():
        assert abs(float(loss) - got["stats"][0]) <= 1e-4 * max(1.0, abs(float(loss)))
    k = ~doubtful
    gm64, gv64, gl64 = mean.grad.numpy(), value.grad.numpy(), log_std.grad.numpy()
    gm32, gv32 = got["grad_mean"][:M].astype(np.float64), got["grad_value"][:M].astype(np.float64)
    gl32 = np.array([math.fsum(want["terms"]["ls_term"][k, j].astype(np.float64)) for j in range(NU)]) - float(f(ent_coef))
    if not doubtful.any():
        assert np.abs(gl32 - got["grad_log_std"][:NU]).max() <= 2.0 ** -22 * np.abs(gl32).max()
    for name, a32, a64 in (("grad_mean", gm32[k], gm64[k]), ("grad_value", gv32, gv64), ("grad_log_std", gl32, gl64)):
        err, big = np.abs(a32 - a64).max(), np.abs(a64).max()
        print(f"{name}: max |float32 - float64| = {err:.3e}, largest |gradient| = {big:.3e}, ratio {err / big:.2e}")
        assert err <= 1e-4 * big, name
    assert (gm64[~k] == 0).all()


# ---- 5. refusals without a device ------------------------------------------------------------------------------------------------------
P_ = 0x10000                                                  # a non-null pointer: never followed, nothing is launched
MB_ = 0x100000                                                # the distance between two of them: 130 x 24 floats fit many times


def good_batch_args():
    from gl_gym_amd import _lib as L
    p = [P_ + k * MB_ for k in range(16)]
    return L.make_plan_args(L.PpoBatchArgs, 520, 130, 260, 23, 1, 0, None, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11],
                            p[12], p[13], p[14], L.PPO_BATCH_WS_BYTES)


def good_loss_args():
    from gl_gym_amd import _lib as L
    p = [P_ + k * MB_ for k in range(20)]
    return L.make_plan_args(L.PpoLossArgs, 130, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], 0.2, 0.1, 0.5, 0.0, p[10], p[11], p[12],
                            p[13], p[14], p[15], p[16], L.PPO_LOSS_WS_BYTES)


NAN, INF = float("nan"), float("inf")
BATCH_REFUSALS = [("struct_size", 8, b"struct_size"), ("N", 0, b"N < 1"), ("N", -3, b"N < 1"), ("N", 2 ** 31 - 255, b"2^31 - 256 transitions"),
                  ("M", 0, b"M < 1"), ("M", -1, b"M < 1"), ("offset", -1, b"offset < 0"), ("offset", 391, b"offset + M > N"),
                  ("M", 261, b"offset + M > N"), ("in_dim", 0, b"in_dim outside"), ("in_dim", 1025, b"in_dim outside"),
                  ("obs", None, b"null obs"), ("action", None, b"null obs"), ("logp", None, b"null obs"), ("advantage", None, b"null obs"),
                  ("returns", None, b"null obs"), ("value", None, b"null obs"), ("mb_obs", None, b"null mb_obs"), ("mb_action", None, b"null mb_obs"),
                  ("mb_logp", None, b"null mb_obs"), ("mb_adv", None, b"null mb_obs"), ("mb_ret", None, b"null mb_obs"),
                  ("mb_value", None, b"null mb_obs"), ("workspace", None, b"without a workspace"), ("workspace_bytes", 16383, b"workspace smaller"),
                  ("mb_obs", P_, b"overlaps a source"), ("mb_obs", P_ + 520 * 23 * 4 - 4, b"overlaps a source"),
                  ("mb_logp", P_ + 3 * MB_, b"overlaps a source"), ("mb_index", P_ + MB_, b"overlaps a source"),
                  ("adv_stats", P_ + 5 * MB_ + 520 * 4 - 8, b"overlaps a source"), ("workspace", P_ + 4 * MB_, b"overlaps a source"),
                  ("mb_action", P_ + 6 * MB_ + 130 * 23 * 4 - 4, b"overlaps another output"), ("mb_index", P_ + 9 * MB_, b"overlaps another output"),
                  ("adv_stats", P_ + 14 * MB_ + 16384 - 8, b"overlaps another output")]
LOSS_REFUSALS = [("struct_size", 4, b"struct_size"), ("M", 0, b"M < 1"), ("M", 2 ** 31 - 255, b"2^31 - 256 rows"), ("clip_range", 0.0, b"clip_range not > 0"),
                 ("clip_range", -0.2, b"clip_range not > 0"), ("clip_range", NAN, b"clip_range not > 0"), ("clip_range", INF, b"clip_range not > 0"),
                 ("clip_range_vf", NAN, b"clip_range_vf not finite"), ("clip_range_vf", INF, b"clip_range_vf not finite"),
                 ("vf_coef", NAN, b"vf_coef not finite"), ("vf_coef", -INF, b"vf_coef not finite"), ("ent_coef", NAN, b"ent_coef not finite"),
                 ("ent_coef", INF, b"ent_coef not finite"), ("mb_value", None, b"without mb_value"), ("mean", None, b"null mean"),
                 ("value", None, b"null mean"), ("log_std", None, b"null mean"), ("inv_std", None, b"null mean"), ("mb_action", None, b"null mean"),
                 ("mb_logp", None, b"null mean"), ("mb_adv", None, b"null mean"), ("mb_ret", None, b"null mean"), ("grad_mean", None, b"null grad_mean"),
                 ("grad_value", None, b"null grad_mean"), ("grad_log_std", None, b"null grad_mean"), ("stats", None, b"null grad_mean"),
                 ("workspace", None, b"null workspace"), ("workspace_bytes", 90111, b"workspace smaller"), ("workspace_bytes", 0, b"workspace smaller"),
                 ("grad_mean", P_, b"overlaps an input"), ("grad_mean", P_ + 130 * 24 - 4, b"overlaps an input"),
                 ("grad_value", P_ + 8 * MB_, b"overlaps an input"), ("stats", P_ + 9 * MB_ + 8, b"overlaps an input"),
                 ("grad_log_std", P_ + 2 * MB_ + 20, b"overlaps an input"), ("workspace", P_ + 5 * MB_, b"overlaps an input"),
                 ("ratio_out", P_ + 10 * MB_ + 130 * 24 - 4, b"overlaps another output"), ("logp_out", P_ + 14 * MB_, b"overlaps another output"),
                 ("stats", P_ + 16 * MB_ + 90112 - 8, b"overlaps another output")]


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
    refused(lib, lib.glgym_ppo_batch, None, good_batch_args(), b"glgym_ppo_batch: null handle")
    for path, value, word in BATCH_REFUSALS:
        a = good_batch_args()
        set_path(a, path, value)
        refused(lib, lib.glgym_ppo_batch, None, a, word)
        assert b"glgym_ppo_batch" in lib.glgym_last_error()
    a = good_batch_args()
    a.M, a.offset = 1, 0
    refused(lib, lib.glgym_ppo_batch, None, a, b"adv_stats with M < 2")
    a.adv_stats = a.workspace = None                              # without adv_stats neither the workspace nor M >= 2 is asked for
    a.workspace_bytes = 0
    refused(lib, lib.glgym_ppo_batch, None, a, b"null handle")
    a = good_batch_args()                                         # the optional index left out; the whole permutation in one minibatch
    a.mb_index, a.M, a.offset = None, 520, 0
    refused(lib, lib.glgym_ppo_batch, None, a, b"null handle")
    assert lib.glgym_ppo_batch(None, None, None) == L.EINVAL

    refused(lib, lib.glgym_ppo_loss, None, good_loss_args(), b"glgym_ppo_loss: null handle")
    for path, value, word in LOSS_REFUSALS:
        a = good_loss_args()
        set_path(a, path, value)
        refused(lib, lib.glgym_ppo_loss, None, a, word)
        assert b"glgym_ppo_loss" in lib.glgym_last_error()
    a = good_loss_args()                                          # every optional pointer left out, the value clip off
    a.mb_value = a.adv_stats = a.ratio_out = a.logp_out = None
    a.clip_range_vf = -1.0
    refused(lib, lib.glgym_ppo_loss, None, a, b"null handle")
    assert lib.glgym_ppo_loss(None, None, None) == L.EINVAL


def test_ppo_refuses_what_is_out_of_scope():
    import gl_gym_amd

    class Col:                                                    # the constructor's checks come before anything is allocated
        T, B, D, device = 4, 130, 23, "cpu"
    for kw, exc in ((dict(target_kl=0.01), NotImplementedError), (dict(clip_range=lambda p: 0.2), NotImplementedError),
                    (dict(clip_range_vf=lambda p: 0.2), NotImplementedError), (dict(clip_range=0.0), ValueError),
                    (dict(clip_range_vf=-1.0), ValueError)):
        with pytest.raises(exc):
            gl_gym_amd.PPO(Col(), None, **kw)


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """tests/ppohost/ppohost.cpp with its own main, AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (nothing is
    loaded into Python): exactly sized heap buffers, so an index past a source row, a minibatch row or the stated workspace is reported."""
    exe = tmp_path / "ppohost_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DPPOHOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ppohost ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
