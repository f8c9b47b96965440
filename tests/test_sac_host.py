"""CPU tests of soft actor-critic: csrc/gl_sac.hpp (host instantiation, tests/sachost/sachost.cpp -- a lane is a pass of a loop, a butterfly
a loop over 64) against NumPy restatements written from the text of include/glgym.h; the gradients against torch's autograd in float64; the
refusals of the five entry points through libglgym.so (no device: every check precedes the handle).  The helpers below are also what
tests/test_gpu_sac.py compares the kernels with.

Bounds.  u = 2^-24 is float32's unit roundoff.
* Philox words (through the uniform mode, whose arithmetic is exact in double), the sampling indices, the gathered rows, u = mean + std e and
  c = (1 - a a) + 1e-6 given std and a, the log-probability and the executed action given e, ls and l, the backward pass given what the
  forward pass saved, every per-row output and every sum of the two loss stages, the Polyak update: EXACT.  Every step is a single correctly
  rounded operation in a fixed order, which NumPy performs in the same order (np_reduce of tests/test_ppo_host.py for the sums).
* the noise e: within one float32 ulp of the float64 Box-Muller value rounded to float (the host's libm and NumPy's differ in the last
  bits of a double), as tests/test_collect_host.py holds glgym_ac_rows' noise.
* std, tanh and the log term l: within one float32 ulp of np.exp / np.tanh / np.log in double rounded to float.
* float32 against float64 autograd, the squashed sample (test_sample_gradients_against_float64_autograd): the float64 chain starts from the
  same float32 mean, log_std and e, so only roundings separate the two.  With s = std e:
    du   = |s| (2^-23 + u) + u |u|                         std is within one ulp (relative 2^-23), the product and the sum round once each
    da   = 1.01 g du + 2^-23                               d tanh / du = g = 1 - a a (1 % for its change over du); tanh within one ulp, and
                                                           its ulp is at most 2^-24 below 1 -- twice that for the comparison value's own rounding
    dg   = 2 |a| da + 2 u                                  a a and 1 - a a round once each
    t4   = 2 a g / (g + 1e-6):  dt4 = (2 |a| 1e-6 / (g_lo + 1e-6)^2) dg + (2 g / (g + 1e-6)) da + 5 u |t4|,   g_lo = max(g - dg, 0)
                                                           the first factor is |d t4 / d g|, largest at the lower end of g's interval: a
                                                           saturated tanh (g below 1e-6) is ill-conditioned by up to 2e6, and the bound says so
    dgu  = |ga| dg + u |ga g| + |gl| dt4 + u |gl t4| + u |gu|
    dgls = dgu |s| + 3 u |gu s| + u |grad_log_std| + ref
  grad_mean is held to dgu and grad_log_std to dgls element by element.  ref is the float64 reference's own error, which only grad_log_std
  has: Normal.log_prob(u) forms x = u - mean again from a rounded u, |x - s| <= dx = 2^-53 (|u| + |s|), and autograd's two paths into
  log_std -- x x / std^2 through the scale and -x s' / std^2 through u, s' the float64 product std e within 2^-53 |s| of s -- leave
  x (x - s') / std^2, of the size |e| (dx + 2^-53 |s|) / std, where the exact chain leaves 0; each path is about eight float64 operations on
  a term of the size e e.  So ref = |gl| (|e| (dx + 2^-53 |s|) / std + 8 2^-53 e e): small against u except where std is near exp(-20) and
  |mean| is not.  The two paths into mean (through loc and through value) carry the same rounded x with opposite signs and cancel exactly:
  grad_mean needs no such term.  Rows with a log_std within 1e-4 of -20 or 2 are left out (the
  clamp's gate can flip there): at most 1 % of the rows, asserted.
* float32 against float64 autograd, the loss stages: y is four float32 operations on terms no larger than |r| + |m| + |alpha logp| and a
  float32 gamma: dy = 5 u (|r| + |m| + |alpha logp|); grad_q = w (q - y): w dy + 3 u |grad_q| (the difference, the product, w's own
  rounding).  Actor stage: grad_logp = w alpha within 2 u of itself, grad_q exactly -w (up to w's rounding, u w) on the side of the smaller
  q; rows with |q1 - q2| < 1e-4 are left out (at most 1 %, asserted).  grad_log_alpha: the mean of M float32 sums logp + target_entropy,
  each within u of its value: u mean |term| + u |g| for the final cast."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_collect_host import AC_TAG, same_u32
from test_plan_cem_host import KEY_TAG as CEM_TAG, np_philox, within_one_f32_ulp
from test_plan_policy_host import set_path
from test_ppo_host import PPO_TAG, n_blocks, np_reduce, same_f64, sum_bound

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SRC = ROOT / "tests" / "sachost" / "sachost.cpp"
NU = 6
SAC_TAG, SMP_TAG = 0x53414331, 0x534D5031
M32 = 0xFFFFFFFF
BLOCK, MAX_BLOCKS, N_SUM = 256, 1024, 5
HALF_LOG_2PI = np.float32(0.9189385)
SENTINEL = np.float32(7.25)
GUARD = 3
IN_DIMS = [1, 23, 24]
U = 2.0 ** -24
f = np.float32


def build_host(path):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.sachost_sizeof.argtypes, lib.sachost_sizeof.restype = [C.c_int], C.c_int
    lib.sachost_key_tag.argtypes, lib.sachost_key_tag.restype = [C.c_int], C.c_uint
    lib.sachost_ws_bytes.argtypes, lib.sachost_ws_bytes.restype = [], C.c_longlong
    lib.sachost_noise.argtypes = [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_void_p]
    lib.sachost_noise.restype = None
    lib.sachost_rows.argtypes, lib.sachost_rows.restype = [C.c_void_p] * 6, None
    lib.sachost_u.argtypes, lib.sachost_u.restype = [C.c_void_p] * 6, None
    for name in ("sachost_rows_grad", "sachost_batch", "sachost_loss", "sachost_polyak"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [C.c_void_p], None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_sac.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    return build_host(tmp_path_factory.mktemp("sachost") / "libsachost.so")


def guarded(shape, dtype=np.float32):
    """An output array with GUARD sentinel rows behind the last one, all sentinel to begin with."""
    return np.full((shape[0] + GUARD,) + tuple(shape[1:]), SENTINEL, dtype=dtype)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return same_f64(a, b) if a.dtype == np.float64 else same_u32(a, b) if a.dtype == np.float32 else np.array_equal(a, b)


# ---- the restatements: noise -------------------------------------------------------------------------------------------------------------
def np_words(keys, step, blk0, D, seed, tag=SAC_TAG):
    """r0..r7 [M, 8] uint64 of the row keys: counter (k, 4 step + blk0 + blk, lo32(D), hi32(D)), key (lo32(seed), hi32(seed) ^ tag)."""
    k = np.asarray(keys, dtype=np.uint64) & np.uint64(M32)
    return np.concatenate([np_philox(k, 4 * step + blk0 + blk, D & M32, D >> 32, seed & M32, ((seed >> 32) ^ tag) & M32) for blk in (0, 1)], axis=-1)


def np_eps64(keys, step, blk0, D, seed, tag=SAC_TAG):
    """e (blk0 = 0) or e2 (blk0 = 2) [M, 6] in float64: Box-Muller on words 0..5."""
    u = (np_words(keys, step, blk0, D, seed, tag).astype(np.float64) + 0.5) * 2.0 ** -32
    e = np.empty((len(u), NU))
    for m in range(3):
        rad, ang = np.sqrt(-2.0 * np.log(u[:, 2 * m])), 2.0 * np.pi * u[:, 2 * m + 1]
        e[:, 2 * m], e[:, 2 * m + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return e


def np_uniform(keys, step, D, seed):
    r = np_words(keys, step, 0, D, seed)[:, :NU].astype(np.float64)
    return (2.0 * ((r + 0.5) * 2.0 ** -32) - 1.0).astype(f)


# ---- the squashed Gaussian -----------------------------------------------------------------------------------------------------------------
class RowsCase:
    """Inputs of one glgym_sac_rows call in NumPy: the actor's outputs mean and log_std [M, 6] (log_std beyond both clamps) and observations."""

    def __init__(self, M, in_dim=3, seed=0):
        rng = np.random.default_rng([seed, M, in_dim, 41])
        self.M, self.in_dim = M, in_dim
        self.mean_in = (rng.normal(size=(M, NU)) * 1.5).astype(f)
        self.log_std_in = rng.uniform(-21.0, 3.0, (M, NU)).astype(f)
        self.obs = rng.uniform(-2, 2, (M, in_dim)).astype(f)

    def arrays(self):
        return {k: getattr(self, k) for k in ("mean_in", "log_std_in", "obs")}


ROWS_OUT = ("obs_out", "action", "action_env", "action_slot", "logp", "eps", "eps2", "std", "tanh", "corr")
UNIFORM_OUT = ("obs_out", "action", "action_env", "action_slot")


def rows_output_shapes(M, in_dim):
    d = {k: ((M, NU), np.float32) for k in ROWS_OUT}
    d["obs_out"], d["logp"] = ((M, in_dim), np.float32), ((M,), np.float32)
    return d


def rows_args(case, ptr, out, step=0, seed=1, draw_index=0, draw_base=None, row0=0, deterministic=0, uniform=0, sigma=0.0):
    """The glgym_sac_rows_args of a case: ptr(name) -> the address of the input array `name`, out: {name: address} of the outputs wanted."""
    from gl_gym_amd import _lib as L
    return L.make_plan_args(L.SacRowsArgs, case.M, case.in_dim, step, deterministic, uniform, row0, ptr("mean_in"), ptr("log_std_in"), seed, draw_index,
                            draw_base, sigma, ptr("obs"), *[out.get(k) for k in ROWS_OUT])


def host_rows(host, case, given=None, want=ROWS_OUT, draw_base=None, **kw):
    """sachost_rows on the case -> {name: array with its GUARD rows} for every output, the ones not in `want` untouched.  given: {"eps",
    "eps2", "std", "tanh", "corr"} arrays [M, 6] that replace the noise and the transcendentals' results."""
    arrays = case.arrays()
    outs = {k: guarded(s, dt) for k, (s, dt) in rows_output_shapes(case.M, case.in_dim).items()}
    base = None if draw_base is None else np.array([draw_base], dtype=np.uint64)
    a = rows_args(case, lambda k: arrays[k].ctypes.data, {k: outs[k].ctypes.data for k in want}, draw_base=None if base is None else base.ctypes.data, **kw)
    g = {k: np.ascontiguousarray(v, dtype=f) for k, v in (given or {}).items()}
    host.sachost_rows(C.addressof(a), *[g[k].ctypes.data if k in g else None for k in ("eps", "eps2", "std", "tanh", "corr")])
    return outs


def host_u(host, case, std, tanh, eps=None, **kw):
    """-> u, c [M, 6] of the call given its deviations and tanh values."""
    arrays = case.arrays()
    a = rows_args(case, lambda k: arrays[k].ctypes.data, {}, **kw)
    u, c = np.empty((case.M, NU), dtype=f), np.empty((case.M, NU), dtype=f)
    std, tanh = np.ascontiguousarray(std, dtype=f), np.ascontiguousarray(tanh, dtype=f)
    eps = None if eps is None else np.ascontiguousarray(eps, dtype=f)
    host.sachost_u(C.addressof(a), None if eps is None else eps.ctypes.data, std.ctypes.data, u.ctypes.data, c.ctypes.data, tanh.ctypes.data)
    return u, c


def np_clamp_ls(log_std_in):
    with np.errstate(all="ignore"):
        return np.fmin(np.fmax(log_std_in, f(-20)), f(2))


def np_rows(case, e, e2, std, tanh, corr, sigma=0.0):
    """Everything the call writes given its noise and the three transcendentals' results, float32, every operation on its own."""
    with np.errstate(all="ignore"):
        ls = np_clamp_ls(case.log_std_in)
        e, a, l = np.asarray(e, dtype=f), np.asarray(tanh, dtype=f), np.asarray(corr, dtype=f)
        s = np.zeros(case.M, dtype=f)
        for j in range(NU):
            s = s + (((f(-0.5) * e[:, j]) * e[:, j] - ls[:, j]) - HALF_LOG_2PI)
        for j in range(NU):
            s = s - l[:, j]
        v = a + f(sigma) * np.asarray(e2, dtype=f) if sigma > 0 else a
        env = np.fmin(np.fmax(v, f(-1)), f(1))
    return dict(obs_out=case.obs, action=a, action_env=env.astype(f), action_slot=env.astype(f), logp=s, eps=e, eps2=np.asarray(e2, dtype=f) if sigma > 0 else np.zeros((case.M, NU), dtype=f), std=np.asarray(std, dtype=f), tanh=a, corr=l)


def check_outputs(got, want, n_rows, written):
    """got: guarded outputs.  Every name in `written` equals want bit for bit in rows < n with its guard intact; the others are untouched."""
    for k, v in got.items():
        if k in written:
            assert same_bits(v[:n_rows], want[k]), (k, v[:n_rows], want[k])
            assert (v[n_rows:] == v.dtype.type(SENTINEL)).all(), k
        else:
            assert (v == v.dtype.type(SENTINEL)).all(), k


def grad_args(M, ptr, out):
    from gl_gym_amd import _lib as L
    return L.make_plan_args(L.SacRowsGradArgs, M, ptr("grad_action"), ptr("grad_logp"), ptr("eps"), ptr("std"), ptr("tanh"), ptr("log_std_in"),
                            out["grad_mean"], out["grad_log_std"])


def host_grad(host, inputs):
    M = len(inputs["grad_logp"])
    outs = dict(grad_mean=guarded((M, NU)), grad_log_std=guarded((M, NU)))
    a = grad_args(M, lambda k: inputs[k].ctypes.data, {k: v.ctypes.data for k, v in outs.items()})
    host.sachost_rows_grad(C.addressof(a))
    return outs


def np_grad(i):
    with np.errstate(all="ignore"):
        a, e, sd, ga, gl, ls_in = i["tanh"], i["eps"], i["std"], i["grad_action"], i["grad_logp"][:, None], i["log_std_in"]
        g = f(1) - a * a
        gu = (ga * g) + (gl * (((f(2) * a) * g) / (g + f(1e-6))))
        inside = (ls_in >= f(-20)) & (ls_in <= f(2))
        gls = np.where(inside, (gu * (sd * e)) - gl, f(0)).astype(f)
    return dict(grad_mean=gu.astype(f), grad_log_std=gls)


def grad_inputs(host, case, seed=3, **kw):
    """A forward pass of the host build on the case and random upstream gradients -> the inputs of the backward pass."""
    rng = np.random.default_rng([seed, case.M])
    fw = host_rows(host, case, **kw)
    M = case.M
    return dict(grad_action=rng.normal(size=(M, NU)).astype(f), grad_logp=rng.normal(size=M).astype(f), eps=fw["eps"][:M].copy(),
                std=fw["std"][:M].copy(), tanh=fw["tanh"][:M].copy(), log_std_in=case.log_std_in)


# ---- the replay ring ---------------------------------------------------------------------------------------------------------------------
class RingCase:
    """A replay ring in NumPy: obs [S, B, D] whose first column names its own flat row, action, reward, done."""

    def __init__(self, S, B, in_dim, seed=0):
        rng = np.random.default_rng([seed, S, B, in_dim, 9])
        self.S, self.B, self.in_dim = S, B, in_dim
        self.obs = rng.uniform(-2, 2, (S, B, in_dim)).astype(f)
        self.obs[:, :, 0] = np.arange(S * B, dtype=f).reshape(S, B)          # exact in float32 below 2^24
        self.action = rng.normal(size=(S, B, NU)).astype(f)
        self.reward = rng.normal(size=(S, B)).astype(f)
        self.done = (rng.random((S, B)) < 0.2).astype(np.uint8)

    def arrays(self):
        return {k: getattr(self, k) for k in ("obs", "action", "reward", "done")}


BATCH_OUT = ("mb_obs", "mb_next_obs", "mb_action", "mb_reward", "mb_done", "index_out")


def batch_output_shapes(M, in_dim):
    return dict(mb_obs=((M, in_dim), np.float32), mb_next_obs=((M, in_dim), np.float32), mb_action=((M, NU), np.float32),
                mb_reward=((M,), np.float32), mb_done=((M,), np.uint8), index_out=((M,), np.int64))


def batch_args(c, M, head, n_valid, ptr, out, seed=1, draw_index=0, draw_base=None, want_index=True):
    from gl_gym_amd import _lib as L
    return L.make_plan_args(L.SacBatchArgs, c.S, c.B, c.in_dim, M, head, n_valid, 0, seed, draw_index, draw_base, ptr("obs"), ptr("action"),
                            ptr("reward"), ptr("done"), out["mb_obs"], out["mb_next_obs"], out["mb_action"], out["mb_reward"], out["mb_done"],
                            out["index_out"] if want_index else None)


def host_batch(host, c, M, head, n_valid, draw_base=None, **kw):
    arrays = c.arrays()
    outs = {k: guarded(s, dt) for k, (s, dt) in batch_output_shapes(M, c.in_dim).items()}
    base = None if draw_base is None else np.array([draw_base], dtype=np.uint64)
    a = batch_args(c, M, head, n_valid, lambda k: arrays[k].ctypes.data, {k: v.ctypes.data for k, v in outs.items()},
                   draw_base=None if base is None else base.ctypes.data, **kw)
    host.sachost_batch(C.addressof(a))
    return outs


def np_index(M, S, B, head, n_valid, D, seed):
    """-> flat rows slot * B + b of the transitions and of their successor observations, [M] int64 each, in exact integer arithmetic."""
    r = np_philox(np.arange(M, dtype=np.uint64), 0, D & M32, D >> 32, seed & M32, ((seed >> 32) ^ SMP_TAG) & M32)
    n = n_valid * B
    row, nxt = np.empty(M, dtype=np.int64), np.empty(M, dtype=np.int64)
    for p in range(M):
        w = (int(r[p, 0]) << 32) | int(r[p, 1])
        idx = (w * n) >> 64
        slot, b = (head + idx // B) % S, idx % B
        row[p], nxt[p] = slot * B + b, ((slot + 1) % S) * B + b
    return row, nxt


def np_batch(c, M, head, n_valid, D, seed, want_index=True):
    row, nxt = np_index(M, c.S, c.B, head, n_valid, D, seed)
    flat = lambda a: a.reshape((c.S * c.B,) + a.shape[2:])  # noqa: E731
    out = dict(mb_obs=flat(c.obs)[row], mb_next_obs=flat(c.obs)[nxt], mb_action=flat(c.action)[row], mb_reward=flat(c.reward)[row],
               mb_done=flat(c.done)[row])
    if want_index:
        out["index_out"] = row
    return out


# ---- the loss stages -----------------------------------------------------------------------------------------------------------------------
class LossCase:
    """Inputs of a glgym_sac_loss call of either stage in NumPy: q drawn from N(0, 1)."""

    def __init__(self, M, seed=0):
        rng = np.random.default_rng([seed, M, 13])
        self.M = M
        self.q1, self.q2, self.q1_next, self.q2_next = (rng.normal(size=M).astype(f) for _ in range(4))
        self.logp = (rng.normal(size=M) * 2 - 4).astype(f)
        self.reward = rng.normal(size=M).astype(f)
        self.done = (rng.random(M) < 0.1).astype(np.uint8)
        self.alpha = np.array([0.2], dtype=f)
        self.log_alpha = np.log(self.alpha.astype(np.float64)).astype(f)

    def arrays(self):
        return {k: getattr(self, k) for k in ("q1", "q2", "logp", "q1_next", "q2_next", "reward", "done", "alpha", "log_alpha")}


LOSS_OUT = {0: ("grad_q1", "grad_q2", "target_out", "stats"), 1: ("grad_q1", "grad_q2", "grad_logp", "grad_log_alpha", "stats")}
ALL_LOSS_OUT = ("grad_q1", "grad_q2", "grad_logp", "target_out", "grad_log_alpha", "stats")


def loss_output_shapes(M):
    return dict(grad_q1=((M,), np.float32), grad_q2=((M,), np.float32), grad_logp=((M,), np.float32), target_out=((M,), np.float32),
                grad_log_alpha=((1,), np.float32), stats=((8,), np.float64))


def loss_rows(M):
    return dict(grad_q1=M, grad_q2=M, grad_logp=M, target_out=M, grad_log_alpha=1, stats=8)


def loss_args(M, stage, ptr, out, workspace, gamma=0.9631, target_entropy=-6.0, workspace_bytes=None, want=None):
    from gl_gym_amd import _lib as L
    want = LOSS_OUT[stage] if want is None else want
    o = lambda k: out[k] if k in want else None  # noqa: E731
    c = stage == 0
    return L.make_plan_args(L.SacLossArgs, M, stage, 0, ptr("q1"), ptr("q2"), ptr("logp"), ptr("q1_next") if c else None, ptr("q2_next") if c else None,
                            ptr("reward") if c else None, ptr("done") if c else None, ptr("alpha"), None if c else ptr("log_alpha"), gamma,
                            target_entropy, o("grad_q1"), o("grad_q2"), o("grad_logp"), o("target_out"), o("grad_log_alpha"), o("stats"), workspace,
                            L.SAC_LOSS_WS_BYTES if workspace_bytes is None else workspace_bytes)


def host_loss(host, c, stage, **kw):
    from gl_gym_amd import _lib as L
    arrays = c.arrays()
    outs = {k: guarded(s, dt) for k, (s, dt) in loss_output_shapes(c.M).items()}
    ws = np.zeros(L.SAC_LOSS_WS_BYTES // 8)
    a = loss_args(c.M, stage, lambda k: arrays[k].ctypes.data, {k: v.ctypes.data for k, v in outs.items()}, ws.ctypes.data, **kw)
    host.sachost_loss(C.addressof(a))
    return outs


def np_loss(c, stage, gamma=0.9631, target_entropy=-6.0):
    M = c.M
    with np.errstate(all="ignore"):
        w, alpha, m = f(1.0 / M), c.alpha[0], np.float64(M)
        if stage == 0:
            mn = np.fmin(c.q1_next, c.q2_next)
            nd = f(1) - (c.done != 0).astype(f)
            y = c.reward + ((nd * f(gamma)) * (mn - (alpha * c.logp)))
            d1, d2 = c.q1 - y, c.q2 - y
            S1, S2, Q1, Q2, Y = (np_reduce(t) for t in (d1 * d1, d2 * d2, c.q1, c.q2, y))
            stats = np.array([(0.5 * (S1 + S2)) / m, S1 / m, S2 / m, Q1 / m, Q2 / m, Y / m, np.float64(alpha), m])
            return dict(grad_q1=(w * d1).astype(f), grad_q2=(w * d2).astype(f), target_out=y.astype(f), stats=stats)
        first = c.q1 <= c.q2
        ta = (alpha * c.logp) - np.fmin(c.q1, c.q2)
        te = c.logp + f(target_entropy)
        A, E, P = np_reduce(ta), np_reduce(te), np_reduce(c.logp)
        la = np.float64(c.log_alpha[0])
        stats = np.array([A / m, -(la * (E / m)), -(E / m), P / m, np.float64(alpha), la, 0.0, m])
        return dict(grad_q1=np.where(first, -w, f(0)).astype(f), grad_q2=np.where(first, f(0), -w).astype(f),
                    grad_logp=np.full(M, w * alpha, dtype=f), grad_log_alpha=np.array([-(E / m)]).astype(f), stats=stats)


def check_loss(got, want, stage):
    for k, v in got.items():
        n = loss_rows(len(got["grad_q1"]) - GUARD)[k]
        if k in LOSS_OUT[stage]:
            assert same_bits(v[:n], want[k]), (k, v[:n], want[k])
            assert (v[n:] == v.dtype.type(SENTINEL)).all(), k
        else:
            assert (v == v.dtype.type(SENTINEL)).all(), k


# ---- Polyak ----------------------------------------------------------------------------------------------------------------------------------
POLYAK_COUNTS = [0, 1, 63, 257, 1025]


def np_polyak(t, s, tau):
    tau = f(tau)
    return ((f(1) - tau) * t) + (tau * s)


def polyak_tensors(counts=POLYAK_COUNTS, seed=0):
    """-> (targets, sources): float32 arrays of the given sizes; the 257-element pair is a view at an odd element offset of a larger array."""
    rng = np.random.default_rng([seed, 17])
    ts, ss = [], []
    for n in counts:
        t, s = rng.normal(size=n + 1).astype(f), rng.normal(size=n + 1).astype(f)
        ts.append(t[1:] if n == 257 else t[:n])
        ss.append(s[1:] if n == 257 else s[:n])
    return ts, ss


def polyak_args(n, dst, src, count, max_count, tau):
    from gl_gym_amd import _lib as L
    return L.make_plan_args(L.PolyakArgs, n, dst, src, count, max_count, tau)


# ---- 0. the feature is there -----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_bound_and_declared(host):
    from gl_gym_amd import _lib as L
    header = (ROOT / "include" / "glgym.h").read_text()
    names = ("glgym_sac_rows", "glgym_sac_rows_grad", "glgym_sac_batch", "glgym_sac_loss", "glgym_polyak")
    for name in names:
        assert name in L.PROTOTYPES and f"int {name}(glgym_handle h" in header
    assert "#define GLGYM_ABI_VERSION 7" in header and L.ABI_VERSION == 7
    structs = (L.SacRowsArgs, L.SacRowsGradArgs, L.SacBatchArgs, L.SacLossArgs, L.PolyakArgs)
    assert [host.sachost_sizeof(i) for i in range(5)] == [C.sizeof(s) for s in structs]
    assert host.sachost_key_tag(0) == SAC_TAG == L.SAC_KEY_TAG and "0x53414331" in header
    assert host.sachost_key_tag(1) == SMP_TAG == L.SAC_SAMPLE_TAG and "0x534d5031" in header
    assert len({SAC_TAG, SMP_TAG, AC_TAG, CEM_TAG, PPO_TAG, 0x5343454E, 0x5753434E}) == 7
    assert host.sachost_ws_bytes() == L.SAC_LOSS_WS_BYTES == 40960 and "40 960 bytes" in header
    import gl_gym_amd
    assert {"SAC", "ReplayCollector", "squashed_sample"} <= set(gl_gym_amd.__all__)


# ---- 1. noise and the squashed Gaussian ----------------------------------------------------------------------------------------------------
def host_noise(host, row0, M, step, blk0, D, seed):
    out = np.full((M, NU), 7, dtype=f)
    host.sachost_noise(row0, M, step, blk0, D, seed, out.ctypes.data)
    return out


def test_words_are_exact_and_noise_matches_the_float64_box_muller(host):
    for row0, step, D, seed in ((0, 0, 0, 0), (1000, 7, 3, 0xFEDCBA9876543210), (2 ** 32 - 300, 2 ** 30 - 1, 2 ** 40 + 17, 2 ** 64 - 1)):
        M = 300
        keys = row0 + np.arange(M)
        # the uniform mode is exact arithmetic on the words: equality there is equality of the Philox words
        c = RowsCase(M)
        got = host_rows(host, c, want=UNIFORM_OUT, uniform=1, row0=row0, step=step, seed=seed, draw_index=D)
        want = np_uniform(keys, step, D, seed)
        assert same_u32(got["action"][:M], want) and same_u32(got["action_env"][:M], want) and (np.abs(want) <= 1).all()
        for blk0 in (0, 2):
            e = host_noise(host, row0, M, step, blk0, D, seed)
            assert within_one_f32_ulp(e, np_eps64(keys, step, blk0, D, seed)), (row0, step, blk0)
    # row0 + r is the key: a call on rows 100 .. 149 is rows 100 .. 149 of a call on 0 .. 299, whatever M
    whole, part = host_noise(host, 0, 300, 2, 0, 5, 9), host_noise(host, 100, 50, 2, 0, 5, 9)
    assert same_u32(whole[100:150], part)
    # step, draw, seed, block pair and tag each change the draw
    ref = host_noise(host, 0, 64, 2, 0, 5, 9)
    for other in (host_noise(host, 0, 64, 3, 0, 5, 9), host_noise(host, 0, 64, 2, 2, 5, 9), host_noise(host, 0, 64, 2, 0, 6, 9),
                  host_noise(host, 0, 64, 2, 0, 5, 10), host_noise(host, 0, 64, 2, 0, 5 + 2 ** 32, 9), host_noise(host, 0, 64, 2, 0, 5, 9 + 2 ** 32)):
        assert not (other == ref).any()
    assert not (np_eps64(np.arange(64), 2, 0, 5, 9, AC_TAG).astype(f) == ref).any()
    # blocks 2 | 3 of step k are not blocks 0 | 1 of step k + 1: the counter's second word is 4 step + blk
    assert not (host_noise(host, 0, 64, 2, 2, 5, 9) == host_noise(host, 0, 64, 3, 0, 5, 9)).any()


@pytest.mark.parametrize("in_dim", IN_DIMS)
def test_rows_match_numpy(host, in_dim):
    for M, sigma, det in ((1, 0.0, 0), (65, 0.05, 0), (257, 0.0, 0), (257, 0.3, 1)):
        c = RowsCase(M, in_dim, seed=M)
        kw = dict(step=3, seed=0xABCDEF0123, draw_index=5, row0=17, deterministic=det, sigma=sigma)
        got = host_rows(host, c, draw_base=9, **kw)
        keys = 17 + np.arange(M)
        e, std, a, l = (got[k][:M] for k in ("eps", "std", "tanh", "corr"))
        e2 = host_noise(host, 17, M, 3, 2, 14, 0xABCDEF0123)                             # D = draw_index + *draw_base
        assert same_u32(got["eps2"][:M], e2 if sigma > 0 else np.zeros_like(e2))
        if det:
            assert not e.any()
        else:
            assert within_one_f32_ulp(e, np_eps64(keys, 3, 0, 14, 0xABCDEF0123))
        assert within_one_f32_ulp(e2, np_eps64(keys, 3, 2, 14, 0xABCDEF0123))
        ls = np_clamp_ls(c.log_std_in)
        assert ls.min() == -20 and ls.max() == 2 or M == 1
        # the three transcendentals, each within one ulp of NumPy's double result; u and c exactly
        u, cc = host_u(host, c, std, a, draw_base=None, **{**kw, "draw_index": 14})
        with np.errstate(all="ignore"):
            assert same_u32(u, c.mean_in + std * e) and same_u32(cc, (f(1) - a * a) + f(1e-6))
        assert within_one_f32_ulp(std, np.exp(ls.astype(np.float64)))
        assert within_one_f32_ulp(a, np.tanh(u.astype(np.float64)))
        assert within_one_f32_ulp(l, np.log(cc.astype(np.float64)))
        # everything else exactly, given them -- and handing them back in gives the same call
        want = np_rows(c, e, e2, std, a, l, sigma)
        check_outputs(got, want, M, ROWS_OUT)
        check_outputs(host_rows(host, c, given=dict(std=std, tanh=a, corr=l), draw_base=9, **kw), want, M, ROWS_OUT)
        assert (np.abs(got["action_env"][:M]) <= 1).all() and np.isfinite(got["logp"][:M]).all()
        # outputs not asked for are not written; the others do not change
        lean = ("action_env", "logp")
        check_outputs(host_rows(host, c, want=lean, draw_base=9, **kw), want, M, lean)


def test_extreme_inputs_give_a_legal_executed_action(host):
    M = 64
    c = RowsCase(M)
    c.mean_in[0], c.mean_in[1], c.mean_in[2], c.mean_in[3, 2] = np.nan, np.inf, -np.inf, np.nan
    c.log_std_in[4], c.log_std_in[5], c.log_std_in[6], c.log_std_in[7] = -20, 2, -np.inf, np.inf
    c.log_std_in[8], c.log_std_in[9, 1] = np.nan, np.nan
    for sigma in (0.0, 0.05):
        got = host_rows(host, c, sigma=sigma, seed=4)
        env, a = got["action_env"][:M], got["action"][:M]
        assert (np.abs(env) <= 1).all() and same_u32(env, got["action_slot"][:M])           # NaN <= 1 is false: no NaN either
        assert (env[0] == -1).all() and env[3, 2] == -1 and np.isnan(a[0]).all()             # a NaN reads as -1
        assert (env[1] == 1).all() and (env[2] == -1).all() or sigma > 0
        assert within_one_f32_ulp(got["std"][6], np.full(NU, np.exp(-20.0))) and within_one_f32_ulp(got["std"][7], np.full(NU, np.exp(2.0)))
        assert within_one_f32_ulp(got["std"][8], np.full(NU, np.exp(-20.0)))                  # fmaxf hands on -20 for a NaN log_std
        want = np_rows(c, got["eps"][:M], host_noise(host, 0, M, 0, 2, 0, 4), got["std"][:M], got["tanh"][:M], got["corr"][:M], sigma)
        check_outputs(got, want, M, ROWS_OUT)


def test_backward_matches_numpy(host):
    for M in (1, 65, 257):
        c = RowsCase(M, seed=M + 1)
        i = grad_inputs(host, c, seed=5)
        got, want = host_grad(host, i), np_grad(i)
        for k in ("grad_mean", "grad_log_std"):
            assert same_u32(got[k][:M], want[k]) and (got[k][M:] == SENTINEL).all(), k
        outside = (c.log_std_in < -20) | (c.log_std_in > 2)
        assert outside.any() or M == 1
        assert not got["grad_log_std"][:M][outside].any()
    i["log_std_in"] = i["log_std_in"].copy()
    i["log_std_in"][0, 0], i["log_std_in"][0, 1], i["log_std_in"][0, 2] = np.nan, -20, 2     # NaN: outside; the ends: inside
    got = host_grad(host, i)
    assert got["grad_log_std"][0, 0] == 0 and same_u32(got["grad_log_std"][:M], np_grad(i)["grad_log_std"])
    assert got["grad_log_std"][0, 1] != 0 and got["grad_log_std"][0, 2] != 0


# ---- 2. sampling from the ring -----------------------------------------------------------------------------------------------------------
RING_CASES = [(3, 5, 0, 1), (3, 5, 2, 2), (4, 1, 3, 3), (2, 65537, 0, 1)]


@pytest.mark.parametrize("S,B,head,n_valid", RING_CASES)
def test_sampling_indices_are_exact_and_land_in_valid_slots(host, S, B, head, n_valid):
    for in_dim, M in ((1, 257), (23, 65), (24, 1)):
        c = RingCase(S, B, in_dim)
        seed, draw_index, base = 0xABCDEF0123, 5, 9
        got = host_batch(host, c, M, head, n_valid, seed=seed, draw_index=draw_index, draw_base=base)
        want = np_batch(c, M, head, n_valid, draw_index + base, seed)
        check_outputs(got, want, M, BATCH_OUT)
        row = got["index_out"][:M]
        slot, b = row // B, row % B
        assert (((slot - head) % S) < n_valid).all() and (b < B).all()
        # the next observation comes from the successor slot, across the wrap
        assert np.array_equal(got["mb_obs"][:M, 0], row.astype(f)) and np.array_equal(got["mb_next_obs"][:M, 0], (((slot + 1) % S) * B + b).astype(f))
        if (S, head, n_valid) == (3, 2, 2) and M == 257:
            assert (slot == 2).any() and (slot == 0).any() and not (slot == 1).any()         # head 2, two slots: 2 and, wrapped, 0
        lean = host_batch(host, c, M, head, n_valid, seed=seed, draw_index=draw_index, draw_base=base, want_index=False)
        del want["index_out"]
        check_outputs(lean, want, M, tuple(want))
    other = host_batch(host, c, 1, head, n_valid, seed=seed, draw_index=draw_index + 1, draw_base=base)
    assert other["index_out"][0] != got["index_out"][0] or n_valid * B < 64


def test_sampling_is_uniform_over_the_valid_cells(host):
    """M = 65 536 draws over 64 cells (S = 5, B = 16, four valid slots from head 3, wrapping), one fixed seed: Pearson's chi-square with 63
    degrees of freedom against its 99.9 % quantile, 103.44."""
    S, B, head, n_valid, M = 5, 16, 3, 4, 65536
    c = RingCase(S, B, 1)
    got = host_batch(host, c, M, head, n_valid, seed=2026, draw_index=1)
    row = got["index_out"][:M]
    assert np.array_equal(row, np_index(M, S, B, head, n_valid, 1, 2026)[0])
    cell = ((row // B - head) % S) * B + row % B
    counts = np.bincount(cell, minlength=64)
    assert len(counts) == 64
    chi2 = float(((counts - M / 64) ** 2 / (M / 64)).sum())
    print(f"chi-square of {M} draws over 64 cells: {chi2:.2f} (99.9 % quantile 103.44)")
    assert chi2 <= 103.44


# ---- 3. the loss stages and Polyak ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 4096])
def test_loss_matches_numpy(host, M):
    c = LossCase(M, seed=1)
    for stage in (0, 1):
        for cfg in (dict(), dict(gamma=0.5, target_entropy=-3.25)):
            check_loss(host_loss(host, c, stage, **cfg), np_loss(c, stage, **cfg), stage)
    lean = host_loss(host, c, 0, want=("grad_q1", "grad_q2", "stats"))                    # the optional target left out
    assert (lean["target_out"] == SENTINEL).all() and same_u32(lean["grad_q1"][:M], np_loss(c, 0)["grad_q1"])


def test_loss_sums_against_fsum(host):
    M = 4096
    c = LossCase(M, seed=2)
    got, want = host_loss(host, c, 0)["stats"][:8], np_loss(c, 0)
    y = want["target_out"]
    d1, d2 = c.q1 - y, c.q2 - y
    for k, terms in ((1, d1 * d1), (2, d2 * d2), (3, c.q1), (4, c.q2), (5, y)):
        terms = np.asarray(terms, dtype=np.float64)
        assert abs(got[k] * M - math.fsum(terms)) <= sum_bound(terms) + 2.0 ** -52 * abs(got[k] * M), k
    assert abs(got[0] - 0.5 * (got[1] + got[2])) <= 2.0 ** -50 * got[0] and got[7] == M
    a = host_loss(host, c, 1)["stats"][:8]
    for k, terms, sign in ((0, c.alpha[0] * c.logp - np.fmin(c.q1, c.q2), 1.0), (2, c.logp + f(-6.0), -1.0), (3, c.logp, 1.0)):
        terms = np.asarray(terms, dtype=np.float64)
        assert abs(sign * a[k] * M - math.fsum(terms)) <= sum_bound(terms) + 2.0 ** -52 * abs(a[k] * M), k
    assert a[1] == -(np.float64(c.log_alpha[0]) * -a[2]) and a[4] == np.float64(c.alpha[0]) and a[7] == M


def test_nan_follows_fminf(host):
    M = 300
    c = LossCase(M, seed=3)
    clean0, clean1 = host_loss(host, c, 0), host_loss(host, c, 1)
    c.q1_next[5], c.q1_next[6], c.q2_next[6], c.logp[7], c.q1[8] = np.nan, np.nan, np.nan, np.nan, np.nan
    got = host_loss(host, c, 0)
    check_loss(got, np_loss(c, 0), 0)
    y = got["target_out"][:M]
    assert np.isfinite(y[5]) and np.isnan(y[6]) and np.isnan(y[7]) and np.isfinite(y[8])      # one NaN target critic: the other's value
    assert np.isnan(got["grad_q1"][8]) and np.isfinite(got["grad_q2"][8]) and np.isnan(got["stats"][0]) and np.isnan(got["stats"][5])
    others = np.ones(M, bool)
    others[[5, 6, 7, 8]] = False
    assert same_u32(got["grad_q1"][:M][others], clean0["grad_q1"][:M][others])
    got = host_loss(host, c, 1)
    check_loss(got, np_loss(c, 1), 1)
    w = f(1.0 / M)
    assert got["grad_q1"][8] == 0 and got["grad_q2"][8] == -w                                # NaN <= q2 is false: the gradient goes to q2
    assert np.isnan(got["stats"][0]) and np.isnan(got["stats"][2]) and np.isnan(got["grad_log_alpha"][0])
    assert same_u32(got["grad_logp"][:M], clean1["grad_logp"][:M])


def test_polyak_matches_numpy(host):
    for tau in (0.0135, 0.0, 1.0, 0.5):
        ts, ss = polyak_tensors()
        before = [t.copy() for t in ts]
        lead = [float(t.base[0]) for t in ts]                     # the element in front of the odd-offset view, and of the others
        n = len(ts)
        dst = (C.c_void_p * n)(*[t.ctypes.data for t in ts])
        src = (C.c_void_p * n)(*[s.ctypes.data for s in ss])
        cnt = (C.c_int64 * n)(*[len(t) for t in ts])
        a = polyak_args(n, C.addressof(dst), C.addressof(src), C.addressof(cnt), max(len(t) for t in ts), tau)
        host.sachost_polyak(C.addressof(a))
        for t, s, b, l0 in zip(ts, ss, before, lead):
            assert same_u32(t, np_polyak(b, s, tau)), (tau, len(t))
            if len(t) == 257:
                assert float(t.base[0]) == l0 and t.ctypes.data % 8 == 4
            else:
                assert same_u32(t.base[len(t):], np.asarray(t.base[len(t):]))
        if tau == 1.0:
            assert all(same_u32(t, s) for t, s in zip(ts, ss))
        if tau == 0.0:
            assert all(same_u32(t, b) for t, b in zip(ts, before))


# ---- 4. against autograd ---------------------------------------------------------------------------------------------------------------
def test_sample_gradients_against_float64_autograd(host):
    """Bounds: the module's docstring.  Figures of this run are printed before they are asserted."""
    import torch
    M = 4096
    c = RowsCase(M, seed=0)
    i = grad_inputs(host, c, seed=7)
    got = host_grad(host, i)
    g32m, g32s = got["grad_mean"][:M].astype(np.float64), got["grad_log_std"][:M].astype(np.float64)
    near = (np.abs(c.log_std_in - f(-20)) < 1e-4) | (np.abs(c.log_std_in - f(2)) < 1e-4)
    doubtful = near.any(axis=1)
    print(f"rows left out: {int(doubtful.sum())} of {M}")
    assert doubtful.mean() <= 0.01
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    mean, log_std = T(c.mean_in).requires_grad_(), T(c.log_std_in).requires_grad_()
    e = T(i["eps"])
    ls = torch.clamp(log_std, -20.0, 2.0)
    std = ls.exp()
    u = mean + std * e
    a = torch.tanh(u)
    logp = torch.distributions.Normal(mean, std).log_prob(u).sum(-1) - torch.log(1 - a ** 2 + 1e-6).sum(-1)
    ((a * T(i["grad_action"])).sum() + (logp * T(i["grad_logp"])).sum()).backward()
    g64m, g64s = mean.grad.numpy(), log_std.grad.numpy()
    with torch.no_grad():
        A, S, G, sd = a.numpy(), (std * e).numpy(), (1 - a ** 2).numpy(), std.numpy()
        ga, gl = np.abs(i["grad_action"].astype(np.float64)), np.abs(i["grad_logp"].astype(np.float64))[:, None]
        du = np.abs(S) * (2.0 ** -23 + U) + U * np.abs(u.numpy())
        da = 1.01 * G * du + 2.0 ** -23
        dg = 2 * np.abs(A) * da + 2 * U
        g_lo = np.maximum(G - dg, 0.0)
        t4 = 2 * A * G / (G + 1e-6)
        dt4 = (2 * np.abs(A) * 1e-6 / (g_lo + 1e-6) ** 2) * dg + (2 * G / (G + 1e-6)) * da + 5 * U * np.abs(t4)
        # the float64 chain's own error, grad_log_std only (the docstring's ref): x = u - mean against std e
        EA = np.abs(e.numpy())
        dx = 2.0 ** -53 * (np.abs(u.numpy()) + np.abs(S))
        ref = gl * (EA * (dx + 2.0 ** -53 * np.abs(S)) / sd + 8 * 2.0 ** -53 * EA ** 2)
        gu = g64m
        dgu = ga * dg + U * ga * G + gl * dt4 + U * gl * np.abs(t4) + U * np.abs(gu)
        dgls = dgu * np.abs(S) + 3 * U * np.abs(gu * S) + U * np.abs(g64s) + ref
    k = ~doubtful
    inside = ((c.log_std_in >= -20) & (c.log_std_in <= 2))
    err_m, err_s = np.abs(g32m - g64m), np.abs(g32s - g64s)
    well = dgu < 1e-4
    print(f"grad_mean: largest error / bound {np.max(err_m[k] / dgu[k]):.3f}; elements with a bound below 1e-4: {well[k].mean():.3f}, their largest "
          f"error {err_m[k][well[k]].max():.3e}; largest |gradient| {np.abs(g64m).max():.3e}")
    print(f"grad_log_std: largest error / bound {np.max(err_s[k][inside[k]] / dgls[k][inside[k]]):.3f}")
    assert (err_m[k] <= dgu[k]).all()
    assert (err_s[k] <= dgls[k] * inside[k]).all()               # outside the clamp both sides are exactly 0
    assert well[k].mean() > 0.9                                  # the bound is a tight one on a good share of the elements


def test_loss_gradients_against_float64_autograd(host):
    import torch
    M, gamma, te = 4096, 0.9631, -6.0
    c = LossCase(M, seed=0)
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    alpha = float(c.alpha[0])
    # critic stage: stable_baselines3's 0.5 * sum of the two mse losses against a target formed under no_grad
    got = host_loss(host, c, 0)
    q1, q2 = T(c.q1).requires_grad_(), T(c.q2).requires_grad_()
    with torch.no_grad():
        m = torch.min(T(c.q1_next), T(c.q2_next))
        y = T(c.reward) + (1 - T(c.done)) * gamma * (m - alpha * T(c.logp))
    loss = 0.5 * (torch.nn.functional.mse_loss(q1, y) + torch.nn.functional.mse_loss(q2, y))
    loss.backward()
    dy = 5 * U * (np.abs(c.reward) + np.abs(m.numpy()) + np.abs(alpha * c.logp)).astype(np.float64)
    assert (np.abs(got["target_out"][:M] - y.numpy()) <= dy).all()
    for name, q in (("grad_q1", q1), ("grad_q2", q2)):
        err, bound = np.abs(got[name][:M] - q.grad.numpy()), dy / M + 3 * U * np.abs(q.grad.numpy())
        print(f"{name}: largest error / bound {np.max(err / bound):.3f}, largest |gradient| {np.abs(q.grad.numpy()).max():.3e}")
        assert (err <= bound).all(), name
    # the loss: 0.5 mean d^2 over both critics, d = q - y off by dy and its own rounding, the square by one more
    d1, d2 = np.abs(c.q1 - y.numpy()), np.abs(c.q2 - y.numpy())
    loss_bound = float(((d1 + d2) * dy).mean() + 4 * U * float(loss.detach()))
    print(f"critic loss: {got['stats'][0]:.9f} against {float(loss.detach()):.9f}, bound {loss_bound:.2e}")
    assert abs(got["stats"][0] - float(loss.detach())) <= loss_bound
    # actor stage and the entropy coefficient
    got = host_loss(host, c, 1, target_entropy=te)
    doubtful = np.abs(c.q1.astype(np.float64) - c.q2) < 1e-4
    print(f"rows left out: {int(doubtful.sum())} of {M}")
    assert doubtful.mean() <= 0.01
    q1, q2, logp = T(c.q1).requires_grad_(), T(c.q2).requires_grad_(), T(c.logp).requires_grad_()
    log_alpha = T(c.log_alpha).requires_grad_()
    (alpha * logp - torch.min(q1, q2)).mean().backward()
    (-(log_alpha * (logp.detach() + te)).mean()).backward()
    k, w = ~doubtful, 1.0 / M
    assert (np.abs(got["grad_q1"][:M] - q1.grad.numpy())[k] <= U * w).all() and (np.abs(got["grad_q2"][:M] - q2.grad.numpy())[k] <= U * w).all()
    assert (np.abs(got["grad_logp"][:M] - logp.grad.numpy()) <= 2 * U * w * alpha).all()
    g = float(log_alpha.grad[0])
    bound = U * float(np.abs(c.logp.astype(np.float64) + te).mean()) + U * abs(g)
    print(f"grad_log_alpha: {got['grad_log_alpha'][0]:.7f} against {g:.7f}, bound {bound:.2e}")
    assert abs(float(got["grad_log_alpha"][0]) - g) <= bound and abs(got["stats"][2] - g) <= bound


# ---- 5. refusals without a device ------------------------------------------------------------------------------------------------------
P_ = 0x10000                                                  # a non-null pointer: never followed, nothing is launched
MB_ = 0x100000                                                # the distance between two of them
NAN, INF = float("nan"), float("inf")


def good_rows_args():
    from gl_gym_amd import _lib as L
    p = [P_ + k * MB_ for k in range(14)]
    return L.make_plan_args(L.SacRowsArgs, 130, 23, 0, 0, 0, 0, p[0], p[1], 1, 0, None, 0.05, p[2], *p[3:13])


def good_grad_args():
    from gl_gym_amd import _lib as L
    return L.make_plan_args(L.SacRowsGradArgs, 130, *[P_ + k * MB_ for k in range(8)])


def good_batch_args():
    from gl_gym_amd import _lib as L
    p = [P_ + k * MB_ for k in range(10)]
    return L.make_plan_args(L.SacBatchArgs, 4, 130, 23, 200, 1, 3, 0, 1, 0, None, *p)


def good_loss_args(stage=0):
    from gl_gym_amd import _lib as L
    p = [P_ + k * MB_ for k in range(16)]
    return L.make_plan_args(L.SacLossArgs, 130, stage, 0, *p[:9], 0.99, -6.0, *p[9:16], L.SAC_LOSS_WS_BYTES)


def good_polyak_args():
    return polyak_args(64, P_, P_ + MB_, P_ + 2 * MB_, 1000, 0.005)


ROWS_REFUSALS = [("struct_size", 8, b"struct_size"), ("M", 0, b"M < 1"), ("M", -5, b"M < 1"), ("M", 2 ** 31 - 255, b"2^31 - 256 rows"),
                 ("step", -1, b"step outside"), ("step", 2 ** 30, b"step outside"), ("row0", -1, b"row0 < 0"), ("row0", 2 ** 32 - 129, b"row0 + M > 2^32"),
                 ("deterministic", 2, b"must be 0 or 1"), ("uniform", -1, b"must be 0 or 1"), ("action_noise_sigma", -0.1, b"action_noise_sigma"),
                 ("action_noise_sigma", NAN, b"action_noise_sigma"), ("action_noise_sigma", INF, b"action_noise_sigma"),
                 ("mean_in", None, b"null mean_in"), ("log_std_in", None, b"null mean_in"), ("in_dim", 0, b"in_dim outside"),
                 ("in_dim", 1025, b"in_dim outside"), ("obs", None, b"null obs"), ("obs_out", P_ + 2 * MB_ + 130 * 23 * 4 - 4, b"overlaps an input"),
                 ("action", P_, b"overlaps an input"), ("logp", P_ + MB_ + 130 * 24 - 4, b"overlaps an input"),
                 ("eps", P_ + 4 * MB_ + 130 * 24 - 4, b"overlaps another output"), ("corr", P_ + 7 * MB_ + 516, b"overlaps another output"), ("eps2", P_ + 8 * MB_ + 4, b"overlaps another output")]
GRAD_REFUSALS = [("struct_size", 4, b"struct_size"), ("M", 0, b"M < 1"), ("M", 2 ** 31 - 255, b"2^31 - 256 rows")] + \
                [(k, None, b"null grad_action") for k in ("grad_action", "grad_logp", "eps", "std", "tanh", "log_std_in")] + \
                [("grad_mean", None, b"null grad_mean"), ("grad_log_std", None, b"null grad_mean"), ("grad_mean", P_ + 130 * 24 - 4, b"overlaps an input"),
                 ("grad_log_std", P_ + MB_ + 516, b"overlaps an input"), ("grad_log_std", P_ + 6 * MB_ + 130 * 24 - 4, b"overlaps another output")]
BATCH_REFUSALS = [("struct_size", 8, b"struct_size"), ("S", 1, b"S < 2"), ("B", 0, b"B < 1"), ("S", 2 ** 24, b"S * B > 2^31 - 1"), ("M", 0, b"M < 1"),
                  ("M", 2 ** 31 - 255, b"2^31 - 256 rows"), ("in_dim", 0, b"in_dim outside"), ("in_dim", 1025, b"in_dim outside"),
                  ("head", -1, b"head outside"), ("head", 4, b"head outside"), ("n_valid", 0, b"n_valid < 1"), ("n_valid", -2, b"n_valid < 1"),
                  ("n_valid", 4, b"without a successor"), ("n_valid", 9, b"without a successor")] + \
                 [(k, None, b"null obs") for k in ("obs", "action", "reward", "done")] + \
                 [(k, None, b"null mb_obs") for k in ("mb_obs", "mb_next_obs", "mb_action", "mb_reward", "mb_done")] + \
                 [("mb_obs", P_ + 4 * 130 * 23 * 4 - 4, b"overlaps a source"), ("mb_done", P_ + 3 * MB_ + 519, b"overlaps a source"),
                  ("index_out", P_ + 2 * MB_, b"overlaps a source"), ("mb_next_obs", P_ + 4 * MB_ + 200 * 23 * 4 - 4, b"overlaps another output"),
                  ("index_out", P_ + 8 * MB_ + 199, b"overlaps another output")]
LOSS_REFUSALS = {0: [("struct_size", 4, b"struct_size"), ("M", 0, b"M < 1"), ("M", 2 ** 31 - 255, b"2^31 - 256 rows"), ("stage", 2, b"stage must be"),
                     ("stage", -1, b"stage must be"), ("gamma", -0.1, b"gamma outside"), ("gamma", 1.5, b"gamma outside"), ("gamma", NAN, b"gamma outside"),
                     ("q1", None, b"null q1"), ("q2", None, b"null q1"), ("logp", None, b"null q1"), ("alpha", None, b"null q1"),
                     ("grad_q1", None, b"null grad_q1"), ("grad_q2", None, b"null grad_q1"), ("stats", None, b"null grad_q1"),
                     ("q1_next", None, b"critic stage with a null"), ("q2_next", None, b"critic stage with a null"), ("reward", None, b"critic stage with a null"),
                     ("done", None, b"critic stage with a null"), ("workspace", None, b"null workspace"), ("workspace_bytes", 40959, b"workspace smaller"),
                     ("workspace_bytes", 0, b"workspace smaller"), ("grad_q1", P_ + 516, b"overlaps an input"), ("target_out", P_ + 6 * MB_ + 129, b"overlaps an input"),
                     ("stats", P_ + 7 * MB_, b"overlaps an input"), ("workspace", P_ + 5 * MB_, b"overlaps an input"),
                     ("grad_q2", P_ + 9 * MB_ + 516, b"overlaps another output"), ("stats", P_ + 15 * MB_ + 40960 - 8, b"overlaps another output")],
                 1: [("target_entropy", NAN, b"target_entropy not finite"), ("target_entropy", INF, b"target_entropy not finite"),
                     ("log_alpha", None, b"actor stage with a null"), ("grad_logp", None, b"actor stage with a null"),
                     ("grad_logp", P_ + 8 * MB_, b"overlaps an input"), ("grad_log_alpha", P_ + 7 * MB_ + 3, b"overlaps an input"),
                     ("grad_log_alpha", P_ + 11 * MB_ + 516, b"overlaps another output")]}
POLYAK_REFUSALS = [("struct_size", 8, b"struct_size"), ("n", 0, b"n < 1"), ("n", 65, b"more than 64 tensors"), ("dst", None, b"null dst"),
                   ("src", None, b"null dst"), ("count", None, b"null dst"), ("tau", -0.1, b"tau outside"), ("tau", 1.5, b"tau outside"),
                   ("tau", NAN, b"tau outside"), ("max_count", -1, b"max_count < 0")]


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
    table = [("glgym_sac_rows", good_rows_args, ROWS_REFUSALS), ("glgym_sac_rows_grad", good_grad_args, GRAD_REFUSALS),
             ("glgym_sac_batch", good_batch_args, BATCH_REFUSALS), ("glgym_sac_loss", good_loss_args, LOSS_REFUSALS[0]),
             ("glgym_sac_loss", lambda: good_loss_args(1), LOSS_REFUSALS[1]), ("glgym_polyak", good_polyak_args, POLYAK_REFUSALS)]
    for name, good, refusals in table:
        fn = getattr(lib, name)
        refused(lib, fn, None, good(), f"{name}: null handle".encode())
        for path, value, word in refusals:
            a = good()
            set_path(a, path, value)
            refused(lib, fn, None, a, word)
            assert name.encode() in lib.glgym_last_error(), (name, path)
        assert fn(None, None, None) == L.EINVAL
    # glgym_sac_rows: no output at all; both modes; uniform needs neither mean nor log_std but refuses what it cannot write
    a = good_rows_args()
    for k in ROWS_OUT:
        setattr(a, k, None)
    refused(lib, lib.glgym_sac_rows, None, a, b"no output")
    a = good_rows_args()
    a.deterministic = a.uniform = 1
    refused(lib, lib.glgym_sac_rows, None, a, b"both set")
    a = good_rows_args()
    a.uniform = 1
    refused(lib, lib.glgym_sac_rows, None, a, b"uniform with a logp")
    a.logp = a.eps = a.eps2 = a.std = a.tanh = a.corr = a.mean_in = a.log_std_in = None
    refused(lib, lib.glgym_sac_rows, None, a, b"null handle")
    a = good_rows_args()                                          # without obs_out neither obs nor in_dim is asked for
    a.obs_out, a.obs, a.in_dim = None, None, 0
    refused(lib, lib.glgym_sac_rows, None, a, b"null handle")
    a = good_rows_args()
    a.row0 = 2 ** 32 - 130                                        # the last key is 2^32 - 1
    refused(lib, lib.glgym_sac_rows, None, a, b"null handle")
    # glgym_sac_batch: n_valid = S - 1 is the full ring; glgym_sac_loss: each stage leaves the other's pointers alone
    a = good_batch_args()
    a.index_out, a.head = None, 3
    refused(lib, lib.glgym_sac_batch, None, a, b"null handle")
    a = good_loss_args(0)
    a.log_alpha = a.grad_logp = a.grad_log_alpha = a.target_out = None
    a.target_entropy = NAN
    refused(lib, lib.glgym_sac_loss, None, a, b"null handle")
    a = good_loss_args(1)
    a.q1_next = a.q2_next = a.reward = a.done = a.target_out = a.grad_log_alpha = None
    a.gamma = NAN
    refused(lib, lib.glgym_sac_loss, None, a, b"null handle")
    a = good_polyak_args()
    a.max_count = 0
    refused(lib, lib.glgym_polyak, None, a, b"null handle")


def test_sac_refuses_what_is_out_of_scope():
    import gl_gym_amd
    for kw in (dict(use_sde=True), dict(n_critics=3), dict(n_critics=1), dict(learning_rate=lambda p: 3e-4), dict(recurrent=True),
               dict(prioritized_replay=True)):
        with pytest.raises(NotImplementedError):                  # the constructor's checks come before anything is looked at
            gl_gym_amd.SAC(None, None, None, None, None, **kw)
    for kw in (dict(gamma=1.5), dict(tau=-0.1), dict(batch_size=0), dict(target_update_interval=0), dict(ent_coef="fixed"), dict(ent_coef=0.0)):
        with pytest.raises(ValueError):
            gl_gym_amd.SAC(None, None, None, None, None, **kw)


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """tests/sachost/sachost.cpp with its own main, AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (nothing is
    loaded into Python): exactly sized heap buffers, so an index past a ring row, a minibatch row or the stated workspace is reported."""
    exe = tmp_path / "sachost_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DSACHOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sachost ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
