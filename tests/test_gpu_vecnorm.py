"""glgym_vecnorm (vecnorm_moments / returns / merge / apply / reward kernels) against oracle/vecnorm_oracle.py, called through
ctypes on caller-owned tensors: every launch geometry of the entry point (tests/ancillary_inputs.py VN_SHAPES), its modes, its
refusals, and columns whose mean dwarfs their spread.  Every output buffer carries guard elements behind it and the workspace
starts from a sentinel pattern; every element of every result is compared, at the tolerances of
tests/test_gpu_env_api.py::test_vecnormalize_on_device_matches_sb3_algorithm."""
import ctypes as C

import numpy as np
import pytest

import ancillary_inputs as A

pytestmark = pytest.mark.gpu

PAD = 67                      # guard elements behind every buffer the entry point writes
G32, G64, WS_FILL = -7.7725e5, -3.25e200, 3.0e33
EPS = 1e-8


class Handle:
    """A glgym handle made as WeatherPipeline makes its own; dtype decides how ``reward`` is read."""

    def __init__(self, f64):
        import torch
        from gl_gym_amd import _lib as L
        from gl_gym_amd.parameters import init_default_params
        self.t, self.L, self.f64, self.dev = torch, L, f64, torch.device("cuda:0")
        self.lib, self.h = L.load(), C.c_void_p()
        p = np.ascontiguousarray(init_default_params(L.NP), dtype=np.float64)
        L.check(self.lib.glgym_create(L.NX, L.NU, L.ND, L.NP, 900.0, p.ctypes.data_as(L._DP), L.F64 if f64 else L.F32, 4, 0,
                                      C.byref(self.h)), "glgym_create")

    def close(self):
        self.lib.glgym_destroy(self.h)


@pytest.fixture(scope="module")
def handles():
    import torch
    assert torch.cuda.is_available()
    hs = {False: Handle(False), True: Handle(True)}
    yield hs
    for h in hs.values():
        h.close()


class Buffers:
    """Caller-owned tensors of one VecNormalize instance.  obs_out, reward_out, returns, obs_mean and obs_var are the front of
    longer allocations whose tail holds a sentinel."""

    def __init__(self, hd, B, dim, mean=None, var=None, count=1e-4, ret_stats=(0.0, 1.0, 1e-4), returns=None):
        t, dev = hd.t, hd.dev
        self.hd, self.B, self.dim = hd, B, dim
        f64 = dict(dtype=t.float64, device=dev)
        self.obs_out = t.full((B * dim + PAD,), G32, dtype=t.float32, device=dev)
        self.reward_out = t.full((B + PAD,), G32, dtype=t.float32, device=dev)
        self.returns = t.full((B + PAD,), G64, **f64)
        self.returns[:B] = 0.0 if returns is None else t.as_tensor(returns, **f64)
        self.mean = t.full((dim + PAD,), G64, **f64)
        self.var = t.full((dim + PAD,), G64, **f64)
        self.mean[:dim] = 0.0 if mean is None else t.as_tensor(np.asarray(mean, dtype=np.float64), **f64)
        self.var[:dim] = 1.0 if var is None else t.as_tensor(np.asarray(var, dtype=np.float64), **f64)
        self.count = t.full((1 + PAD,), G64, **f64)
        self.count[0] = count
        self.ret_stats = t.full((3 + PAD,), G64, **f64)
        self.ret_stats[:3] = t.tensor(ret_stats, **f64)
        self.ws = t.empty(32 * dim + 2 + PAD, **f64)

    def call(self, obs, reward=None, done=None, *, in_place=False, training=1, norm_obs=1, norm_reward=1, gamma=0.99,
             clip_obs=10.0, clip_reward=10.0, expect=0, override=None):
        """One glgym_vecnorm call on host arrays.  -> obs_out [B, dim] (float32, from ``obs`` itself when in_place)."""
        hd, t, B, dim = self.hd, self.hd.t, self.B, self.dim
        self.obs_t = t.as_tensor(np.ascontiguousarray(obs, dtype=np.float32), device=hd.dev).reshape(-1)
        if in_place:                               # obs_out == obs: the rows live in the guarded buffer
            self.obs_out[:B * dim] = self.obs_t
            self.obs_t = self.obs_out
        self.rew_t = None if reward is None else t.as_tensor(
            np.ascontiguousarray(reward, dtype=np.float64 if hd.f64 else np.float32), device=hd.dev)
        self.done_t = None if done is None else t.as_tensor(np.ascontiguousarray(done, dtype=np.uint8), device=hd.dev)
        self.ws.fill_(WS_FILL)                     # the entry point clears what it uses
        ptr = dict(obs=self.obs_t.data_ptr(), obs_out=self.obs_out.data_ptr(),
                   reward=None if self.rew_t is None else self.rew_t.data_ptr(), reward_out=self.reward_out.data_ptr(),
                   done=None if self.done_t is None else self.done_t.data_ptr(), obs_mean=self.mean.data_ptr(),
                   obs_var=self.var.data_ptr(), obs_count=self.count.data_ptr(), ret_stats=self.ret_stats.data_ptr(),
                   returns=self.returns.data_ptr(), workspace=self.ws.data_ptr())
        dims = dict(B=B, dim=dim)
        for k, v in (override or {}).items():
            (dims if k in dims else ptr)[k] = v
        a = hd.L.VecNormArgs(dims["B"], dims["dim"], ptr["obs"], ptr["obs_out"], ptr["reward"], ptr["reward_out"], ptr["done"],
                             ptr["obs_mean"], ptr["obs_var"], ptr["obs_count"], ptr["ret_stats"], ptr["returns"],
                             ptr["workspace"], gamma, EPS, clip_obs, clip_reward, int(training), int(norm_obs),
                             int(norm_reward))
        t.cuda.synchronize()
        rc = hd.lib.glgym_vecnorm(hd.h, C.byref(a), C.c_void_p(t.cuda.current_stream(hd.dev).cuda_stream))
        t.cuda.synchronize()
        assert rc == expect, (rc, hd.lib.glgym_last_error().decode())
        return self.obs_out[:B * dim].cpu().numpy().reshape(B, dim)

    def snapshot(self):
        return {k: getattr(self, k).clone() for k in ("obs_out", "reward_out", "returns", "mean", "var", "count", "ret_stats", "ws")}

    def assert_unchanged(self, snap, keys=None):
        for k in keys or snap:
            assert self.hd.t.equal(getattr(self, k), snap[k]), f"{k} changed"

    def assert_guards(self):
        B, dim = self.B, self.dim
        for name, buf, n, g in (("obs_out", self.obs_out, B * dim, G32), ("reward_out", self.reward_out, B, G32),
                                ("returns", self.returns, B, G64), ("obs_mean", self.mean, dim, G64),
                                ("obs_var", self.var, dim, G64), ("obs_count", self.count, 1, G64),
                                ("ret_stats", self.ret_stats, 3, G64), ("workspace", self.ws, 32 * dim + 2, WS_FILL)):
            tail = buf[n:].cpu().numpy()
            assert tail.size == PAD and np.all(tail == tail.dtype.type(g)), f"guard behind {name} was written"

    def stats(self):
        return (self.mean[:self.dim].cpu().numpy(), self.var[:self.dim].cpu().numpy(), float(self.count[0]),
                self.ret_stats[:3].cpu().numpy(), self.returns[:self.B].cpu().numpy())


def check_against(buf, orc, obs_n=None, ref_obs=None, rew_ref=None, what=""):
    mean, var, count, ret, returns = buf.stats()
    cl = np.testing.assert_allclose
    if ref_obs is not None:
        cl(obs_n, ref_obs, *A.VN_TOL["obs"], err_msg=f"{what}: normalised observations")
    if rew_ref is not None:
        cl(buf.reward_out[:buf.B].cpu().numpy(), rew_ref, *A.VN_TOL["reward"], err_msg=f"{what}: rewards")
    cl(mean, orc.obs_rms.mean, *A.VN_TOL["mean"], err_msg=f"{what}: running mean")
    cl(var, orc.obs_rms.var, *A.VN_TOL["var"], err_msg=f"{what}: running variance")
    assert abs(count - orc.obs_rms.count) < A.VN_COUNT_ATOL, what
    cl(ret[0], orc.ret_rms.mean, *A.VN_TOL["mean"], err_msg=f"{what}: return mean")
    assert abs(ret[1] - orc.ret_rms.var) < 1e-9 * max(1.0, orc.ret_rms.var), what      # as the existing test states it
    assert abs(ret[2] - orc.ret_rms.count) < A.VN_COUNT_ATOL, what
    cl(returns, orc.returns, *A.VN_TOL["returns"], err_msg=f"{what}: returns")
    buf.assert_guards()


def _oracle(B, dim, **kw):
    from oracle.vecnorm_oracle import VecNormalizeOracle
    return VecNormalizeOracle(B, dim, epsilon=EPS, **kw)


def _rew_in(hd, reward):
    """The reward as the handle's dtype carries it, widened for the oracle."""
    return np.asarray(reward, dtype=np.float64 if hd.f64 else np.float32).astype(np.float64)


@pytest.mark.parametrize("B,dim", A.VN_SHAPES, ids=[f"B{b}-dim{d}" for b, d in A.VN_SHAPES])
def test_every_launch_geometry_three_merges_from_cold(handles, B, dim):
    """A reset call and two step calls with fresh data: the statistics are merged twice on top of the cold start."""
    hd = handles[False]
    clip = A.vn_clip_obs(B)
    buf, orc = Buffers(hd, B, dim), _oracle(B, dim, clip_obs=clip, gamma=0.9631)
    for call in range(A.VN_N_CALLS):
        obs, rew, done = A.vn_batch(B, dim, call)
        if call == 0:                                # the reset call: reward = NULL
            got = buf.call(obs, clip_obs=clip, gamma=0.9631)
            ref_o, ref_r = orc.reset(obs.astype(np.float64)), None
        else:
            got = buf.call(obs, rew, done, clip_obs=clip, gamma=0.9631)
            ref_o, ref_r = orc.step(obs.astype(np.float64), _rew_in(hd, rew), done)
        check_against(buf, orc, got, ref_o, ref_r, f"B={B} dim={dim} call {call}")
        assert np.abs(got).max() <= clip


MODES = ["reset", "no_done", "done_lanes", "eval", "copy", "copy_in_place", "norm_in_place", "cast_reward", "f64",
         "gamma0", "gamma1"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,dim", A.VN_MODE_SHAPES, ids=[f"B{b}-dim{d}" for b, d in A.VN_MODE_SHAPES])
def test_modes(handles, B, dim, mode):
    hd = handles[mode == "f64"]
    t = hd.t
    gamma = {"gamma0": 0.0, "gamma1": 1.0}.get(mode, 0.9631)
    kw = dict(clip_obs=10.0, gamma=gamma)
    okw = dict(kw)
    # warm everything with one ordinary step, so that each mode starts from statistics and returns that are not the defaults
    obs0, rew0, done0 = A.vn_batch(B, dim, 0)
    obs, rew, done = A.vn_batch(B, dim, 1)
    buf, orc = Buffers(hd, B, dim), _oracle(B, dim, **okw)
    buf.call(obs0, rew0, done0 & False, **kw)
    orc.step(obs0.astype(np.float64), _rew_in(hd, rew0), done0 & False)
    check_against(buf, orc, what=f"{mode}: warm-up")
    assert np.all(orc.returns != 0.0)
    snap = buf.snapshot()
    o64 = obs.astype(np.float64)
    if mode == "reset":                              # reward = NULL: the returns and their statistics stay untouched
        got = buf.call(obs, **kw)
        if orc.training and orc.norm_obs:
            orc.obs_rms.update(o64)
        check_against(buf, orc, got, orc.normalize_obs(o64), what=mode)
        buf.assert_unchanged(snap, ("returns", "ret_stats", "reward_out"))
    elif mode == "no_done":
        got = buf.call(obs, rew, None, **kw)
        ref_o, ref_r = orc.step(o64, _rew_in(hd, rew), np.zeros(B, bool))
        check_against(buf, orc, got, ref_o, ref_r, mode)
        assert np.all(buf.returns[:B].cpu().numpy() != 0.0)
    elif mode == "done_lanes":                       # lane 0, last lane of wave 0, lane 0 of wave 1, the last env -- and only those
        d = np.zeros(B, bool)
        d[[0, 63, 64, B - 1]] = True
        got = buf.call(obs, rew, d, **kw)
        ref_o, ref_r = orc.step(o64, _rew_in(hd, rew), d)
        check_against(buf, orc, got, ref_o, ref_r, mode)
        assert np.array_equal(buf.returns[:B].cpu().numpy() == 0.0, d)
    elif mode == "eval":                             # training = 0 on LOADED statistics: bit-identical after, rows normalised
        mean, var, count = A.vn_eval_stats(dim, EPS)
        buf = Buffers(hd, B, dim, mean, var, count, ret_stats=(0.5, 7.0, 99.0), returns=np.arange(1.0, B + 1))
        snap = buf.snapshot()
        orc.obs_rms.mean, orc.obs_rms.var, orc.obs_rms.count = mean, var, count
        orc.training = False
        rows = A.vn_eval_batch(B, dim, 10.0)
        got = buf.call(rows, rew, done, training=0, **kw)
        buf.assert_unchanged(snap, ("mean", "var", "count", "ret_stats"))
        ref = orc.normalize_obs(rows.astype(np.float64))
        np.testing.assert_allclose(got, ref, *A.VN_TOL["obs"])
        # scale is exactly 1/2 and the means whole numbers: the rows placed on and beside the clip come out exact
        assert np.array_equal(got[:6], ref[:6]) and np.all(got[0] == 10.0) and np.all(got[1] == -10.0)
        assert np.all(got[3] < 10.0) and np.all(got[4] > -10.0) and np.all(got[2] == 10.0) and np.all(got[5] == -10.0)
        rr = _rew_in(hd, rew)
        np.testing.assert_allclose(buf.reward_out[:B].cpu().numpy(), np.clip(rr / np.sqrt(7.0 + EPS), -10, 10), *A.VN_TOL["reward"])
        want_ret = np.where(done, 0.0, np.arange(1.0, B + 1))          # no accumulation, but finished envs still reset
        assert np.array_equal(buf.returns[:B].cpu().numpy(), want_ret)
        buf.assert_guards()
    elif mode in ("copy", "copy_in_place"):          # norm_obs = 0: rows pass through bit for bit, obs statistics untouched
        got = buf.call(obs, rew, done, norm_obs=0, in_place=(mode == "copy_in_place"), **kw)
        assert np.array_equal(got.view(np.uint32), obs.view(np.uint32))
        buf.assert_unchanged(snap, ("mean", "var", "count"))
        orc.norm_obs = False
        _, ref_r = orc.step(o64, _rew_in(hd, rew), done)
        check_against(buf, orc, rew_ref=ref_r, what=mode)
        if mode == "copy":
            assert np.array_equal(buf.obs_t.cpu().numpy().view(np.uint32), obs.reshape(-1).view(np.uint32))
    elif mode == "norm_in_place":
        got = buf.call(obs, rew, done, in_place=True, **kw)
        ref_o, ref_r = orc.step(o64, _rew_in(hd, rew), done)
        check_against(buf, orc, got, ref_o, ref_r, mode)
    elif mode == "cast_reward":                      # norm_reward = 0: the reward is only cast; its statistics still update
        got = buf.call(obs, rew, done, norm_reward=0, **kw)
        orc.norm_reward = False
        ref_o, ref_r = orc.step(o64, _rew_in(hd, rew), done)
        check_against(buf, orc, got, ref_o, what=mode)
        assert np.array_equal(buf.reward_out[:B].cpu().numpy(), _rew_in(hd, rew).astype(np.float32))
    else:                                            # f64 (fp64 rewards the fp32 path would round), gamma0, gamma1
        if mode == "f64":
            rew = rew * (1.0 + 2.0 ** -40)           # not representable in float32
            assert np.any(rew.astype(np.float32).astype(np.float64) != rew)
        got = buf.call(obs, rew, done, **kw)
        ref_o, ref_r = orc.step(o64, _rew_in(hd, rew), done)
        check_against(buf, orc, got, ref_o, ref_r, mode)
    if mode not in ("copy_in_place", "norm_in_place"):
        assert t.equal(buf.obs_t.cpu(), t.as_tensor((rows if mode == "eval" else obs).reshape(-1))), "the input rows were written"


REFUSALS = [("B", 0), ("B", -3), ("dim", 0), ("dim", -1), ("obs", None), ("obs_out", None), ("obs_mean", None),
            ("obs_var", None), ("obs_count", None), ("workspace", None), ("reward_out", None), ("ret_stats", None),
            ("returns", None)]


@pytest.mark.parametrize("field,value", REFUSALS, ids=[f"{f}={v}" for f, v in REFUSALS])
def test_refusals_change_nothing(handles, field, value):
    hd = handles[False]
    B, dim = 65, 63
    obs, rew, done = A.vn_batch(B, dim, 0)
    buf = Buffers(hd, B, dim)
    buf.ws.fill_(WS_FILL)
    snap = buf.snapshot()
    buf.call(obs, rew, done, expect=hd.L.EINVAL, override={field: value})
    buf.assert_unchanged(snap)
    assert np.array_equal(buf.obs_t.cpu().numpy(), obs.reshape(-1))
    assert hd.lib.glgym_vecnorm(None, None, None) == hd.L.EINVAL


@pytest.mark.parametrize("warm", [False, True], ids=["cold", "warm"])
@pytest.mark.parametrize("B", A.ILL_BATCHES)
def test_ill_conditioned_columns(handles, B, warm):
    """Columns whose mean is up to 1e7 spreads from zero, and a constant one: the batch variance has to come from a
    well-conditioned pass.  Taken as E[x^2] - E[x]^2 about zero in fp64 (the kernels before the pivot), the running variance
    left the tolerance by the factors recorded in profiles/vecnorm_moments_cost.txt; `warm` starts from the columns' exact
    statistics with a count of ten batches, where no cold-start term hides the batch variance and the error reaches the
    normalised rows."""
    hd = handles[False]
    obs = A.ill_batch(B)
    dim = obs.shape[1]
    orc = _oracle(B, dim)
    if warm:
        m, v, c = A.ill_warm_stats(obs)
        orc.obs_rms.mean, orc.obs_rms.var, orc.obs_rms.count = m, v, c
        buf = Buffers(hd, B, dim, m, v, c)
    else:
        buf = Buffers(hd, B, dim)
    got = buf.call(obs)
    ref = orc.reset(obs.astype(np.float64))
    mean, var, count, _, _ = buf.stats()
    for j, (mu, s) in enumerate(A.ILL_COLUMNS):
        print(f"B={B} {'warm' if warm else 'cold'} column ({mu:g}, {s:g}): var {var[j]:.9e} oracle {orc.obs_rms.var[j]:.9e} "
              f"-> {A.tol_ratio(var[j], orc.obs_rms.var[j], *A.VN_TOL['var']):.3g} of tolerance; mean "
              f"{A.tol_ratio(mean[j], orc.obs_rms.mean[j], *A.VN_TOL['mean']):.3g}; rows "
              f"{A.tol_ratio(got[:, j], ref[:, j], *A.VN_TOL['obs']):.3g}")
    check_against(buf, orc, got, ref, what=f"B={B} warm={warm}")
    if warm:
        assert 0.0 <= var[A.ILL_CONST_COL] <= A.VN_TOL["var"][1]
