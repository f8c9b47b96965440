"""Rollout collection on the GPU: glgym_ac_rows, glgym_gae (include/glgym.h) and gl_gym_amd.collector.RolloutCollector.

What can be exact is compared bit for bit: the sample, the log-probability and GAE against the host instantiation of
csrc/gl_actor.hpp (tests/achost/achost.cpp) and the NumPy restatements of tests/test_collect_host.py; a captured graph against the eager
calls; collect() against a loop over its parts on an identically seeded environment.  The one thing that is not: the six normals are
made in double by the device's log / sqrt / cos / sin, which are not the host's -- eps is compared with the float64 Box-Muller
restatement within one float32 ulp, and what follows from it (action, logp) is compared exactly GIVEN the device's own eps.
Every output buffer has guard rows behind row B-1 and guard bytes around it (0xFF); an optional output that is not asked for and
every output of a refused call must come back untouched.  Batches stay <= 257 rows."""
import ctypes as C

import numpy as np
import pytest

import envlayer_inputs as E
from test_collect_host import (ALL_OUT, AC_REFUSALS, GAE_REFUSALS, GUARD, NU, AcCase, ac_args, build_host, case_arrays, gae_args, host_gae,
                               host_rows, make_gae_case, np_eps64, np_gae, np_rows, output_shapes, same_u32, set_path, within_one_f32_ulp)
from test_gpu_plan import make_env

pytestmark = pytest.mark.gpu
IN_DIMS = [1, 23, 64, 65, 130]


@pytest.fixture(scope="module")
def hd():
    h = E.Handle(False)
    yield h
    h.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("achost_gpu") / "libachost.so")


class DeviceCase:
    """The arrays of an AcCase on the device, each between guard bytes, and guarded outputs with GUARD rows behind row B-1."""

    def __init__(self, case):
        self.case = case
        self.inputs = {k: E.Guarded(v) for k, v in case_arrays(case).items()}
        self.outs = {k: E.Guarded(shape=(s[0] + GUARD,) + tuple(s[1:]), dtype=np.float32) for k, s in output_shapes(case).items()}

    def args(self, draw_base_ptr=None, **kw):
        return ac_args(self.case, lambda k: self.inputs[k].ptr, {k: v.ptr for k, v in self.outs.items()}, draw_base=draw_base_ptr, **kw)

    def read(self, written):
        """{name: rows < B} of the outputs in `written`; asserts every guard, and that the other outputs were not touched."""
        B, got = self.case.B, {}
        for g in self.inputs.values():
            g.read()
        for k, g in self.outs.items():
            v = g.read()
            if k in written:
                assert np.all(v[B:].view(np.uint8) == 0xFF), f"a guard row of {k} was written"
                got[k] = v[:B]
            else:
                assert np.all(v.view(np.uint8) == 0xFF), f"{k} was written"
        return got


def run_rows(hd, case, written=ALL_OUT, draw_base=None, **kw):
    dc = DeviceCase(case)
    base = None if draw_base is None else E.Guarded(np.array([draw_base], dtype=np.uint64))
    a = dc.args(None if base is None else base.ptr, **kw)
    hd.sync()
    rc = hd.lib.glgym_ac_rows(hd.h, C.byref(a), hd.stream())
    hd.sync()
    assert rc == 0, (rc, hd.error())
    return dc.read(written)


def same_named(got, want, names):
    for k in names:
        assert same_u32(got[k], want[k]), (k, np.abs(got[k] - want[k]).max())


# ---- 1. the stage kernel against the host build -------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130, 255, 256, 257])
def test_ac_rows_against_the_host_build(hd, host, B):
    kw = dict(step=4, seed=0xABCDEF0123, draw_index=5, draw_base=9)
    lean = ("action", "action_env", "logp", "value")
    for in_dim in IN_DIMS:
        case = AcCase(in_dim, B, seed=B)
        ref = {k: v[:B] for k, v in host_rows(host, case, **kw).items()}
        # stochastic: the device's own eps is within an ulp of the restatement and of the host's; given it, everything is exact
        got = run_rows(hd, case, **kw)
        assert within_one_f32_ulp(got["eps"], np_eps64(B, 4, 14, 0xABCDEF0123)), in_dim
        same_named(got, np_rows(case, got["eps"]), ALL_OUT)
        same_named(got, ref, ("obs_out", "value"))
        # the optional outputs left out
        got_lean = run_rows(hd, case, written=lean, want_obs_out=False, want_eps=False, **kw)
        same_named(got_lean, got, lean)
        # deterministic and value_only: no noise, the host build bit for bit
        det = run_rows(hd, case, deterministic=1, **kw)
        same_named(det, {k: v[:B] for k, v in host_rows(host, case, deterministic=1, **kw).items()}, ALL_OUT)
        assert not det["eps"].any()
        same_named(run_rows(hd, case, written=("value",), value_only=1, **kw), ref, ("value",))
    # env b's noise does not depend on B
    if B == 130:
        small = run_rows(hd, AcCase(23, 64, seed=1), **kw)
        big = run_rows(hd, AcCase(23, 130, seed=2), **kw)
        assert same_u32(small["eps"], big["eps"][:64])


def test_step_draw_base_and_seed_each_change_the_noise(hd):
    case = AcCase(23, 65)
    ref = run_rows(hd, case, step=3, seed=7, draw_index=10, draw_base=0)["eps"]
    assert same_u32(run_rows(hd, case, step=3, seed=7, draw_index=4, draw_base=6)["eps"], ref)           # D = draw_index + *draw_base
    assert same_u32(run_rows(hd, case, step=3, seed=7, draw_index=10)["eps"], ref)                      # draw_base NULL: 0
    for kw in (dict(step=4, seed=7, draw_index=10), dict(step=3, seed=8, draw_index=10), dict(step=3, seed=7, draw_index=10, draw_base=1),
               dict(step=3, seed=7 + 2 ** 32, draw_index=10), dict(step=3, seed=7, draw_index=10 + 2 ** 32)):
        assert not (run_rows(hd, case, **kw)["eps"] == ref).any(), kw


def test_nan_means_never_reach_the_env(hd):
    case = AcCase(23, 65)
    case.mean_in[::2] = np.nan
    got = run_rows(hd, case)
    assert np.isnan(got["action"][::2]).all() and (got["action_env"][::2] == -1).all() and np.isfinite(got["action"][1::2]).all()


def test_deterministic_action_is_the_mean(hd, host):
    case = AcCase(23, 65)
    det = run_rows(hd, case, deterministic=1)
    assert same_u32(det["action"], case.mean_in + np.float32(0))
    case.std = np.zeros(NU, dtype=np.float32)                    # a second, stochastic call with std = 0: a = mean + 0 * e
    assert same_u32(run_rows(hd, case)["action"], det["action"])


# ---- 2. GAE ---------------------------------------------------------------------------------------------------------------------------
def run_gae(hd, reward, done, value, last, gamma, lam):
    T, B = reward.shape
    ins = [E.Guarded(v) for v in (reward, done, value, last)]
    adv, ret = E.Guarded(shape=(T + GUARD, B), dtype=np.float32), E.Guarded(shape=(T + GUARD, B), dtype=np.float32)
    a = gae_args(T, B, *[g.ptr for g in ins], gamma, lam, adv.ptr, ret.ptr)
    hd.sync()
    rc = hd.lib.glgym_gae(hd.h, C.byref(a), hd.stream())
    hd.sync()
    assert rc == 0, (rc, hd.error())
    for g in ins:
        g.read()
    a_, r_ = adv.read(), ret.read()
    assert np.all(a_[T:].view(np.uint8) == 0xFF) and np.all(r_[T:].view(np.uint8) == 0xFF), "a guard row was written"
    return a_[:T], r_[:T]


@pytest.mark.parametrize("T,B", [(1, 1), (2, 257), (5, 65)])
def test_gae_against_the_host_build(hd, host, T, B):
    for pattern in ("first", "last", "all", "none", "random"):
        reward, done, value, last = make_gae_case(T, B, pattern, seed=4)
        for gamma, lam in ((0.99, 0.95), (0.9631, 0.95), (1.0, 1.0), (0.0, 0.5)):
            adv, ret = run_gae(hd, reward, done, value, last, gamma, lam)
            adv_h, ret_h = host_gae(host, reward, done, value, last, gamma, lam)
            assert same_u32(adv, adv_h) and same_u32(ret, ret_h), (pattern, gamma, lam)
            adv_n, ret_n = np_gae(reward, done, value, last, gamma, lam)
            assert same_u32(adv, adv_n) and same_u32(ret, ret_n), (pattern, gamma, lam)


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hd):
    """Every refusal returns GLGYM_EINVAL with its text and leaves every output as it was.  The argument blocks point at real device
    buffers throughout: a pointer that a table entry sets is replaced by a real one of the same role."""
    L = hd.L
    case = AcCase(23, 130)
    dc = DeviceCase(case)
    spare = E.Guarded(shape=(130 * 23 + 64,), dtype=np.float32)

    def good():
        return dc.args(step=3, seed=1)

    for path, value, word in AC_REFUSALS:
        a = good()
        if path == "obs_out":                                    # obs itself, and a span that overlaps its last float
            value = dc.inputs["obs"].ptr + (0 if (value - 0x10000) % 0x100000 == 0 else 130 * 23 * 4 - 4)
        elif isinstance(value, int) and value >= 0x10000 and path not in ("B",):
            value = spare.ptr                                    # "some non-null pointer"
        set_path(a, path, value)
        hd.sync()
        assert hd.lib.glgym_ac_rows(hd.h, C.byref(a), hd.stream()) == L.EINVAL, (path, value)
        assert word in hd.lib.glgym_last_error() and b"glgym_ac_rows" in hd.lib.glgym_last_error(), (path, hd.error())
    hd.sync()
    dc.read(())                                                  # nothing was written, no guard either
    assert spare.untouched()
    rc = hd.lib.glgym_ac_rows(hd.h, C.byref(good()), hd.stream())            # ... and the block they were derived from is good
    hd.sync()
    assert rc == 0, hd.error()
    dc.read(ALL_OUT)

    T, B = 5, 65
    reward, done, value, last = make_gae_case(T, B, "random")
    ins = [E.Guarded(v) for v in (reward, done, value, last)]
    adv, ret = E.Guarded(shape=(T, B), dtype=np.float32), E.Guarded(shape=(T, B), dtype=np.float32)
    by_offset = {0: ins[0].ptr, 1: ins[1].ptr, 2: ins[2].ptr, 3: ins[3].ptr, 4: adv.ptr}      # the table's k-th megabyte -> the k-th buffer
    for path, val, word in GAE_REFUSALS:
        a = gae_args(T, B, *[g.ptr for g in ins], 0.99, 0.95, adv.ptr, ret.ptr)
        if isinstance(val, int) and val >= 0x10000:
            k, rest = divmod(val - 0x10000, 0x100000)
            val = by_offset[k] + rest
        set_path(a, path, val)
        hd.sync()
        assert hd.lib.glgym_gae(hd.h, C.byref(a), hd.stream()) == L.EINVAL, (path, val)
        assert word in hd.lib.glgym_last_error() and b"glgym_gae" in hd.lib.glgym_last_error(), (path, hd.error())
    hd.sync()
    assert adv.untouched() and ret.untouched()
    for g, v in zip(ins, (reward, done, value, last)):
        assert np.array_equal(E.bits(g.read()), E.bits(v))


# ---- 4. graph capture -------------------------------------------------------------------------------------------------------------------
def test_both_calls_in_one_captured_graph(hd, host):
    import torch
    case = AcCase(23, 130)
    dc = DeviceCase(case)
    base_t = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    T, B = 3, 130
    reward, done, value, last = make_gae_case(T, B, "random")
    ins = [E.Guarded(v) for v in (reward, done, value, last)]
    adv, ret = E.Guarded(shape=(T, B), dtype=np.float32), E.Guarded(shape=(T, B), dtype=np.float32)
    a = dc.args(base_t.data_ptr(), step=2, seed=11, draw_index=3)
    g = gae_args(T, B, *[v.ptr for v in ins], 0.99, 0.95, adv.ptr, ret.ptr)

    def both():
        assert hd.lib.glgym_ac_rows(hd.h, C.byref(a), hd.stream()) == 0, hd.error()
        assert hd.lib.glgym_gae(hd.h, C.byref(g), hd.stream()) == 0, hd.error()

    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    base_t.fill_(5)                                              # the device word moves on between replays
    both()
    hd.sync()
    eager = dc.read(ALL_OUT)
    eager_adv = adv.read().copy()
    for o in list(dc.outs.values()) + [adv, ret]:
        o.t[E.GUARD:E.GUARD + o.n] = 0xFF
    graph.replay()
    hd.sync()
    replay = dc.read(ALL_OUT)
    same_named(replay, eager, ALL_OUT)
    assert within_one_f32_ulp(replay["eps"], np_eps64(B, 2, 8, 11))                   # D = 3 + 5: the replay read the advanced word
    assert same_u32(adv.read(), eager_adv) and same_u32(adv.read(), host_gae(host, reward, done, value, last, 0.99, 0.95)[0])


# ---- 5. collect() against its parts -----------------------------------------------------------------------------------------------------
def stack_of(dtype, wrapped, B):
    from gl_gym_amd.vec_monitor import VecMonitorGPU
    from gl_gym_amd.vec_normalize import VecNormalizeGPU
    env = make_env(B, dtype, auto_reset=True)
    return VecNormalizeGPU(VecMonitorGPU(env), norm_obs=True, norm_reward=True, clip_obs=10.0, gamma=0.9631) if wrapped else env


def elementwise_heads(device):
    """Heads without a reduction, so that two evaluations of the same observations agree bit for bit whatever GEMM torch would pick:
    six means and a value as elementwise functions of observation columns."""
    import torch

    class Pi(torch.nn.Module):
        def forward(self, obs):
            return torch.tanh(obs[:, :NU] * 1e-2) * 1.5

    class Vf(torch.nn.Module):
        def forward(self, obs):
            return torch.tanh(obs[:, NU:NU + 1] * 1e-2) - 0.25 * torch.tanh(obs[:, 2:3] * 1e-2)

    return Pi().to(device), Vf().to(device), torch.full((NU,), -0.5, device=device)


def parts_loop(env, heads, T, seed, gamma, lam):
    """The collection written out: the heads, raw glgym_ac_rows calls into buffers of its own, env.step_tensor, NumPy GAE."""
    import torch
    from gl_gym_amd import _lib as L
    pi, vf, log_std = heads
    B, D, dev = env.num_envs, env.obs_dim, env.device
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
    out = dict(observations=z(T, B, D), actions=z(T, B, NU), rewards=z(T, B), dones=z(T, B, dtype=torch.uint8), values=z(T, B),
               log_probs=z(T, B), last_values=z(B))
    act_env, std = z(B, NU), log_std.exp()
    lib = L.load()
    obs = env.reset_tensor(seed)
    for k in range(T + 1):
        last = k == T
        with torch.no_grad():
            mean, value = pi(obs).contiguous(), vf(obs).reshape(B).contiguous()
        a = L.make_plan_args(L.AcRowsArgs, B, D, k, 0, int(last), mean.data_ptr(), value.data_ptr(), log_std.data_ptr(), std.data_ptr(), seed, 0,
                             None, obs.data_ptr(), None if last else out["observations"][k].data_ptr(),
                             None if last else out["actions"][k].data_ptr(), None if last else act_env.data_ptr(), None,
                             None if last else out["log_probs"][k].data_ptr(),
                             out["last_values"].data_ptr() if last else out["values"][k].data_ptr())
        L.check(lib.glgym_ac_rows(env._h, C.byref(a), env._stream()), "glgym_ac_rows")
        if not last:
            obs, rew, done = env.step_tensor(act_env)[:3]
            out["rewards"][k].copy_(rew.float())
            out["dones"][k].copy_(done)
    torch.cuda.synchronize()
    n = {k: v.cpu().numpy() for k, v in out.items()}
    n["advantages"], n["returns"] = np_gae(n["rewards"], n["dones"], n["values"], n["last_values"], gamma, lam)
    return n


@pytest.mark.parametrize("wrapped", [False, True], ids=["bare", "stack"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_collect_is_the_loop_over_its_parts(dtype, wrapped):
    import torch
    from gl_gym_amd import RolloutCollector, TorchHeads
    T, B, seed, gamma, lam = 4, 130, 5, 0.9631, 0.95
    envs = [stack_of(dtype, wrapped, B) for _ in range(3)]
    heads = elementwise_heads(envs[0].device)
    cols = [RolloutCollector(e, T, TorchHeads(*heads), gamma=gamma, gae_lambda=lam, seed=99) for e in envs[:2]]
    outs = []
    for col in cols:
        col.reset(seed=seed)
        got = col.collect()
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy().copy() for k, v in got.items()})
        assert int(col.draw_base_t) == 1 and col.seed == seed
    want = parts_loop(envs[2], heads, T, seed, gamma, lam)
    for k, v in want.items():
        assert np.array_equal(E.bits(outs[0][k]), E.bits(v)), k                       # the loop over its parts
    for k, v in outs[0].items():
        assert np.array_equal(E.bits(outs[1][k]), E.bits(v)), k                       # an identically seeded pair
    first = outs[0]
    assert (first["episode_starts"][0] == 1).all() and np.array_equal(first["episode_starts"][1:], first["dones"][:-1])
    assert np.isfinite(first["advantages"]).all() and np.abs(first["actions"]).max() > 1 and first["values"].std() > 0
    # a second collect: the same tensors, other noise, the episodes go on
    col = cols[0]
    again = col.collect()
    torch.cuda.synchronize()
    assert all(again[k].data_ptr() == col.buffer[k].data_ptr() for k in again) and int(col.draw_base_t) == 2
    second = {k: v.cpu().numpy() for k, v in again.items()}
    assert np.array_equal(second["episode_starts"][0], first["dones"][-1]) and not np.array_equal(second["actions"], first["actions"])
    det = {k: v.cpu().numpy().copy() for k, v in col.collect(deterministic=True).items()}
    assert np.array_equal(det["log_probs"], np.broadcast_to(det["log_probs"][0, 0], det["log_probs"].shape))      # e = 0 everywhere
    for e in envs:
        e.close()


def test_collect_continues_episodes_across_calls_with_linear_layer_heads():
    """A one-day season is 96 steps: 25 collects of 4 steps cross its end.  The heads are small nn.Sequential nets here."""
    import torch
    from gl_gym_amd import RolloutCollector, TorchHeads
    T, B = 4, 130
    env = stack_of("float32", True, B)
    torch.manual_seed(0)
    D = env.obs_dim
    pi = torch.nn.Sequential(torch.nn.Linear(D, 96), torch.nn.Tanh(), torch.nn.Linear(96, NU)).to(env.device)
    vf = torch.nn.Sequential(torch.nn.Linear(D, 80), torch.nn.Tanh(), torch.nn.Linear(80, 1)).to(env.device)
    log_std = torch.nn.Parameter(torch.full((NU,), -0.3, device=env.device))
    col = RolloutCollector(env, T, TorchHeads(pi, vf, log_std), gamma=0.99, gae_lambda=0.9, seed=4)
    col.reset(seed=1)
    prev_done, seen = np.ones(B, dtype=np.uint8), 0
    for it in range(25):
        b = {k: v.cpu().numpy().copy() for k, v in col.collect().items()}
        assert np.array_equal(b["episode_starts"][0], prev_done) and np.array_equal(b["episode_starts"][1:], b["dones"][:-1]), it
        prev_done, seen = b["dones"][-1], seen + int(b["dones"].sum())
        if it == 0:
            with torch.no_grad():
                obs0 = torch.as_tensor(b["observations"][0], device=env.device)
                mean, value = pi(obs0).cpu().numpy(), vf(obs0).reshape(-1).cpu().numpy()
            eps = np_eps64(B, 0, 0, 1).astype(np.float32)
            # the external heads' outputs went through the stage.  Order-of-magnitude checks (a head that was not read gives differences of
            # order 1): torch evaluates the modules a second time here and need not pick the same GEMM, so 1e-5, not bit for bit
            assert np.abs(b["values"][0] - value).max() < 1e-5
            assert np.abs(b["actions"][0] - (mean + np.exp(np.float32(-0.3)) * eps)).max() < 1e-5
            adv, ret = np_gae(b["rewards"], b["dones"], b["values"], b["last_values"], 0.99, 0.9)
            assert same_u32(b["advantages"], adv) and same_u32(b["returns"], ret)
    assert seen >= B and int(col.draw_base_t) == 25                                   # every env finished its day
    env.close()
