"""glgym_step_obs: the one-lane fp32 step kernel writing the observation rows of its own wavefront (csrc/glgym.hip step_kernel, OBS builds), and
the Python routing that lets a full-mode _launch_obs find them there (gl_gym_amd/tomato_env.py).

Everything is compared bit for bit (torch.equal): the fused rows against a direct glgym_obs call on the same state, a fused environment
against a twin that is forced to launch the two kernels, a replayed graph against eager unfused steps, and the fallback paths (four
lanes per environment, fp64) against the two separate calls.  Batches: 1 (one live lane), 16 (one strip), 17 (a strip and one row), 64
(a full wavefront), 65 (a second wavefront with one live row), 100 (a ragged last wavefront, strips of 16 / 16 / 4).  season_length 1:
an episode is 97 steps, so 200 steps see two episode ends of every environment."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

BATCHES = (1, 16, 17, 64, 65, 100)
LAYOUTS = {
    "default": None,                                                      # 263 columns
    "permuted": ["IndoorClimateObservations", "WeatherForecastObservations", "TimeObservations", "ControlObservations",
                 "BasicCropObservations", "WeatherObservations"],
    "no_forecast": ["IndoorClimateObservations", "TimeObservations", "WeatherObservations", "BasicCropObservations",
                    "ControlObservations"],
}
N_STEPS = 200
_W = {}


def weather():
    if "w" not in _W:
        from gl_gym_amd.utils import synthetic_weather
        _W["w"] = synthetic_weather(n_rows=1000)
    return _W["w"]


def make_env(B, scheme="ls5", occ=1, unc=0.0, layout="default", dtype="float32", kernel_layout="one", **kw):
    from gl_gym_amd.tomato_env import TomatoVecEnv
    env = TomatoVecEnv(B, weather=weather(), dtype=dtype, scheme=scheme, season_length=1, pred_horizon=0.5, seed=11,
                       start_rows=[0, 96, 480], uncertainty_scale=unc, observation_modules=LAYOUTS[layout], **kw)
    if dtype == "float32":
        env.set_layout(kernel_layout)
        env.set_occupancy(occ)
    env.reset_tensor()
    return env


def actions(B, n, device, seed=5):
    import torch
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, B, 6, generator=g) * 2 - 1).to(device=device, dtype=torch.float32).contiguous()


def direct_obs(env, out_t):
    """glgym_obs in full mode straight through the library (not through the environment: its bookkeeping does not see this call)."""
    from gl_gym_amd import _lib as L
    L.check(L.load().glgym_obs(env._h, C.byref(env._obs_args(out_t)), env._stream()), "glgym_obs")


def begin_step(env, a, want_obs):
    env.action_t.copy_(a)
    env._action_src = env.action_t
    env._launch_step(raw_control=False, want_obs=want_obs)


def finish_step(env):
    env._launch_reset(env.done_t)
    env._launch_obs(env.obs_t, env.done_t, env.term_obs_t)


def unfused_step(env, a):
    begin_step(env, a, want_obs=False)
    env._launch_obs(env.obs_t)
    finish_step(env)


def assert_twins_equal(env, twin, where):
    import torch
    B = env.B
    for name in ("x_T", "u_T", "reward_t", "done_t", "info_T", "obs_t", "step_flags_t", "timestep_t", "w_off_t"):
        assert torch.equal(getattr(env, name), getattr(twin, name)), (name, where)
    done = env.done_t.bool()
    assert torch.equal(env.term_obs_t[done], twin.term_obs_t[done]), ("term_obs_t", where)
    assert env.x.shape[0] == B


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("unc", [0.0, 0.2])
@pytest.mark.parametrize("occ", [1, 2])
@pytest.mark.parametrize("scheme", ["ls5", "rk4"])
@pytest.mark.parametrize("B", BATCHES)
def test_fused_rows_equal_obs_kernel_and_unfused_twin(B, scheme, occ, unc, layout):
    """After every fused step the rows in obs_t equal what glgym_obs writes for the same state; over two episode ends the fused
    environment and a twin that launches step and observation kernels separately agree in everything a step produces."""
    import torch
    env, twin = (make_env(B, scheme, occ, unc, layout) for _ in range(2))
    acts = actions(B, N_STEPS, env.device)
    scratch = torch.empty_like(env.obs_t)
    ends = torch.zeros(B, dtype=torch.int64, device=env.device)
    for i in range(N_STEPS):
        begin_step(env, acts[i], want_obs=True)
        scratch.fill_(-3.0)
        direct_obs(env, scratch)
        assert torch.equal(env.obs_t, scratch), i
        elided = env.n_obs_elided
        env._launch_obs(env.obs_t)
        assert env.n_obs_elided == elided + 1
        ends += env.done_t
        finish_step(env)
        unfused_step(twin, acts[i])
        assert_twins_equal(env, twin, i)
    assert int(ends.min()) >= 2                     # two episode ends in every environment
    assert env.n_fused_steps == N_STEPS and twin.n_fused_steps == 0 and twin.n_obs_elided == 0
    env.close(); twin.close()


def test_skip_fires_only_where_it_may():
    """One elision per step in the plain pattern; none, and a correct obs_t, when a torch-side write to the state, the observation block
    or the clocks, a reset, or another output tensor comes between the fused step and the observation call."""
    import torch
    B = 100
    env = make_env(B)
    acts = actions(B, 16, env.device, seed=9)
    other, want = torch.empty_like(env.obs_t), torch.empty_like(env.obs_t)

    def expect_launch(between, out=None):
        i = expect_launch.i = expect_launch.i + 1
        begin_step(env, acts[i], want_obs=True)
        between()
        direct_obs(env, want)                       # the observation of what is in memory now
        elided, out_t = env.n_obs_elided, env.obs_t if out is None else out
        env._launch_obs(out_t)
        assert env.n_obs_elided == elided
        assert torch.equal(out_t, want)
        finish_step(env)
    expect_launch.i = -1

    for _ in range(3):                              # the plain pattern
        expect_launch.i += 1
        begin_step(env, acts[expect_launch.i], want_obs=True)
        elided = env.n_obs_elided
        env._launch_obs(env.obs_t)
        assert env.n_obs_elided == elided + 1
        finish_step(env)
    expect_launch(lambda: env.x.mul_(1.0))
    expect_launch(lambda: env.obs_t.fill_(-7.0))
    expect_launch(lambda: env.timestep_t.add_(0))
    expect_launch(lambda: env._launch_reset(env.done_t))
    expect_launch(lambda: None, out=other)
    # a write that does change the state: the observation follows it
    expect_launch(lambda: env.x.mul_(1.01))
    # the token is single-use: a second full-mode call launches
    begin_step(env, acts[12], want_obs=True)
    env._launch_obs(env.obs_t)
    elided = env.n_obs_elided
    env.obs_t.fill_(-7.0)
    direct_obs(env, want)
    env._launch_obs(env.obs_t)
    assert env.n_obs_elided == elided and torch.equal(env.obs_t, want)
    env.close()


def test_adaptive_arming():
    """A bare _launch_step fuses only after a step that was followed by a full-mode observation call; loops without one never do."""
    B = 65
    env = make_env(B)
    acts = actions(B, 8, env.device, seed=2)
    for i in range(4):                              # step + reset only
        begin_step(env, acts[i], want_obs=None)
        env._launch_reset(env.done_t)
    assert env.n_fused_steps == 0 and env.n_obs_elided == 0
    for i in range(4):                              # bench.py's loop: the first step finds out, the others fuse
        begin_step(env, acts[i], want_obs=None)
        env._launch_obs(env.obs_t)
        finish_step(env)
    assert env.n_fused_steps == 3 and env.n_obs_elided == 3
    begin_step(env, acts[4], want_obs=None)         # fused, and nobody asks for the rows ...
    env._launch_reset(env.done_t)
    begin_step(env, acts[5], want_obs=None)         # ... so this one is not
    env._launch_reset(env.done_t)
    assert env.n_fused_steps == 4 and env.n_obs_elided == 3
    env.close()


def test_graph_replay_equals_eager_unfused_steps():
    import torch
    B = 100
    env, twin = make_env(B), make_env(B)
    acts = actions(B, N_STEPS, env.device, seed=4)
    replay = env.capture_step_graph(want_obs=True)
    for i in range(N_STEPS):
        replay(acts[i])
        unfused_step(twin, acts[i])
        if i % 8 == 0 or i > N_STEPS - 8:
            assert_twins_equal(env, twin, i)
    assert torch.equal(env.term_obs_t, twin.term_obs_t)
    env.close(); twin.close()


@pytest.mark.parametrize("dtype,kernel_layout", [("float32", "quad"), ("float64", "one")])
def test_fallback_equals_two_calls(dtype, kernel_layout):
    """Handles without a fused kernel (four lanes per environment, fp64): glgym_step_obs gives the bits of the two separate calls."""
    import torch
    B = 17
    env, twin = (make_env(B, dtype=dtype, kernel_layout=kernel_layout) for _ in range(2))
    acts = actions(B, 100, env.device, seed=6)
    for i in range(100):
        begin_step(env, acts[i], want_obs=True)
        env._launch_obs(env.obs_t)
        finish_step(env)
        unfused_step(twin, acts[i])
    assert env.n_fused_steps == 100 and env.n_obs_elided == 100
    assert_twins_equal(env, twin, "end")
    assert torch.equal(env.term_obs_t, twin.term_obs_t)
    env.close(); twin.close()


def test_step_obs_refuses_a_mask():
    from gl_gym_amd import _lib as L
    env = make_env(16)
    before = env.x_T.clone()
    a = L.make_step_args(env.B, env.ld, env.x_T.data_ptr(), env.u_T.data_ptr(), env.action_t.data_ptr(), None, env.weather_t.data_ptr(),
                         env.weather_rows, env.w_off_t.data_ptr(), env.timestep_t.data_ptr(), None, env.N, env.reward_t.data_ptr(),
                         env.info_T.data_ptr(), env.done_t.data_ptr(), None, env.step_flags_t.data_ptr())
    o = env._obs_args(env.obs_t, env.done_t, env.term_obs_t)
    assert L.load().glgym_step_obs(env._h, C.byref(a), C.byref(o), env._stream()) == L.EINVAL
    assert (env.x_T == before).all()                # nothing ran
    env.close()
