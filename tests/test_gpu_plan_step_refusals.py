"""What glgym_step refuses, the closed-loop rollouts refuse before their first prologue, in glgym_step's words.

glgym_plan_rollout_scenarios, glgym_plan_rollout_rule and glgym_plan_rollout_policy (include/glgym.h) launch a prologue -- the scenario
kernel, glgym_obs, the rule or policy rows -- in front of every env-step.  In every state in which glgym_step returns GLGYM_EINVAL
without launching, they must return GLGYM_EINVAL too, leave glgym_last_error() byte-equal to what glgym_step leaves when called with
the same step block on the same handle, and have written nothing: every buffer a prologue writes still holds the sentinel it was
filled with.  These are argument refusals that return an error code; nothing is launched in them.  One accepted case per rollout runs
to n_steps == 2, so that the refusals are not the only thing the arguments built here can produce.
2 greenhouses x 2 candidates x 2 scenarios (8 children, ld 64; 4 children without scenarios), horizon 2, fp32."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_plan_policy import spec_for
from test_gpu_plan_rule import TUNE

pytestmark = pytest.mark.gpu
B, K, S, H = 2, 2, 2, 2
SENTINEL = 0x5A
BDF, EXPLICIT = 1, 0                                               # GLGYM_INTEGRATOR_*


class Rig:
    """One fp32 handle over 14-column weather rows (so that GLGYM_ODE_PIPE can be set on it) and the planner objects whose buffers
    the calls below use: the scenario planner, and a rule search and a policy search with S = 2 and without scenarios."""

    def __init__(self):
        import torch
        from gl_gym_amd import _lib as L
        from gl_gym_amd.baseline import RuleBasedController
        from gl_gym_amd.tomato_env import TomatoVecEnv
        from gl_gym_amd.utils import synthetic_weather
        w = synthetic_weather(n_rows=2000)
        w = np.concatenate([w, np.zeros((len(w), 4))], axis=1)     # ODE_pipe's columns: measured pipe temperature, switch-off flag
        w[:, 10] = 45.0
        self.torch, self.L = torch, L
        self.env = env = TomatoVecEnv(B, weather=w, dtype="float32", season_length=1, start_rows=[0, 96, 480], seed=3, auto_reset=False)
        env.reset_tensor()
        for _ in range(2):
            env.step_tensor(controller=RuleBasedController(), want_obs=True)
        self.lib, self.h = env._lib, env._h
        scen = dict(n_scenarios=S, noise_scale=0.2)
        spec = spec_for(env, hidden=(8,))
        self.planner = env.planner(K, H, **scen)
        self.rule = {S: env.rule_search(K, H, tune=TUNE, **scen), 0: env.rule_search(K, H, tune=TUNE)}
        self.policy = {S: env.policy_search(K, H, spec, **scen), 0: env.policy_search(K, H, spec)}
        g = torch.Generator().manual_seed(7)
        rand = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).to(device=env.device, dtype=torch.float32).contiguous()  # noqa: E731
        self.actions = rand(H, B * K, L.NU)
        self.theta = {id(s): rand(s.Ht, s.J, L.NU) for s in list(self.rule.values()) + list(self.policy.values())}
        for s in self.policy.values():                             # padding: never read
            self.theta[id(s)][-1, :, (s.D - 1) % 6 + 1:] = 0.0
        # S = 0 children carry no crop block of their own: this one stands in where a state needs one
        self.spare_crop = torch.zeros(L.NCROP, 64, dtype=torch.float32, device=env.device)

    def close(self):
        self.env.close()

    # ---- the three calls: (entry point, its argument block, the step block it will use, the buffers its prologues write) ----
    def call(self, which, s, crop):
        L = self.L
        if which == "scenarios":
            p = self.planner
            r = p._rollout_args(self.actions.data_ptr(), None)
            a = L.make_plan_args(L.PlanRolloutScenariosArgs, *p._scenario_args(), p.stage_t.data_ptr(), r)
            written = [p.stage_t, p.crop_T, p.ret_t]
            use = dict(action=p.stage_t.data_ptr(), control=None)
            fn = self.lib.glgym_plan_rollout_scenarios
        elif which == "rule":
            rs = self.rule[s]
            p = rs.plan
            r = p._rollout_args(None, rs._plane_T.data_ptr())
            a = L.make_plan_args(L.PlanRolloutRuleArgs, 0, r, rs._space, self.theta[id(rs)].data_ptr(), p.start_day_t.data_ptr(), rs.J,
                                 *p._scenario_args())
            written = [rs._plane_T, p.ret_t] + ([p.crop_T] if s else [])
            use = dict(action=None, control=rs._plane_T.data_ptr())
            fn = self.lib.glgym_plan_rollout_rule
        else:
            ps = self.policy[s]
            p = ps.plan
            r = p._rollout_args(None, None)
            a = L.make_plan_args(L.PlanRolloutPolicyArgs, 0, r, ps._net, self.theta[id(ps)].data_ptr(), p.start_day_t.data_ptr(),
                                 ps.obs_t.data_ptr(), ps._plane_t.data_ptr(), self.env.Np, ps.row_mode, ps.J, *p._scenario_args())
            written = [ps._plane_t, ps.obs_t, p.ret_t] + ([p.crop_T] if s else [])
            use = dict(action=ps._plane_t.data_ptr(), control=None)
            fn = self.lib.glgym_plan_rollout_policy
        if crop and not s:
            a.rollout.step.crop_p = self.spare_crop.data_ptr()
            written.append(self.spare_crop)
        return fn, a, use, written, p

    def fill(self, tensors):
        for t in tensors:
            t.view(self.torch.uint8).fill_(SENTINEL)
        self.torch.cuda.synchronize(self.env.device)

    def untouched(self, tensors):
        self.torch.cuda.synchronize(self.env.device)
        return [bool((t.view(self.torch.uint8) == SENTINEL).all()) for t in tensors]


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


# state -> (handle setters to apply, edit of the step block, whether the state needs a crop block)
def _handle(variant=0, scheme="ls5", step_integrator=EXPLICIT, integrator=EXPLICIT):
    return dict(variant=variant, scheme=scheme, step_integrator=step_integrator, integrator=integrator)


STATES = {
    "struct_size": (_handle(), lambda st: setattr(st, "struct_size", 8), False),
    "null_x": (_handle(), lambda st: setattr(st, "x", None), False),
    "weather_rows_0": (_handle(), lambda st: setattr(st, "weather_rows", 0), False),
    "pipe_with_crop": (_handle(variant=1, scheme="rk4"), None, True),
    "pipe_not_rk4": (_handle(variant=1, scheme="ls5"), None, False),
    "pipe_bdf_step": (_handle(variant=1, scheme="rk4", step_integrator=BDF), None, False),
    "bdf_evalf_explicit_steps": (_handle(integrator=BDF), None, False),
}
CALLS = [("scenarios", S), ("rule", S), ("rule", 0), ("policy", S), ("policy", 0)]


def set_handle(rig, variant, scheme, step_integrator, integrator):
    L, lib, h = rig.L, rig.lib, rig.h
    assert lib.glgym_set_model_variant(h, variant) == L.OK
    assert lib.glgym_set_scheme(h, L.SCHEMES[scheme]) == L.OK
    assert lib.glgym_set_step_integrator(h, step_integrator) == L.OK
    assert lib.glgym_set_integrator(h, integrator) == L.OK


@pytest.mark.parametrize("which,s", CALLS, ids=[f"{w}_S{s}" for w, s in CALLS])
@pytest.mark.parametrize("state", list(STATES))
def test_rollout_refuses_in_glgym_steps_words_and_writes_nothing(rig, state, which, s):
    L, lib, h = rig.L, rig.lib, rig.h
    handle, edit, crop = STATES[state]
    fn, a, use, written, p = rig.call(which, s, crop)
    if edit:
        edit(a.rollout.step)
    stream = rig.env._stream()
    p.fork()
    rig.fill(written)
    set_handle(rig, **handle)
    try:
        direct = L.StepArgs.from_buffer_copy(a.rollout.step)     # the block as the rollout hands it to glgym_step
        direct.metrics, direct.action, direct.control = None, use["action"], use["control"]
        rc_step = lib.glgym_step(h, C.byref(direct), stream)
        words = lib.glgym_last_error()
        rc = fn(h, C.byref(a), stream)
        got = lib.glgym_last_error()
    finally:
        set_handle(rig, **_handle())
    print(f"{state} {which} S={s}: glgym_step {rc_step} {words!r}; rollout {rc} {got!r}")
    assert rc_step == L.EINVAL and words.startswith(b"glgym_step")
    assert rc == L.EINVAL
    assert got == words
    assert all(rig.untouched(written)), rig.untouched(written)


@pytest.mark.parametrize("which,s,handle", [("rule", 0, _handle(variant=1, scheme="rk4")), ("scenarios", S, _handle()),
                                            ("policy", S, _handle())], ids=["rule_S0_ode_pipe_rk4", "scenarios_default", "policy_default"])
def test_an_accepted_rollout_runs_its_two_steps(rig, which, s, handle):
    L = rig.L
    fn, a, _, written, p = rig.call(which, s, False)
    p.fork()
    rig.fill([t for t in written if t is not p.ret_t])
    if handle["scheme"] != "ls5":
        rig.env.set_scheme(handle["scheme"])                      # with the scheme's own sub-step count and window
    set_handle(rig, **handle)
    try:
        rc = fn(rig.h, C.byref(a), rig.env._stream())
        err = rig.lib.glgym_last_error()
        rig.torch.cuda.synchronize(rig.env.device)
    finally:
        rig.env.set_scheme("ls5")                                  # the construction's preset again
        set_handle(rig, **_handle())
    assert rc == L.OK, err
    assert (p.n_steps_t == H).all() and p.alive_t.all() and not p.failed_t.any()
    assert not any(rig.untouched([t for t in written if t is not p.ret_t]))       # every prologue ran
