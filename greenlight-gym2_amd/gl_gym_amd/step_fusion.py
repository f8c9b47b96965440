"""Host-side bookkeeping of the fused env-step (glgym_step_obs, glgym_step_obs_reset): what the last step's launch has already done, and
which of the calls that follow it therefore launch nothing.  Pure Python over duck-typed tensors (data_ptr(), _version): it imports
neither the library nor torch, and runs without a GPU (tests/test_step_fusion_host.py)."""
from typing import Optional

# every tensor a full-mode observation reads or lands in / a fused auto-reset reads or writes (attributes of the environment)
OBS_DEPS = ("x_T", "u_T", "timestep_t", "w_off_t", "start_day_t", "weather_t", "obs_t")
RESET_DEPS = ("x_T", "u_T", "timestep_t", "w_off_t", "start_day_t", "episode_t", "done_t", "obs_t", "term_obs_t", "weather_t")


def _snapshot(env, names):
    """Address and torch version counter of each tensor: an in-place write to one of them, or to a view of it, changes a counter."""
    return tuple((t.data_ptr(), t._version) for t in (getattr(env, n) for n in names))


class _StepRecord:
    """What one _launch_step left behind (StepFusion)."""
    __slots__ = ("obs_token", "reset_token", "pattern", "obs_followed", "applied")

    def __init__(self):
        self.obs_token = None       # set: the launch wrote the full-mode rows into obs_t; (id(obs_t), epoch, snapshot), single-use
        self.reset_token = None     # set: the launch also did the auto-reset and the terminal rows; (epoch, snapshot)
        self.pattern = 0            # follow-up calls so far: full obs (1), reset(done_t) (2), masked obs (3), in this order; -1: broken
        self.obs_followed = False   # a full-mode observation into obs_t followed
        self.applied = None         # a fused auto-reset: dict(done, timestep: (address, version); reset_seen, obs_seen, added)


class StepFusion:
    """One per TomatoVecEnv.  Holds the epoch, the four public counters and one record of the last _launch_step (None before the first:
    then every call launches as ever).

    The epoch advances with every call into the library through the environment (_EpochLib: kernel launches, setters, the planner,
    raw-pointer calls through env._lib) and with every assignment that replaces a buffer (the weather_data setter).  A token is the epoch
    and a snapshot taken right after the step's library call; it is honoured only while both are unchanged, so any library call and any
    in-place torch write to a dependency (OBS_DEPS / RESET_DEPS) in between makes the follow-up call compute from memory, as it always did.

    begin_step: a step asks for the observation epilogue when told to (want_obs), or, on a bare call (None, bench.py's loop), when the
    previous step was followed by a full-mode observation into obs_t -- loops that never ask for observations never pay for them, and
    a fused observation that went unconsumed ends the fusing.  It asks for the auto-reset epilogue when told to (with_reset; step_tensor,
    capture_step_graph), or, on a bare call, when the previous step was followed by exactly full obs -> reset(done_t) -> masked
    obs(obs_t, done_t, term_obs_t); always only together with the observation, with auto_reset and never with rng="numpy" (start draws
    from device streams between step and reset).  own_calls(): step_tensor and capture_step_graph made the follow-up calls themselves;
    those arm no bare step.

    full_obs: a full-mode observation into the very obs_t a fused step wrote, under an unchanged token, launches nothing (counted in
    n_obs_elided).  reset / masked_obs after a step with a fused auto-reset: under an unchanged token, reset(done_t) and then the masked
    observation over the whole triple launch nothing (each counted in n_reset_elided).  CONTRACT of such a step: x_T, u_T, timestep_t,
    w_off_t, start_day_t and episode_t hold the POST-RESET state of the finished environments and obs_t the first observation of their
    new episodes already when _launch_step returns; done_t, reward_t, info_T, step_flags_t and the metrics are the step's.  So where the
    token no longer holds, that step's reset is still applied and reset_kernel, which counts episodes and draws a new start each time it
    runs, must not run over it again: the first reset(done_t) after such a step launches nothing while done_t is unwritten; after an
    in-place write to done_t it runs over done_t AND timestep_t != 0 -- a step leaves timestep_t >= 1 in every environment it did not
    reset, so this keeps exactly the environments the caller added -- and raises if timestep_t was written as well (nothing tells the
    two apart).  Likewise the first masked observation over done_t computes the rows again without saving them to term_obs_t (the
    terminal rows are there already; the added environments get both, first) and raises if it is not over obs_t and term_obs_t."""

    def __init__(self):
        self.epoch = 0
        self.n_fused_steps = 0      # steps launched through glgym_step_obs / glgym_step_obs_reset
        self.n_obs_elided = 0       # full-mode observations that found their rows already written and launched nothing
        self.n_fused_resets = 0     # steps whose auto-reset and terminal observations ran inside the step's own launch
        self.n_reset_elided = 0     # reset(done_t) / masked observation calls that found their work done and launched nothing
        self._rec: Optional[_StepRecord] = None

    def advance(self):
        self.epoch += 1

    def own_calls(self):
        if self._rec is not None:
            self._rec.pattern = -1

    def begin_step(self, want_obs, with_reset, can_reset):
        """(fuse, with_reset) for the step about to be launched, and a fresh record."""
        rec = self._rec
        fuse = (rec is not None and rec.obs_followed) if want_obs is None else bool(want_obs)
        if with_reset is None:
            with_reset = want_obs is None and rec is not None and rec.pattern == 3
        self._rec = _StepRecord()
        return fuse, bool(with_reset) and fuse and can_reset

    def step_launched(self, env, with_reset, fused_reset=0):
        """After the library call of a step with the observation epilogue (with_reset: glgym_step_obs_reset, which reported fused_reset)."""
        rec = self._rec
        self.n_fused_steps += 1
        rec.obs_token = (id(env.obs_t), self.epoch, _snapshot(env, OBS_DEPS))
        if with_reset:
            self.n_fused_resets += fused_reset
            rec.reset_token = (self.epoch, _snapshot(env, RESET_DEPS))
            rec.applied = dict(done=_snapshot(env, ("done_t",)), timestep=_snapshot(env, ("timestep_t",)), reset_seen=False,
                               obs_seen=False, added=None)

    def _reset_token_holds(self, env, token):
        """True, and counted, if `token` is that of a fused auto-reset nothing has come after."""
        if token is None or token != (self.epoch, _snapshot(env, RESET_DEPS)):
            return False
        self.n_reset_elided += 1
        return True

    def full_obs(self, env, out_t):
        """True: the rows are in out_t already, launch nothing."""
        rec = self._rec
        if rec is None:
            return False
        token, rec.obs_token = rec.obs_token, None
        own = out_t is env.obs_t
        rec.pattern = 1 if (own and rec.pattern == 0) else -1
        if own:
            rec.obs_followed = True
            if token is not None and token == (id(out_t), self.epoch, _snapshot(env, OBS_DEPS)):
                self.n_obs_elided += 1
                return True
        rec.reset_token = None                                     # a launched observation: the pattern of a fused auto-reset is broken
        return False

    def reset(self, env, mask_t):
        """(launch, mask): whether reset_kernel runs, and over which mask."""
        rec = self._rec
        if rec is None:
            return True, mask_t
        token, rec.reset_token = rec.reset_token, None
        own = mask_t is env.done_t
        rec.pattern = 2 if (own and rec.pattern == 1) else -1
        if own and self._reset_token_holds(env, token):
            rec.reset_token = token                                # the masked observation that follows is part of the same fused step
            return False, None
        st = rec.applied
        if own and st is not None and not st["reset_seen"]:
            st["reset_seen"] = True
            if st["done"] == _snapshot(env, ("done_t",)):
                return False, None                                 # this step's reset, already applied by the step's own launch
            if st["timestep"] != _snapshot(env, ("timestep_t",)):
                raise RuntimeError("done_t and timestep_t were both written between a step with a fused auto-reset and its "
                                   "_launch_reset(done_t): the environments that step has already reset cannot be told from the ones "
                                   "added to the mask; reset those through a mask tensor of their own")
            mask_t = st["added"] = env.done_t * (env.timestep_t != 0).to(env.done_t.dtype)
        return True, mask_t

    def masked_obs(self, env, out_t, mask_t, term_t):
        """The (mask, term) pairs to launch glgym_obs with, in order; empty: the rows are where they belong already."""
        rec = self._rec
        if rec is None:
            return [(mask_t, term_t)]
        whole = out_t is env.obs_t and mask_t is env.done_t and term_t is env.term_obs_t
        token, rec.reset_token = rec.reset_token, None
        follows = whole and rec.pattern == 2
        rec.pattern = 3 if follows else -1
        if follows and self._reset_token_holds(env, token):
            return []
        st = rec.applied
        if mask_t is not env.done_t or term_t is None or st is None or st["obs_seen"]:
            return [(mask_t, term_t)]
        if not whole:
            raise RuntimeError("the terminal observations of a step with a fused auto-reset are in term_obs_t; a masked "
                               "_launch_obs over done_t after it takes obs_t and term_obs_t")
        st["obs_seen"] = True
        return ([(st["added"], term_t)] if st["added"] is not None else []) + [(mask_t, None)]
