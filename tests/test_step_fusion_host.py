"""CPU test of the fused-step bookkeeping (gl_gym_amd/step_fusion.py as TomatoVecEnv uses it): seeded random call sequences over a shell
environment -- a TomatoVecEnv without a GPU: CPU torch tensors, a stub library that records the entry points called -- replayed from
tests/golden/step_fusion_traces.json, which holds the generator's seed and what the bookkeeping of the commit before step_fusion.py existed
did with each call: the library entry points called, the mask of each reset / observation and whether term_obs was passed, the four
counters, the exception type.  Everything is compared EXACTLY.

The stub moves what the bookkeeping reads from memory, through raw pointers as a kernel would (no torch version counter changes): a
step writes `done` and advances `timestep`; glgym_reset and glgym_step_obs_reset zero `timestep` where their mask is set."""
import ctypes as C
import json
import random
from pathlib import Path

import pytest
import torch

from gl_gym_amd import _lib as L                                    # noqa: E402
from gl_gym_amd.tomato_env import TomatoVecEnv, _EpochLib           # noqa: E402

FIXTURE = Path(__file__).resolve().parent / "golden" / "step_fusion_traces.json"
B, LD, OBS_DIM = 4, 64, 5
OBS_DEP_TENSORS = ("x_T", "u_T", "timestep_t", "w_off_t", "start_day_t", "weather_t", "obs_t")      # what a full-mode observation depends on
DEP_TENSORS = ("x_T", "u_T", "timestep_t", "w_off_t", "start_day_t", "episode_t", "done_t", "obs_t", "term_obs_t", "weather_t")
COUNTERS = ("n_fused_steps", "n_obs_elided", "n_fused_resets", "n_reset_elided")


class StubLib:
    """Records [entry point without its glgym_ prefix, mask source, mask contents as a 0/1 string, term_obs passed] per call; every call
    returns GLGYM_OK."""

    def __init__(self, fused_out):
        self.fused_out, self.calls, self.env, self.next_done = fused_out, [], None, [0] * B

    def _mask(self, ptr):
        if not ptr:
            return "none", None
        env = self.env
        src = "done_t" if ptr == env.done_t.data_ptr() else "other" if ptr == env.other_mask.data_ptr() else "derived"
        return src, "".join(str(int(v != 0)) for v in (C.c_ubyte * B).from_address(ptr))

    def _timestep(self):
        return (C.c_int32 * B).from_address(self.env.timestep_t.data_ptr())

    def _step(self, reset):
        ts, done = self._timestep(), (C.c_ubyte * B).from_address(self.env.done_t.data_ptr())
        for b in range(B):
            done[b] = self.next_done[b]
            ts[b] = 0 if (reset and done[b]) else ts[b] + 1

    def __getattr__(self, name):
        def call(*args):
            rec = [name[len("glgym_"):]]
            if name in ("glgym_obs", "glgym_reset"):
                a = args[1]._obj
                src, mask = self._mask(a.mask)
                rec += [src, mask] + ([bool(a.term_obs)] if name == "glgym_obs" else [])
                if name == "glgym_reset":
                    ts = self._timestep()
                    for b in range(B):
                        if mask is None or mask[b] == "1":
                            ts[b] = 0
            elif name in ("glgym_step", "glgym_step_obs"):
                self._step(False)
            elif name == "glgym_step_obs_reset":
                self._step(True)
                args[-1]._obj.value = self.fused_out
            self.calls.append(rec)
            return 0
        return call


def make_shell(stub, auto_reset, rng):
    """A TomatoVecEnv with everything the step / observation / reset methods touch, and nothing else."""
    from gl_gym_amd.step_fusion import StepFusion
    env = object.__new__(TomatoVecEnv)
    env._fusion = StepFusion()
    env._lib = _EpochLib(stub, env._fusion)
    env._action_src, env.freeze_crop_noise, env._u_applied_valid = None, False, False
    return fill_shell(env, stub, auto_reset, rng)


def fill_shell(env, stub, auto_reset, rng):
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)  # noqa: E731
    stub.env = env
    env.torch, env.device, env.tdtype = torch, torch.device("cpu"), torch.float32
    env._h, env._stream, env._env_at_create = C.c_void_p(1), (lambda: C.c_void_p(0)), None
    env.B, env.ld, env.N, env.Np, env.obs_dim, env.dt, env.c = B, LD, 8, 1, OBS_DIM, 900.0, 86400
    env.auto_reset, env.rng, env.uncertainty_scale, env.seed_value, env._draw = auto_reset, rng, 0.0, 0, 0
    env.x_T, env.u_T, env.ctrl_T, env.info_T = z(L.NX, LD), z(L.NU, LD), z(L.NU, LD), z(L.NINFO, LD)
    env.reward_t, env.done_t, env.other_mask = z(LD), z(B, dtype=torch.uint8), torch.ones(B, dtype=torch.uint8)
    env.timestep_t, env.w_off_t, env.episode_t = (z(B, dtype=torch.int32) for _ in range(3))
    env.step_flags_t, env.start_day_t, env.action_t = z(B, dtype=torch.int32), z(B), z(B, L.NU)
    env.obs_t, env.term_obs_t, env.other_obs, env.other_term = (z(B, OBS_DIM) for _ in range(4))
    env.metrics_t = env.crop_T = env._u_applied_T = None
    env._keep_applied_u = False
    env._weather_data = torch.zeros(16, L.ND, dtype=torch.float64).numpy()
    env.weather_t, env.weather_rows = z(16, L.ND), 16
    env.start_rows, env.start_days, env.start_grid = [0], [0.0], (1, 1)
    env._start_rows_t, env._start_days_t = z(1, dtype=torch.int32), z(1)
    env.rng_state_t = z(5, LD, dtype=torch.int64) if rng == "numpy" else None
    return env


# ---- the scenario driver ----------------------------------------------------------------------------------------------------------
def generate(rng, max_calls=40):
    """One sequence: [config, ops].  Mostly bench.py's loop (bare step, full obs, reset(done_t), masked obs over the whole triple) with
    other calls and writes in between, so that every path behind a fused step is reached."""
    config = dict(auto_reset=rng.random() < 0.85, rng="numpy" if rng.random() < 0.1 else "philox", fused_out=int(rng.random() < 0.8))
    choice = lambda seq: seq[int(rng.random() * len(seq))]          # noqa: E731  (random() alone: the one stream Python guarantees for a seed)
    tri = lambda: choice([None, None, True, False])                 # noqa: E731
    bits = lambda p: "".join(str(int(rng.random() < p)) for _ in range(B))      # noqa: E731

    def other():
        k = int(rng.random() * 9)
        if k == 0:
            return ["step", int(rng.random() < 0.3), tri(), tri(), bits(0.3)]
        if k == 1:
            return ["step_tensor", choice("ac"), int(rng.random() < 0.8), int(rng.random() < 0.4), bits(0.3)]
        if k == 2:
            return ["obs", choice(["own", "own", "other"])]
        if k == 3:
            return ["reset", choice(["done", "done", "other", "none"])]
        if k == 4:
            return ["mobs", choice(["own", "own", "own", "other"]), choice(["done", "done", "done", "other"]),
                    choice(["own", "own", "own", "other", "none"])]
        if k in (5, 6):
            name = choice(DEP_TENSORS + ("done_t",) * 4 + ("timestep_t",) * 3)
            return ["write", name] + ([bits(0.4)] if name == "done_t" else [])
        if k == 7:
            return ["setter"] if rng.random() < 0.5 else ["weather"]
        return None                                                 # both of done_t and timestep_t written: two ops

    def more():
        op = other()
        return [op] if op is not None else [["write", "done_t", bits(0.4)], ["write", "timestep_t"]]

    ops = []
    while len(ops) < max_calls - 4:
        if rng.random() < 0.75:
            for op in (["step", 0, None, None, bits(0.3)], ["obs", "own"], ["reset", "done"], ["mobs", "own", "done", "own"]):
                while rng.random() < 0.15:
                    ops += more()
                ops.append(op)
        else:
            ops += more()
    return [config, ops[:max_calls]]


LOOP = [["step", 0, None, None, "0100"], ["obs", "own"], ["reset", "done"], ["mobs", "own", "done", "own"]]     # bench.py's loop


def scripted():
    """The sequences no random draw is trusted with.  For every dependency tensor: one in-place write between a step with fused
    observation and auto-reset and its first, second or third follow-up call, and one between a step with the fused observation alone
    (auto_reset off) and its observation -- each after one loop iteration that arms the fusing, and followed by another.  Last: a step
    with want_obs=True and with_reset=None right after a complete pattern (it must not take the auto-reset)."""
    on = dict(auto_reset=True, rng="philox", fused_out=1)
    off = dict(on, auto_reset=False)
    out = []
    for name in DEP_TENSORS:
        write = ["write", name] + (["0010"] if name == "done_t" else [])
        out += [[on, LOOP + LOOP[:k + 1] + [write] + LOOP[k + 1:] + LOOP] for k in range(3)]
        out.append([off, LOOP[:2] + [LOOP[0], write, LOOP[1]] + LOOP[:2]])
    out.append([on, LOOP * 2 + [["step", 0, True, None, "0100"]] + LOOP[1:] + LOOP])
    return out


def sequences(seed, n_random):
    rng = random.Random(seed)
    return scripted() + [generate(rng) for _ in range(n_random)]


def apply(env, stub, op):
    kind, pick = op[0], lambda name, **t: t[name]                   # noqa: E731
    ints = lambda bits: [int(c) for c in bits]                      # noqa: E731
    if kind == "step":
        stub.next_done = ints(op[4])
        env._action_src = env.action_t
        env._launch_step(bool(op[1]), want_obs=op[2], with_reset=op[3])
    elif kind == "step_tensor":
        stub.next_done, env._keep_applied_u = ints(op[4]), bool(op[3])
        try:
            t = torch.zeros(B, L.NU)
            env.step_tensor(**{"actions_t" if op[1] == "a" else "controls_t": t}, want_obs=bool(op[2]))
        finally:
            env._keep_applied_u = False
    elif kind == "obs":
        env._launch_obs(pick(op[1], own=env.obs_t, other=env.other_obs))
    elif kind == "reset":
        env._launch_reset(pick(op[1], done=env.done_t, other=env.other_mask, none=None))
    elif kind == "mobs":
        env._launch_obs(pick(op[1], own=env.obs_t, other=env.other_obs), pick(op[2], done=env.done_t, other=env.other_mask),
                        pick(op[3], own=env.term_obs_t, other=env.other_term, none=None))
    elif kind == "write":
        t = getattr(env, op[1])
        if op[1] == "done_t":
            t.bitwise_or_(torch.tensor(ints(op[2]), dtype=torch.uint8))
        else:
            t.add_(1 if op[1] == "timestep_t" else 0)
    elif kind == "setter":
        env._lib.glgym_set_verify(env._h, 0)
    elif kind == "weather":
        env.weather_data = env._weather_data.copy()


def run_sequence(shell, config, ops):
    """What each call did: [library calls, counters, exception type or None]."""
    stub = StubLib(config["fused_out"])
    env = shell(stub, config["auto_reset"], config["rng"])
    trace = []
    for op in ops:
        stub.calls, exc = [], None
        try:
            apply(env, stub, op)
        except RuntimeError as e:
            exc = type(e).__name__
        trace.append([stub.calls, [getattr(env, n) for n in COUNTERS], exc])
    return trace


def record(shell, seed, n_random):
    return dict(seed=seed, traces=[run_sequence(shell, config, ops) for config, ops in sequences(seed, n_random)])


# ---- the tests ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    """[(config, ops, recorded trace)]: the scripted sequences, then the random ones generated again from the fixture's seed."""
    data = json.loads(FIXTURE.read_text())
    seqs = sequences(data["seed"], len(data["traces"]) - len(scripted()))
    return [(config, ops, trace) for (config, ops), trace in zip(seqs, data["traces"])]


def test_bench_loop_counters():
    """Ten bare bench-style steps: 9 fused steps, 9 observations elided, 9 fused resets, 18 reset-side calls elided, and from the second step on one library call per iteration."""
    ops = [["step", 0, None, None, "0100"], ["obs", "own"], ["reset", "done"], ["mobs", "own", "done", "own"]] * 10
    trace = run_sequence(make_shell, dict(auto_reset=True, rng="philox", fused_out=1), ops)
    assert trace[-1][1] == [9, 9, 9, 18] and all(t[2] is None for t in trace)
    names = [c[0] for t in trace for c in t[0]]
    assert names == ["step", "obs", "reset", "obs"] + ["step_obs_reset"] * 9


def test_bookkeeping_reproduces_the_recorded_traces(fixture):
    assert 1 <= len(fixture) <= 400
    for i, (config, ops, trace) in enumerate(fixture):
        assert len(ops) == len(trace) <= 40
        got = json.loads(json.dumps(run_sequence(make_shell, config, ops)))
        for j, (g, w) in enumerate(zip(got, trace)):
            assert g == w, (i, j, config, ops[max(0, j - 6):j + 1])


def test_fixture_reaches_every_outcome(fixture):
    seen = set()
    for _, ops, trace in fixture:
        before = [0, 0, 0, 0]
        for op, (calls, n, exc) in zip(ops, trace):
            elided = n[3] > before[3]
            if n[1] > before[1]:
                seen.add("obs elided")
            if op[0] == "reset" and elided:
                seen.add("reset elided")
            if op[0] == "mobs" and elided:
                seen.add("masked obs elided")
            if op[:2] == ["reset", "done"] and not calls and not elided and exc is None:
                seen.add("reset skipped: applied by the step")
            if op[:2] == ["reset", "done"] and any(c[0] == "reset" and c[1] == "derived" for c in calls):
                seen.add("reset over added environments only")
            if op[0] == "mobs" and op[3] != "none" and calls and calls[-1][1] == "done_t" and calls[-1][3] is False:
                seen.add("terminal rows not saved twice")
            if exc is not None:
                seen.add(exc + " in " + op[0])
            before = n
    assert seen == {"obs elided", "reset elided", "masked obs elided", "reset skipped: applied by the step",
                    "reset over added environments only", "terminal rows not saved twice", "RuntimeError in reset", "RuntimeError in mobs"}


def test_fixture_has_a_write_to_every_dependency_un_elide_every_follow_up_call(fixture):
    """For every tensor a token depends on: one write between a fused step and the follow-up call that would have launched nothing
    otherwise occurs in the fixture, and that call was not elided there -- before the observation (with and without the fused
    auto-reset), before the reset, before the masked observation."""
    seen = set()
    for _, ops, trace in fixture:
        for i, op in enumerate(ops):
            if op[0] != "step" or not trace[i][0]:
                continue
            fused, follow = trace[i][0][-1][0], ops[i + 1:i + 5]
            writes = [k for k, o in enumerate(follow) if o[0] == "write"]
            if fused == "step_obs" and ops[i + 1:i + 3] == [ops[i + 1], LOOP[1]] and writes[:1] == [0] and trace[i + 2][0]:
                seen.add(("obs alone", follow[0][1]))
            if fused != "step_obs_reset" or len(writes) != 1 or writes[0] > 2 or [o for o in follow if o[0] != "write"] != LOOP[1:]:
                continue
            k, j = writes[0], i + 1 + writes[0] + 1               # the write comes before follow-up call k, which is ops[j]
            if k == 1 and trace[j][1][3] == trace[j - 1][1][3]:   # (a reset the step has applied launches nothing either way: the counter tells)
                seen.add(("reset", follow[k][1]))
            if k != 1 and trace[j][0]:
                seen.add((("obs", None, "mobs")[k], follow[k][1]))
    want = {(kind, t) for kind in ("obs alone", "obs") for t in OBS_DEP_TENSORS} | {(kind, t) for kind in ("reset", "mobs") for t in DEP_TENSORS}
    assert want - seen == set()
    assert not {(kind, t) for kind, t in seen if kind.startswith("obs") and t not in OBS_DEP_TENSORS}       # ... and no other write did


def test_want_obs_without_with_reset_takes_no_auto_reset(fixture):
    config, ops, trace = fixture[len(scripted()) - 1]
    i = next(i for i, op in enumerate(ops) if op[:4] == ["step", 0, True, None])
    assert ops[i - 4:i] == LOOP and trace[i - 4][0][-1][0] == "step_obs_reset" and trace[i][0][-1][0] == "step_obs"
