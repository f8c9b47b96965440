"""Constrained candidate ranking on the GPU: glgym_plan_constrain through the C ABI on guarded buffers, and behind the rollouts of
Planner, RuleSearch and PolicySearch (gl_gym_amd.planner.Constraints).

Bounds.  EXACT everywhere.  The stage is compared bit for bit (uint64 views) with the NumPy restatement of tests/plan_constr_inputs.py
-- the one tests/test_plan_constr_host.py holds the host instantiation of csrc/gl_constr.hpp to -- on the same inputs and shapes; end
to end the restatement is applied to the tensors the rollout itself returned.  A planner with constraints must return the five raw
tensors of the same planner without them bit for bit, and a cem() under budgets that are all +inf its best_k, mean and spread.
Child batches stay <= 48 rows and horizons <= 4 steps."""
import ctypes as C

import numpy as np
import pytest

import plan_constr_inputs as I
from envlayer_inputs import Guarded, Handle, bits
from test_gpu_plan import make_env, rand_actions, same_bits

pytestmark = pytest.mark.gpu
OUT_KEYS = ("score", "failed_out", "feasible", "excess", "n_viol", "n_feasible")


@pytest.fixture(scope="module")
def hd():
    h = Handle(False)
    yield h
    h.close()


def stage_buffers(case, alias_failed=False):
    J, P = case["P"] * case["K"], case["P"]
    ins = {k: Guarded(case[k]) for k in ("ret", "failed", "viol", "n_steps")}
    outs = dict(score=Guarded(shape=(J,), dtype=np.float64), failed_out=ins["failed"] if alias_failed else Guarded(shape=(J,), dtype=np.uint8),
                feasible=Guarded(shape=(J,), dtype=np.uint8), excess=Guarded(shape=(J,), dtype=np.float64),
                n_viol=Guarded(shape=(J,), dtype=np.int32), n_feasible=Guarded(shape=(P,), dtype=np.int32))
    return ins, outs


def stage_args(L, case, ins, outs, optional=True, **over):
    c = {**case, **over}
    opt = [outs[k].ptr if optional else None for k in ("feasible", "excess", "n_viol", "n_feasible")]
    return L.make_plan_args(L.PlanConstrainArgs, c["P"], c["O"], c["K"], c["S"], c["ld"], c["per_step"], c["n_allow"], c["mode"],
                            (C.c_double * 3)(*c["budget"]), (C.c_double * 3)(*c["weight"]), c["rho"], ins["ret"].ptr, ins["failed"].ptr,
                            ins["viol"].ptr, ins["n_steps"].ptr, outs["score"].ptr, outs["failed_out"].ptr, *opt)


def launch(hd, a, expect=0):
    hd.sync()
    rc = hd.lib.glgym_plan_constrain(hd.h, C.byref(a), hd.stream())
    hd.sync()
    assert rc == expect, (rc, hd.error())
    return hd.error()


def assert_same(got, want, keys=OUT_KEYS):
    for k in keys:
        assert np.array_equal(bits(got[k]), bits(want[k])), (k, got[k], want[k])


# ---- 1. the stage against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(I.CASES))
def test_stage_equals_the_restatement(hd, name):
    case = I.CASES[name]
    want = I.expect(case)
    ins, outs = stage_buffers(case)
    launch(hd, stage_args(hd.L, case, ins, outs))
    assert_same({k: outs[k].read() for k in OUT_KEYS}, want)
    for k in ("ret", "failed", "viol", "n_steps"):
        assert np.array_equal(bits(ins[k].read()), bits(case[k])), f"input {k} was written"
    ins, outs = stage_buffers(case, alias_failed=True)                      # failed_out = failed_cand, no optional output
    launch(hd, stage_args(hd.L, case, ins, outs, optional=False))
    assert_same({k: outs[k].read() for k in ("score", "failed_out")}, want, keys=("score", "failed_out"))
    assert all(outs[k].untouched() for k in ("feasible", "excess", "n_viol", "n_feasible"))


def test_stage_refusals_leave_the_outputs_untouched(hd):
    L, case = hd.L, I.CASES["allow1"]
    R = case["O"] * case["S"]
    nan = float("nan")
    bad = [dict(n_allow=R + 1), dict(n_allow=-1), dict(budget=[nan, 1.0, 1.0]), dict(budget=[1.0, -0.5, 1.0]), dict(weight=[1.0, -1.0, 1.0]),
           dict(weight=[1.0, I.INF, 1.0]), dict(rho=-1.0), dict(rho=nan), dict(mode=2), dict(per_step=2), dict(K=0), dict(ld=case["ld"] - 4)]
    ins, outs = stage_buffers(case)
    for over in bad:
        assert "glgym_plan_constrain" in launch(hd, stage_args(L, case, ins, outs, **over), expect=L.EINVAL), over
    a = stage_args(L, case, ins, outs)
    a.struct_size -= 8
    assert "struct_size" in launch(hd, a, expect=L.EINVAL)
    a = stage_args(L, case, ins, outs)
    a.score = ins["ret"].ptr                                                # aliasing score with ret_cand
    assert "overlaps" in launch(hd, a, expect=L.EINVAL)
    a.score = ins["ret"].ptr + 8 * (case["P"] * case["K"] - 1)              # ... by one entry
    assert "overlaps" in launch(hd, a, expect=L.EINVAL)
    for name in ("viol", "score", "n_steps"):
        a = stage_args(L, case, ins, outs)
        setattr(a, name, None)
        assert "null" in launch(hd, a, expect=L.EINVAL), name
    assert all(outs[k].untouched() for k in OUT_KEYS)
    for k in ("ret", "failed", "viol", "n_steps"):
        assert np.array_equal(bits(ins[k].read()), bits(case[k]))


# ---- helpers of the rollout tests ---------------------------------------------------------------------------------------------------
def started(B, dtype, n=2, **kw):
    from gl_gym_amd.baseline import RuleBasedController
    env = make_env(B, dtype, **kw)
    env.reset_tensor()
    for _ in range(n):
        env.step_tensor(controller=RuleBasedController(), want_obs=True)
    return env


def host(t):
    return np.ascontiguousarray(t.cpu().numpy())


def restate(plan, constraints, P, O, K, ret, failed):
    """The restatement on what a rollout left in the plan's per-run accumulators, for candidates' returns `ret` / `failed` [P*K]."""
    S = plan.S or 1
    mode = I.FEASIBLE_FIRST if constraints.mode == "feasible_first" else I.PENALTY
    return I.np_constrain(P, O, K, S, 1 if constraints.per == "step" else 0, constraints.n_allow, mode, list(constraints.budgets),
                          list(constraints.weights), constraints.rho, host(ret).reshape(-1), host(failed).reshape(-1), host(plan.viol_T),
                          host(plan.n_steps_t))


def median_budget(viol, steps):
    """(which, budget): the humidity or temperature budget at the median per-step violation of a rollout [3, B, K], the first of the
    two under which some greenhouse has a candidate within and a candidate over it."""
    for i in (2, 1):
        per = viol[i] / np.maximum(steps, 1)
        med = float(np.median(per))
        inside = per <= med
        if (inside.any(axis=1) & ~inside.all(axis=1)).any():
            return i, med
    return None, None


def with_budget(i, budget, **kw):
    from gl_gym_amd.planner import Constraints
    return Constraints(**{("co2", "temp", "rh")[i]: budget}, **kw)


def assert_views(obj, want, rows, K):
    for t, k in ((obj.feasible, "feasible"), (obj.excess, "excess"), (obj.n_violating, "n_viol")):
        assert tuple(t.shape) == (rows, K) and np.array_equal(bits(host(t).reshape(-1)), bits(want[k])), k
    assert np.array_equal(host(obj.n_feasible), want["n_feasible"])


# ---- 2. end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_planner_end_to_end(dtype):
    B, K, H = 2, 16, 4
    env = started(B, dtype)
    actions = rand_actions((H, B * K, 6), 11, env.device)
    plain = env.planner(K, H, gamma=0.97)
    raw = [t.clone() for t in plain.rollout(actions)]
    assert plain._score_t is plain.ret_t and "best_feasible" not in plain.select()
    which, budget = median_budget(host(raw[3]), host(raw[2]))
    print(f"{dtype}: per-step violations co2/temp/rh max {[float(host(raw[3])[i].max()) for i in range(3)]}, budget {which} = {budget}")
    assert which is not None, "no greenhouse has both a candidate within and one over the median humidity / temperature violation"
    con = with_budget(which, budget)
    plan = env.planner(K, H, gamma=0.97, constraints=con)
    out = plan.rollout(actions)
    for a, b in zip(out, raw):                                              # the five returned tensors are the raw ones
        assert same_bits(a, b)
    want = restate(plan, con, B, 1, K, raw[0], raw[4])
    feas = want["feasible"].reshape(B, K) == 1
    assert (feas.any(axis=1) & ~feas.all(axis=1)).any()
    assert_views(plan, want, B, K)
    assert np.array_equal(bits(host(plan.score_con_t)), bits(want["score"])) and np.array_equal(host(plan.failed_con_t), want["failed_out"])
    sel = plan.select()
    order = I.lexicographic_order(K, host(raw[0]).reshape(-1), want["feasible"], want["excess"], want["failed_out"])
    assert np.array_equal(host(sel["best_k"]), order[:, 0].astype(np.int32))
    best_feasible = host(sel["best_feasible"])
    assert np.array_equal(best_feasible == 1, want["n_feasible"] > 0) and np.array_equal(host(sel["n_feasible"]), want["n_feasible"])
    ret = host(raw[0])
    for b in range(B):                                                      # best_return is the score: the return where feasible
        if best_feasible[b]:
            assert host(sel["best_return"])[b] == ret[b, order[b, 0]]
    env.close()


# ---- 3. scenarios: a chance constraint over the sampled futures ------------------------------------------------------------------------
def test_scenarios_and_n_allow():
    B, K, S, H = 2, 4, 3, 4
    env = started(B, "float32", uncertainty_scale=0.3)
    actions = rand_actions((H, B * K, 6), 12, env.device)
    kw = dict(gamma=0.97, n_scenarios=S, scenario_seed=5)
    plain = env.planner(K, H, **kw)
    raw = [t.clone() for t in plain.rollout(actions)]
    per = host(plain.viol_T)[:, :plain.C] / np.maximum(host(plain.n_steps_t), 1)        # per run
    # the budget between the largest and the second-largest run of one candidate: exactly one of its futures is over the line
    runs = np.sort(per.reshape(3, B * K, S), axis=2)
    gap = runs[:, :, S - 1] - runs[:, :, S - 2]
    which, j = np.unravel_index(np.argmax(gap), gap.shape)
    assert gap[which, j] > 0.0, "no candidate's violations differ between its scenarios"
    budget = float(0.5 * (runs[which, j, S - 1] + runs[which, j, S - 2]))
    assert runs[which, j, S - 2] <= budget < runs[which, j, S - 1]
    which = int(which)
    feasible = []
    for n_allow in (0, 1):
        con = with_budget(which, budget, n_allow=n_allow)
        plan = env.planner(K, H, constraints=con, **kw)
        out = plan.rollout(actions)
        for a, b in zip(out, raw):
            assert same_bits(a, b)
        assert same_bits(plan.viol_T, plain.viol_T) and same_bits(plan.n_steps_t, plain.n_steps_t)
        want = restate(plan, con, B, 1, K, raw[0], raw[4])
        assert_views(plan, want, B, K)
        assert np.array_equal(bits(host(plan.score_con_t)), bits(want["score"]))
        feasible.append(want["feasible"])
    print("feasible with n_allow = 0 / 1:", feasible)
    assert not np.array_equal(feasible[0], feasible[1])
    env.close()


# ---- 4. the searches --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rule", "policy_greenhouse", "policy_all"])
def test_searches_rank_the_constrained_scores(kind):
    import torch
    from test_gpu_plan_policy import rand_theta, spec_for
    from test_gpu_plan_rule import TUNE
    B, K, S, H = 3, 4, 2, 3
    env = started(B, "float32", uncertainty_scale=0.3, pred_horizon=0.0)
    kw = dict(gamma=0.97, n_scenarios=S, scenario_seed=5)
    spec = spec_for(env) if kind != "rule" else None

    def build(**more):
        if kind == "rule":
            return env.rule_search(K, H, tune=TUNE, **kw, **more)
        return env.policy_search(K, H, spec, share=kind.split("_")[1], **kw, **more)

    plain = build()
    theta = rand_theta(plain, 4) if kind != "rule" else (torch.rand(plain.Ht, plain.J, 6, generator=torch.Generator().manual_seed(4)) * 2
                                                          - 1).to(env.device).contiguous()
    raw = [t.clone() for t in plain.rollout(theta)]
    per = host(plain.plan.viol_T)[:, :plain.C] / np.maximum(host(plain.plan.n_steps_t), 1)
    which = next((i for i in (2, 1, 0) if np.unique(per[i]).size > 2), None)
    assert which is not None
    con = with_budget(which, float(np.median(per[which])), n_allow=1, weights=(0.5, 2.0, 1.0))
    s = build(constraints=con)
    out = s.rollout(theta)
    for a, b in zip(out, raw):
        assert same_bits(a, b)
    if kind == "policy_all":
        P, O = 1, B
        assert same_bits(s._mean_ret_t, plain.score_t) and same_bits(s._any_failed_t, plain.score_failed_t)
        want = restate(s.plan, con, P, O, K, plain.score_t, plain.score_failed_t)
    else:
        P, O = B, 1
        want = restate(s.plan, con, P, O, K, raw[0], raw[4])
    assert np.array_equal(bits(host(s.score_t)), bits(want["score"])) and np.array_equal(host(s.score_failed_t), want["failed_out"])
    assert_views(s, want, P, K)
    sel = s.select()
    order = I.lexicographic_order(K, host(plain.score_t).reshape(-1), want["feasible"], want["excess"], want["failed_out"])
    assert np.array_equal(host(sel["best_k"]), order[:, 0].astype(np.int32))
    assert np.array_equal(host(sel["best_feasible"]) == 1, want["n_feasible"] > 0)
    env.close()


# ---- 5. cem ---------------------------------------------------------------------------------------------------------------------------
def test_cem_under_infinite_budgets_is_the_unconstrained_cem():
    from gl_gym_amd.planner import Constraints
    B, K, H, E_ = 2, 16, 4, 4
    env = started(B, "float32")
    outs = []
    for con in (None, Constraints()):
        plan = env.planner(K, H, gamma=0.97, constraints=con)
        o = plan.cem(2, E_, carry=1, beta=0.5, seed=3)
        outs.append([t.clone() for t in (o["best_k"], o["mean_sequence"], o["std_sequence"], o["best_return"], o["elite_k"])])
        if con is not None:
            assert bool(o["best_feasible"].all()) and host(o["n_feasible"]).tolist() == [K] * B
    for a, b in zip(*outs):
        assert same_bits(a, b)
    env.close()


def test_constrained_cem_replays_from_a_captured_graph():
    import torch
    B, K, H, E_ = 2, 16, 4, 4
    env = started(B, "float32")
    plain = env.planner(K, H, gamma=0.97)
    raw = plain.rollout(rand_actions((H, B * K, 6), 11, env.device))
    which, budget = median_budget(host(raw[3]), host(raw[2]))
    assert which is not None
    plan = env.planner(K, H, gamma=0.97, constraints=with_budget(which, budget))

    def decision():
        plan._draw = 0
        return plan.cem(2, E_, carry=1, beta=0.5, seed=3)

    def outputs():
        return [plan.score_con_t, plan.failed_con_t, plan.feasible_t, plan.excess_t, plan.n_viol_t, plan.n_feasible_t, plan.cem_mean_t,
                plan.cem_std_t, plan.best_k_t, plan.best_ret_t, plan.best_sequence_t, plan._con.best_feasible_t]

    decision()
    eager = [t.clone() for t in outputs()]
    print(f"feasible candidates of the last population: {int(eager[2].sum())} of {B * K}")
    side = torch.cuda.Stream(device=env.device)
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        decision()
    torch.cuda.current_stream(env.device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        decision()
    outs = outputs()
    for t in outs:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize(env.device)
    for t, e in zip(outs, eager):
        assert same_bits(t, e)
    env.close()
