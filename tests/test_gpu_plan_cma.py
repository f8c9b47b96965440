"""The CMA-ES stages on the GPU: glgym_plan_cma_sample and glgym_plan_cma_update (include/glgym.h) through the C ABI on guarded buffers
against the host build of csrc/gl_cma.hpp, and RuleSearch.cma (gl_gym_amd.planner).

Bounds, those of tests/test_plan_cma_host.py.  Sampled theta: within np.spacing(np.float32(1)) of the float64 restatement (and so within
one float32 ulp of the host build); padding slots exactly 0.  The update: status, p_sigma', p_c', mean', cov' and chol' are the host
build's to the last bit (+, -, *, /, sqrt in the stated order); sigma' within 4 * 2^-52 relative (exp of another libm).  Rows that are
not updated keep every bit, and every buffer has guards in front and behind.  Everything at class level is compared bit for bit: an
iteration's returns against rollout() of its block, cma() against the loop over its parts, a captured graph against the eager call.
Child batches stay <= 800 rows and horizons <= 2 steps."""
import numpy as np
import pytest

import envlayer_inputs as E
from test_gpu_plan import same_bits
from test_gpu_plan_rule import TUNE, started
from test_plan_cem_host import F32_STEP
from test_plan_cma_host import (FEW_ELITES, HYPER, NOT_FINITE, NOT_POSITIVE, SIGMA_RTOL, STATE, UPDATED, build_host, elites_of, flat, hyper_of,
                                make_state, np_cma_sample, planes, run_sample as host_sample, run_update as host_update)
from test_plan_es_host import within_f32_ulps

pytestmark = pytest.mark.gpu
SEED, DRAW, BASE = 0xDEADBEEF12345678, (7 << 32) | 41, (3 << 32) | 5


@pytest.fixture(scope="module")
def hd():
    h = E.Handle(False)
    yield h
    h.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("cmahost_gpu") / "libcmahost.so")


def same_np(a, b):
    return np.array_equal(E.bits(a), E.bits(np.ascontiguousarray(b)))


def launch(hd, name, a):
    import ctypes as C
    hd.sync()
    rc = getattr(hd.lib, name)(hd.h, C.byref(a), hd.stream())
    hd.sync()
    assert rc == 0, (name, rc, hd.error())


def dev_sample(hd, P, K, N, st, base):
    g = [E.Guarded(st[k]) for k in ("mean", "sigma", "chol")]
    word = E.Guarded(np.array([BASE], np.uint64)) if base else None
    out = E.Guarded(shape=(planes(N), P * K, 6), dtype=np.float32)
    L = hd.L
    launch(hd, "glgym_plan_cma_sample", L.make_plan_args(L.PlanCmaSampleArgs, P, K, N, g[0].ptr, g[1].ptr, g[2].ptr, SEED, DRAW,
                                                        word.ptr if base else None, out.ptr))
    for x, k in zip(g, ("mean", "sigma", "chol")):
        assert same_np(x.read(), st[k]), f"input {k} was written"
    assert word is None or word.read()[0] == BASE
    got = out.read()
    assert not np.isnan(got).any(), "a row of the block was not written"
    return got


def dev_update(hd, P, K, N, E_, theta, elite, n_elite, hp, t, st, base):
    """-> the row state after the call and status, read back through the guards."""
    g = {k: E.Guarded(st[k]) for k in STATE}
    ro = {k: E.Guarded(v) for k, v in dict(theta=theta, elite=elite, n_elite=n_elite, w=hp["w"]).items()}
    status = E.Guarded(shape=(P,), dtype=np.int32)
    word = E.Guarded(np.array([BASE], np.uint64)) if base else None
    w_host = np.ascontiguousarray(hp["w"])
    L = hd.L
    a = L.make_plan_args(L.PlanCmaUpdateArgs, P, K, N, E_, ro["theta"].ptr, ro["elite"].ptr, ro["n_elite"].ptr, w_host.ctypes.data, ro["w"].ptr,
                         *(hp[k] for k in HYPER), t - (BASE if base else 0), word.ptr if base else None, *(g[k].ptr for k in STATE), status.ptr)
    launch(hd, "glgym_plan_cma_update", a)
    for k, v in dict(theta=theta, elite=elite, n_elite=n_elite, w=hp["w"]).items():
        assert same_np(ro[k].read(), v), f"input {k} was written"
    res = {k: g[k].read() for k in STATE}
    res["status"] = status.read()
    return res


def check_against_host(got, exp, st):
    assert np.array_equal(got["status"], exp["status"]), (got["status"], exp["status"])
    for k in ("mean", "cov", "chol", "p_sigma", "p_c"):
        assert same_np(got[k], exp[k]), (k, np.abs(got[k].astype(np.float64) - exp[k]).max())
    assert (np.abs(got["sigma"] - exp["sigma"]) <= SIGMA_RTOL * np.abs(exp["sigma"])).all(), (got["sigma"], exp["sigma"])
    keep = exp["status"] != UPDATED
    for k in ("sigma", "cov", "chol", "p_sigma", "p_c"):
        assert same_np(got[k][keep], st[k][keep]), k
    assert same_np(got["mean"][:, keep], st["mean"][:, keep])


# ---- 1. both stages through the C ABI against the host build --------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 7, 32])
@pytest.mark.parametrize("K", [2, 66, 258])
@pytest.mark.parametrize("P", [1, 3])
def test_the_stages_equal_the_host_build(hd, host, P, K, N):
    rng = np.random.default_rng(1000 * N + 10 * K + P)
    st = make_state(rng, P, N)
    if N > 1:
        st["mean"][0, 0, 0] = 1.0                                        # a mean on the box
    for base in (False, True):                                           # sample, with and without the device word
        D = DRAW + (BASE if base else 0)
        theta = dev_sample(hd, P, K, N, st, base)
        err = np.abs(theta.astype(np.float64) - np_cma_sample(P, K, N, st["mean"], st["sigma"], st["chol"], SEED, D)).max()
        assert err <= F32_STEP and (np.abs(theta) <= 1).all(), err
        assert within_f32_ulps(theta, host_sample(host, P, K, N, st["mean"], st["sigma"], st["chol"], SEED, D).astype(np.float64), 1)
        assert same_np(flat(theta, planes(N) * 6)[:, N:], np.zeros((P * K, planes(N) * 6 - N), np.float32))
    for E_ in sorted({1, max(1, K // 2)}):
        hp = hyper_of(N, K, E_)
        elite, n_elite = elites_of(rng, P, K, E_)
        if P > 1:
            n_elite[P - 1] = E_ - 1                                      # the last row has too few elites: it is kept
        for t, base in ((1, False), (BASE + 1000, True)):
            got = dev_update(hd, P, K, N, E_, theta, elite, n_elite, hp, t, st, base)
            exp = host_update(host, P, K, N, E_, theta, elite, n_elite, hp, t, **st)
            check_against_host(got, exp, st)
            assert got["status"].tolist() == [UPDATED] * (P - 1) + [FEW_ELITES if P > 1 else UPDATED]
            assert not same_np(got["cov"][0], st["cov"][0]) and not same_np(got["mean"][:, 0], st["mean"][:, 0])


@pytest.mark.parametrize("N,K", [(1, 700), (5, 700), (7, 600), (32, 130)])
def test_update_with_more_elites_than_a_tile(hd, host, N, K):
    """The kernel stages min(256, 1 024 // N) elites per round: E = K / 2 = 350 / 350 / 300 / 65 elites take 2 / 2 / 3 / 3 rounds, the
    last one partly filled.  The tile depth changes no bit: every sum runs in e ascending inside its owner."""
    P, E_ = 2, K // 2
    assert E_ > min(256, 1024 // N)
    rng = np.random.default_rng(10 * N + K)
    st = make_state(rng, P, N)
    hp = hyper_of(N, K, E_)
    theta = host_sample(host, P, K, N, st["mean"], st["sigma"], st["chol"], 3, 4)
    elite, n_elite = elites_of(rng, P, K, E_)
    got = dev_update(hd, P, K, N, E_, theta, elite, n_elite, hp, 2, st, False)
    exp = host_update(host, P, K, N, E_, theta, elite, n_elite, hp, 2, **st)
    check_against_host(got, exp, st)
    assert got["status"].tolist() == [UPDATED, UPDATED]


def test_rows_that_are_not_updated_keep_every_bit(hd, host):
    P, K, N, E_ = 6, 66, 7, 33
    rng = np.random.default_rng(6)
    st = make_state(rng, P, N)
    hp = hyper_of(N, K, E_)
    theta = host_sample(host, P, K, N, st["mean"], st["sigma"], st["chol"], 1, 2)
    elite, n_elite = elites_of(rng, P, K, E_)
    elite[0, 5] = -1                                                      # 1: an index of -1
    elite[1, E_ - 1] = K                                                  # 1: an index of K
    theta[1, 2 * K + elite[2, 4], 0] = np.nan                             # 2: a NaN in an elite's theta (component 6)
    st["cov"][3] = -np.eye(N)                                             # 3: a cov made indefinite by hand
    st["p_sigma"][4] = 50.0                                               # 0, with h_sigma false
    got = dev_update(hd, P, K, N, E_, theta, elite, n_elite, hp, 3, st, False)
    exp = host_update(host, P, K, N, E_, theta, elite, n_elite, hp, 3, **st)
    assert exp["status"].tolist() == [FEW_ELITES, FEW_ELITES, NOT_FINITE, NOT_POSITIVE, UPDATED, UPDATED]
    check_against_host(got, exp, st)


# ---- 2. RuleSearch.cma ------------------------------------------------------------------------------------------------------------------
HP = dict(init_sigma=0.3, seed=9)
B_, K_, H_ = 2, 8, 2


def tune_of(n):
    return {k: TUNE[k] for k in ("temp_setpoint_day", "co2_day", "rh_max")[:n]}


def cma_outputs(rs):
    st, p = rs._cma(), rs.plan
    return [rs._theta, p.ret_t, p._score_t, p._score_failed_t, rs.mean_t, st.sigma_t, st.cov_t, st.chol_t, st.p_sigma_t, st.p_c_t, st.status_t,
            rs.elite_k_t[:rs.B * (rs.K // 2)], rs.n_elite_t, p.best_k_t, rs.best_theta_t]    # the elite slots that E = K // 2 uses


def by_parts(rs, first, n_iter):
    """cma() as the loop over its parts: the generations first .. first + n_iter - 1 of a search that is (first = 0) or was started."""
    if first == 0:
        rs._es_start()
        rs._cma().restart(HP["init_sigma"])
    for it in range(first, first + n_iter):
        block = rs.sample_cma(seed=HP["seed"], draw_index=it)
        rs.rollout(block)
        status = rs.cma_update()
    return rs.select(), status


@pytest.mark.parametrize("n_tune,kw", [(3, {}), (2, {"n_scenarios": 2})])
def test_cma_equals_its_parts(n_tune, kw):
    import torch
    env = started(B_, "float32")
    mk = lambda: env.rule_search(K_, H_, tune=tune_of(n_tune), gamma=0.97, **kw)  # noqa: E731
    rs = mk()
    out = rs.cma(1, **HP)
    block, ret, score = rs._theta.clone(), rs.plan.ret_t.clone(), rs.plan._score_t.clone()
    other = mk()
    other.rollout(block)
    assert same_bits(other.plan.ret_t, ret) and same_bits(other.plan._score_t, score)   # an iteration's returns are rollout() of its block
    assert float(block.abs().max()) <= 1.0 and float(block.view(-1, 6)[:, n_tune:].abs().max()) == 0.0
    assert out["sigma"].shape == (B_,) and out["cov"].shape == (B_, n_tune, n_tune) and out["status"].cpu().tolist() == [0] * B_
    assert out["mean"].shape == (1, B_, 6) and out["best_theta"].shape == (B_, 6) and set(out["best_params"]) == set(tune_of(n_tune))
    assert same_bits(out["cov"], out["cov"].transpose(1, 2)) and not same_bits(out["cov"], torch.eye(n_tune, dtype=torch.float64, device=env.device).expand(B_, -1, -1))
    whole, parts = mk(), mk()
    res = whole.cma(2, **HP)
    sel, _ = by_parts(parts, 0, 2)
    for a, b in zip(cma_outputs(whole), cma_outputs(parts)):
        assert same_bits(a, b)
    for k in ("best_k", "best_return", "best_theta"):
        assert same_bits(res[k], sel[k]), k
    assert whole._cma().t == 2 and torch.isfinite(whole.mean_t).all()
    # resume continues where one more generation of the loop arrives; a plain call starts again
    whole.cma(1, resume=True, **HP)
    by_parts(parts, 2, 1)
    for a, b in zip(cma_outputs(whole), cma_outputs(parts)):
        assert same_bits(a, b)
    assert whole._cma().t == 3
    whole.cma(1, **HP)
    assert whole._cma().t == 1 and not same_bits(whole._cma().cov_t, parts._cma().cov_t)
    env.close()


def test_cma_replays_from_a_captured_graph():
    import torch
    env = started(B_, "float32")
    rs = env.rule_search(K_, H_, tune=tune_of(3), gamma=0.97, n_scenarios=2)
    rs.cma(1, **HP)                           # the first call allocates

    def decision():
        rs._draw = 0                          # the same draw indices every time: what differs between runs is draw_base_t alone
        return rs.cma(2, **HP)

    decision()
    eager = [t.clone() for t in cma_outputs(rs)]
    side = torch.cuda.Stream(device=env.device)
    side.wait_stream(torch.cuda.current_stream(env.device))
    with torch.cuda.stream(side):
        decision()
    torch.cuda.current_stream(env.device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        decision()
    outs = cma_outputs(rs)
    for t in outs[1:]:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize(env.device)
    for t, e in zip(outs, eager):
        assert same_bits(t, e)
    rs.plan.draw_base_t += 2                  # the device word behind draw_base moves: the replay samples another population
    graph.replay()
    torch.cuda.synchronize(env.device)
    replayed = [t.clone() for t in outs]
    assert not same_bits(replayed[0], eager[0]) and not same_bits(replayed[1], eager[1]) and not same_bits(replayed[6], eager[6])
    decision()                                # eager at the same draw_base: the same bits again
    for t, e in zip(cma_outputs(rs), replayed):
        assert same_bits(t, e)
    env.close()


def test_a_row_without_admissible_candidates_keeps_its_state_and_wrong_arguments_are_refused():
    env = started(B_, "float32")
    rs = env.rule_search(K_, H_, tune=tune_of(3), gamma=0.97)
    rs.cma(1, **HP)
    st = rs._cma()
    block = rs.sample_cma(seed=1, draw_index=7)
    rs.rollout(block)
    rs.plan._score_failed_t.view(B_, K_)[0] = 1                  # greenhouse 0: every candidate failed
    state = (rs.mean_t, st.sigma_t, st.cov_t, st.chol_t, st.p_sigma_t, st.p_c_t)
    before = [t.clone() for t in state]
    status = rs.cma_update()
    assert status.cpu().tolist() == [1, 0] and rs.n_elite_t.cpu().tolist() == [0, K_ // 2]
    for t, b in zip(state, before):
        row = (lambda x: x[:, 0:1]) if t is rs.mean_t else (lambda x: x[0:1])
        other = (lambda x: x[:, 1:2]) if t is rs.mean_t else (lambda x: x[1:2])
        assert same_bits(row(t), row(b)) and not same_bits(other(t), other(b))
    assert rs.cma_t_base.shape == (1,) and set(rs.cma_state) == {"sigma", "cov", "chol", "p_sigma", "p_c", "status"}
    for bad in (dict(n_iter=0), dict(n_elite=0), dict(n_elite=K_ + 1), dict(init_sigma=0.0), dict(min_sigma=-1.0), dict(min_sigma=2.0),
                dict(max_sigma=float("inf")), dict(c_sigma=1.5), dict(c_1=0.9, c_mu=0.9), dict(d_sigma=0.0), dict(chi_n=float("nan")),
                dict(mu_eff=-1.0), dict(w=[0.5, 0.6, -0.1, 0.0]), dict(w=[1.0]), dict(seed=-1), dict(resume=True, mean=rs.mean_t)):
        with pytest.raises(ValueError):
            rs.cma(**{"n_iter": 1, **HP, **bad})
    with pytest.raises(TypeError):
        rs.cma(1, lr=0.1)
    whole = env.rule_search(K_, H_, tune=all_constants())         # the whole controller fits: D = 29, five planes
    out = whole.cma(1, **HP)
    assert whole.D == 29 and out["cov"].shape == (B_, 29, 29) and out["status"].cpu().tolist() == [0, 0]
    env.close()


def all_constants():
    """Every constant of the controller within 10 % of its default (a proportional band's interval must not contain 0)."""
    from gl_gym_amd import _lib as L
    from gl_gym_amd.baseline import RuleBasedController
    base, tune = RuleBasedController(), {}
    for n in L.RULE_FIELDS:
        v = float(getattr(base, n))
        r = 0.1 * abs(v) + (0.0 if n in L.RULE_BANDS else 0.01)
        tune[n] = (v - r, v + r)
    return tune
