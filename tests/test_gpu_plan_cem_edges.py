"""glgym_plan_sample, glgym_plan_elites and glgym_plan_refit through the C ABI on guarded buffers, against plan_inputs.np_sample,
test_plan_cem_host.np_elites and np_refit with the bounds of tests/test_plan_cem_host.py: reserved candidates, copies, elite rows and
n_elite exact, sampled actions within np.spacing(np.float32(1)) of the float64 restatement, refitted values within one float32 ulp.
sample: P*K on both sides of a wavefront (1, 63, 64, 65, 128, 129, the last with a wavefront over two parents), horizons whose last
group of four steps is short, full, or one step, carried elites with counts 0, 1, 4 and 9 and with indices that are not followed.
elites: K on both sides of the 64-key chunk and the 256-key tile, whole parents of equal returns, ties on the chunk and tile boundaries,
E - 1, E, E + 1 admissible candidates.  refit: counts outside 0..E, rows with an index outside 0..K-1, in place and out of place."""
import numpy as np
import pytest

import plan_inputs as I
from test_plan_inputs_host import check_elites_pattern, check_refit_variant

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hd():
    h = I.Handle(False)
    yield h
    h.close()


# ---- sample -------------------------------------------------------------------------------------------------------------------------
def run_sample(hd, P, K, H, mean, std, beta, base, carry=0, prev_E=0, prev=None, elite=None, n_elite=None):
    src = dict(mean=mean, std=std)
    if carry:
        src.update(prev_actions=prev, prev_elite_k=elite, prev_n_elite=n_elite)
    ins = I.guarded(src)
    word, word_ptr, _ = I.draw_word(base)
    out = I.Guarded(shape=(H, P * K, I.NU), dtype=np.float32)
    p = {k: g.ptr for k, g in ins.items()}
    L = hd.L
    a = L.make_plan_args(L.PlanSampleArgs, P, K, H, p["mean"], p["std"], beta, I.SEED, I.DRAW, word_ptr, out.ptr, carry, prev_E,
                         p.get("prev_actions"), p.get("prev_elite_k"), p.get("prev_n_elite"))
    I.launch(hd, "glgym_plan_sample", a)
    I.assert_only_read(ins, src)
    if word is not None:
        assert word.read()[0] == I.BASE
    got = out.read()
    assert not np.isnan(got).any(), "a row of the block was not written"
    return got


@pytest.mark.parametrize("base", [False, True], ids=["nobase", "base"])
@pytest.mark.parametrize("P,K,H,beta", I.SAMPLE_COMBOS)
def test_sample_shapes_and_carried_elites(hd, P, K, H, beta, base):
    mean, std, prev = I.sample_case(P, K, H)
    D = I.DRAW + (I.BASE if base else 0)
    fresh = run_sample(hd, P, K, H, mean, std, beta, base)                       # carry = 0, every prev_ pointer NULL
    exp, exact = I.np_sample(P, K, H, mean, std, beta, I.SEED, D)
    err = np.abs(fresh.astype(np.float64) - exp).max()
    print(f"sample P={P} K={K} H={H} beta={beta}: max |action - float64 restatement| = {err:.2e} (bound {I.F32_STEP:.2e})")
    assert err <= I.F32_STEP and (np.abs(fresh) <= 1).all()
    assert np.array_equal(I.bits(fresh[:, exact]), I.bits(exp[:, exact].astype(np.float32)))         # candidate 0: the clipped mean
    for invalid in (False, True):
        carry, elite, n_elite = I.carry_tables(P, K, invalid)
        got = run_sample(hd, P, K, H, mean, std, beta, base, carry, carry, prev, elite, n_elite)
        exp, exact = I.np_sample(P, K, H, mean, std, beta, I.SEED, D, carry, carry, prev, elite, n_elite)
        assert np.abs(got.astype(np.float64) - exp).max() <= I.F32_STEP and (np.abs(got) <= 1).all()
        assert np.array_equal(I.bits(got[:, exact]), I.bits(exp[:, exact].astype(np.float32)))       # copies: the previous block's rows
        assert np.array_equal(I.bits(got[:, ~exact]), I.bits(fresh[:, ~exact]))  # sampled, or not followed: the carry = 0 run's child
        for p in range(P):
            for k in range(1, min(carry, K - 1) + 1):
                e = elite[p, k - 1]
                followed = k - 1 < n_elite[p] and 0 <= e < K
                assert exact[p * K + k] == followed
                src = prev[:, p * K + e] if followed else fresh[:, p * K + k]
                assert np.array_equal(I.bits(got[:, p * K + k]), I.bits(src)), (p, k, int(e))


# ---- elites -------------------------------------------------------------------------------------------------------------------------
def run_elites(hd, P, K, E, ret, failed):
    src = dict(ret=ret, failed=failed)
    ins = I.guarded(src)
    elite, n_elite = I.Guarded(shape=(P, E), dtype=np.int32), I.Guarded(shape=(P,), dtype=np.int32)
    L = hd.L
    a = L.make_plan_args(L.PlanElitesArgs, P, K, E, ins["ret"].ptr, ins["failed"].ptr, elite.ptr, n_elite.ptr)
    I.launch(hd, "glgym_plan_elites", a)
    I.assert_only_read(ins, src)
    return elite.read(), n_elite.read()


@pytest.mark.parametrize("pattern", I.ELITE_PATTERNS)
@pytest.mark.parametrize("P,K,E", I.ELITE_SHAPES)
def test_elites_shapes_and_tie_patterns(hd, P, K, E, pattern):
    ret, failed = I.elites_case(P, K, E, pattern)
    got = run_elites(hd, P, K, E, ret, failed)
    exp = I.np_elites(P, K, E, ret, failed)
    assert np.array_equal(got[1], exp[1]), (got[1], exp[1])
    wrong = got[0] != exp[0]
    assert not wrong.any(), f"{wrong.sum()} slots differ, the first at (p, slot) = {np.argwhere(wrong)[:4].tolist()}"     # the -1 tail included
    check_elites_pattern(P, K, E, pattern, ret, exp)


# ---- refit --------------------------------------------------------------------------------------------------------------------------
def run_refit(hd, P, K, H, E, actions, elite, n_elite, alpha, min_std, mean, std, in_place=False):
    src = dict(actions=actions, elite_k=elite, n_elite=n_elite, mean=mean, std=std)
    ins = I.guarded(src)
    mo = ins["mean"] if in_place else I.Guarded(shape=mean.shape, dtype=np.float32)
    so = ins["std"] if in_place else I.Guarded(shape=std.shape, dtype=np.float32)
    L = hd.L
    a = L.make_plan_args(L.PlanRefitArgs, P, K, H, E, ins["actions"].ptr, ins["elite_k"].ptr, ins["n_elite"].ptr, alpha, min_std,
                         ins["mean"].ptr, ins["std"].ptr, mo.ptr, so.ptr)
    I.launch(hd, "glgym_plan_refit", a)
    if in_place:
        ins.pop("mean"); ins.pop("std")
    I.assert_only_read(ins, src)
    return mo.read(), so.read()


@pytest.mark.parametrize("alpha,min_std", I.REFIT_PARAMS)
@pytest.mark.parametrize("variant", I.REFIT_VARIANTS)
@pytest.mark.parametrize("P,K,H,E", I.REFIT_SHAPES)
def test_refit_counts_rows_and_parameters(hd, P, K, H, E, variant, alpha, min_std):
    actions, elite, n_elite, n_ref, mean, std = I.refit_case(P, K, H, E, variant)
    mo, so = run_refit(hd, P, K, H, E, actions, elite, n_elite, alpha, min_std, mean, std)
    e_mo, e_so = I.refit_reference(P, K, H, actions, elite, n_ref, alpha, min_std, mean, std)
    assert not np.isnan(mo).any() and not np.isnan(so).any()
    assert I.within_one_f32_ulp(mo, e_mo), np.abs(mo - e_mo).max()
    assert I.within_one_f32_ulp(so, e_so), np.abs(so - e_so).max()
    check_refit_variant(P, variant, alpha, min_std, n_ref, mean, std, mo, so)
    mi, si = run_refit(hd, P, K, H, E, actions, elite, n_elite, alpha, min_std, mean, std, in_place=True)
    assert np.array_equal(I.bits(mi), I.bits(mo)) and np.array_equal(I.bits(si), I.bits(so))         # in place = out of place
