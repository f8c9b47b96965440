"""glgym_plan_select (plan_select_kernel, plan_mean_kernel) through the C ABI on guarded buffers, against test_plan_host.np_select with
the bounds of test_gpu_plan.test_select_on_device_returns: indices, returns and gathered rows exact, the MPPI mean within one float32
ulp of NumPy's rounded mean.  K on both sides of the 64-lane stride and of the butterfly's empty lanes (1, 63, 64, 65, 128, 129, 640),
horizons whose H*6 sequence entries need one, two, three and five rounds of the gather loop (6, 60, 66, 132, 288); the best at the last
k, exact ties across two lanes and inside one, -0.0 against +0.0, parents without an admissible candidate; every subset of the three
action outputs; temperatures from 1e-300 to 1e300, and the refusal of one whose reciprocal is not finite."""
import itertools

import numpy as np
import pytest

import plan_inputs as I
from test_plan_inputs_host import check_pattern

pytestmark = pytest.mark.gpu

OUTPUTS = ("best_action", "best_sequence", "mean_sequence")


@pytest.fixture(scope="module")
def hd():
    h = I.Handle(False)
    yield h
    h.close()


def run_select(hd, P, K, H, ret, failed, actions, temperature=0.0, want=OUTPUTS, with_actions=True, expect=0):
    """One glgym_plan_select -> {output: array, or None if it was not asked for}; the outputs asked for are read with their guards, the
    inputs compared with what was put in."""
    src = dict(ret=ret, failed=failed, actions=actions)
    ins = I.guarded(src)
    outs = dict(best_k=I.Guarded(shape=(P,), dtype=np.int32), best_ret=I.Guarded(shape=(P,), dtype=np.float64),
                best_action=I.Guarded(shape=(P, I.NU), dtype=np.float32), best_sequence=I.Guarded(shape=(H, P, I.NU), dtype=np.float32),
                mean_sequence=I.Guarded(shape=(H, P, I.NU), dtype=np.float32))
    ptr = {k: (outs[k].ptr if k in want else None) for k in OUTPUTS}
    L = hd.L
    a = L.make_plan_args(L.PlanSelectArgs, P, K, H, ins["ret"].ptr, ins["failed"].ptr, ins["actions"].ptr if with_actions else None,
                         outs["best_k"].ptr, outs["best_ret"].ptr, ptr["best_action"], ptr["best_sequence"], temperature, ptr["mean_sequence"])
    msg = I.launch(hd, "glgym_plan_select", a, expect)
    I.assert_only_read(ins, src)
    got = {k: g.read() for k, g in outs.items()}
    for k in OUTPUTS:
        if k not in want or expect:
            assert outs[k].untouched(), f"{k} was written"
            got[k] = None
    if expect:
        assert outs["best_k"].untouched() and outs["best_ret"].untouched()
    got["error"] = msg
    return got


def check_select(got, exp, want=OUTPUTS):
    e_k, e_ret, e_act, e_seq, e_mean = exp
    ok = e_k >= 0
    assert np.array_equal(got["best_k"], e_k)
    assert np.array_equal(I.bits(got["best_ret"][ok]), I.bits(e_ret[ok])) and np.isnan(got["best_ret"][~ok]).all()
    if "best_action" in want:
        assert np.array_equal(I.bits(got["best_action"]), I.bits(e_act))
    if "best_sequence" in want:
        wrong = I.bits(got["best_sequence"]) != I.bits(e_seq)
        assert not wrong.any(), f"best_sequence: {wrong.sum()} entries differ, the first at (h, p, j) = {np.argwhere(wrong)[:4].tolist()}"
    if "mean_sequence" in want:
        assert I.within_one_f32_ulp(got["mean_sequence"], e_mean), np.abs(got["mean_sequence"] - e_mean).max()


@pytest.mark.parametrize("pattern", I.SELECT_PATTERNS)
@pytest.mark.parametrize("P,K,H", I.SELECT_SHAPES)
def test_select_shapes_and_return_patterns(hd, P, K, H, pattern):
    ret, failed, actions = I.select_case(P, K, H, pattern)
    got = run_select(hd, P, K, H, ret, failed, actions, 0.05)
    exp = I.select_reference(P, K, ret, failed, actions, 0.05)
    check_select(got, exp)
    check_pattern(P, K, pattern, ret, failed, exp)
    if pattern == "zeros":
        assert (I.bits(got["best_ret"]) == 1 << 63).all()                       # the bits of the lower k's -0.0


@pytest.mark.parametrize("P,K,H", I.SELECT_SHAPES)
def test_select_output_subsets(hd, P, K, H):
    ret, failed, actions = I.select_case(P, K, H, "random", seed=1)
    exp = I.select_reference(P, K, ret, failed, actions, 1.0)
    full = run_select(hd, P, K, H, ret, failed, actions, 1.0)
    check_select(full, exp)
    for n in range(len(OUTPUTS)):
        for want in itertools.combinations(OUTPUTS, n):
            got = run_select(hd, P, K, H, ret, failed, actions, 1.0, want)
            check_select(got, exp, want)
            for k in ("best_k", "best_ret") + want:                             # whatever is written has the same bits in every subset
                assert np.array_equal(I.bits(got[k]), I.bits(full[k])), (k, want)
    got = run_select(hd, P, K, H, ret, failed, actions, 0.0, (), with_actions=False)
    check_select(got, exp, ())


@pytest.mark.parametrize("temperature", I.SELECT_TEMPERATURES)
@pytest.mark.parametrize("P,K,H", [I.SELECT_SHAPES[i] for i in (0, 3, 5, 6, 11)])
def test_select_temperatures(hd, P, K, H, temperature):
    ret, failed, actions = I.select_case(P, K, H, "ties" if K > 1 else "random")
    got = run_select(hd, P, K, H, ret, failed, actions, temperature)
    check_select(got, I.select_reference(P, K, ret, failed, actions, temperature))
    for p in range(P):
        r, f, a = ret[p * K:(p + 1) * K], failed[p * K:(p + 1) * K], actions[:, p * K:(p + 1) * K].astype(np.float64)
        adm = (f == 0) & np.isfinite(r)
        if temperature == 1e-300:                                               # the mean over the exactly tied maxima
            tied = adm & (r == r[adm].max())
            assert tied.sum() == (2 if K > 1 else 1)
            assert I.within_one_f32_ulp(got["mean_sequence"][:, p], a[:, tied].mean(axis=1))
        if temperature == 1e300:                                                # the plain mean over the admissible candidates
            assert I.within_one_f32_ulp(got["mean_sequence"][:, p], a[:, adm].mean(axis=1))


def test_a_temperature_without_a_finite_reciprocal_is_refused(hd):
    """Before the refusal the device returned NaN in all 36 entries of mean_sequence for temperature = 5e-324 (1 / temperature = +inf, the
    best candidate's own (ret - max) * inf = 0 * inf); now the call is GLGYM_EINVAL with every output untouched, and the smallest
    temperature whose reciprocal is finite gives the mean over the tied maxima."""
    P, K, H = 3, 65, 2
    ret, failed, actions = I.select_case(P, K, H, "ties")
    edge = float(np.nextafter(2.0 ** -1024, 1.0))
    for bad in (I.SMALLEST_SUBNORMAL, 2.0 ** -1024):
        got = run_select(hd, P, K, H, ret, failed, actions, bad, expect=hd.L.EINVAL)
        assert "glgym_plan_select: temperature is too small" in got["error"]
    got = run_select(hd, P, K, H, ret, failed, actions, I.SMALLEST_SUBNORMAL, ("best_action", "best_sequence"))      # ignored without mean_sequence
    check_select(got, I.select_reference(P, K, ret, failed, actions), ("best_action", "best_sequence"))
    got = run_select(hd, P, K, H, ret, failed, actions, edge)
    assert np.isfinite(got["mean_sequence"]).all()
    check_select(got, I.select_reference(P, K, ret, failed, actions, 1e-300))
