"""glgym_plan_scenario, glgym_plan_aggregate and glgym_plan_weather through the C ABI on guarded buffers, bit for bit against
test_plan_scen_host.np_scen_crop / py_aggregate and test_plan_wscen_host.np_wscen.  The three lane-per-child kernels use 256-thread
blocks: 255, 256, 257, 513 and 512 children (S = 256 among them), 248, 256, 264, 520 and 2048 window lanes, so that the second block
and a ragged last block run on their own.  scenario: h_step 0, 1 and 65 535, held and fresh draws, scale 0, with and without the action
pair.  aggregate: tail sizes strictly inside 2..S, one and seventy candidates, S equal returns, zeros of either sign.  weather: rows of
10, 14 and 16 columns, parents whose first steps lie in front of the table (the lower clamp), over its end, behind it, and one with a
large negative timestep; a table of one row; without child offsets.  Both handle dtypes where the kernel is templated."""
import numpy as np
import pytest

import plan_inputs as I

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles():
    hs = {(f64, nd): I.Handle(f64, nd=nd) for f64 in (False, True) for nd in (10, 14, 16)}
    yield hs
    for h in hs.values():
        h.close()


# ---- scenario -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("P,K,S", I.SCEN_SHAPES)
def test_scenario_blocks_of_children(handles, P, K, S, f64):
    hd = handles[(f64, 10)]
    n, ld, L = P * K * S, P * K * S + I.PAD, hd.L
    acts = I.scenario_actions(P, K)
    for h, hold, scale, pair, base in I.SCEN_CALLS:
        ins = I.guarded(dict(actions_in=acts)) if pair else {}
        word, word_ptr, add = I.draw_word(base)
        crop = I.Guarded(shape=(I.NCROP, ld), dtype=hd.T)
        out = I.Guarded(shape=(n, I.NU), dtype=np.float32)
        a = L.make_plan_args(L.PlanScenarioArgs, P, K, S, ld, h, hold, scale, I.SEED, I.DRAW, word_ptr, crop.ptr,
                             ins["actions_in"].ptr if pair else None, out.ptr if pair else None)
        I.launch(hd, "glgym_plan_scenario", a)
        assert word is None or word.read()[0] == I.BASE
        I.assert_only_read(ins, dict(actions_in=acts))
        exp = I.scenario_reference(P, K, S, h, hold, scale, I.SEED, I.DRAW + add)
        got = crop.read()
        wrong = I.bits(got[:, :n]) != I.bits(exp.astype(hd.T))
        assert not wrong.any(), f"(h, hold, scale) = {(h, hold, scale)}: {wrong.sum()} entries differ, first children {np.nonzero(wrong.any(axis=0))[0][:6]}"
        assert I.untouched_past(got, n), "a padding column of the crop block was written"
        if pair:                                                                # row c = the candidate's row c // S
            assert np.array_equal(I.bits(out.read()), I.bits(np.repeat(acts, S, axis=0)))
        else:
            assert out.untouched()


# ---- aggregate ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("J,S,m,kind", I.AGG_CASES)
def test_aggregate_tails_and_candidate_counts(handles, J, S, m, kind):
    hd = handles[(False, 10)]
    ret, failed, viol, n_steps, ld = I.aggregate_edge_case(J, S, m, kind)
    src = dict(ret=ret, failed=failed, viol=viol, n_steps=n_steps)
    ldc, L = J + I.PAD, hd.L
    e_rc, e_fc, e_vc, e_sc = I.py_aggregate(J, S, m, ret, failed, viol, n_steps)
    for optional in (True, False):
        ins = I.guarded(src)
        rc, fc = I.Guarded(shape=(J,), dtype=np.float64), I.Guarded(shape=(J,), dtype=np.uint8)
        vc, sc = I.Guarded(shape=(3, ldc), dtype=np.float64), I.Guarded(shape=(J,), dtype=np.int32)
        a = L.make_plan_args(L.PlanAggregateArgs, J, S, m, ld, ldc, ins["ret"].ptr, ins["failed"].ptr, ins["viol"].ptr if optional else None,
                             ins["n_steps"].ptr if optional else None, rc.ptr, fc.ptr, vc.ptr if optional else None, sc.ptr if optional else None)
        I.launch(hd, "glgym_plan_aggregate", a)
        I.assert_only_read(ins, src)
        assert I.same_f64(rc.read(), e_rc), (rc.read(), e_rc)
        assert np.array_equal(fc.read(), e_fc)
        if optional:
            got = vc.read()
            assert I.same_f64(got[:, :J], e_vc) and I.untouched_past(got, J) and np.array_equal(sc.read(), e_sc)
        else:
            assert vc.untouched() and sc.untouched()
    if kind == "zeros":                                                         # -0.0 and +0.0 tie: the sum in index order of the tied slots
        assert e_rc[0] == 0.0


# ---- weather windows ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("P,S,H,K,nd,rows,first", I.WEATHER_CASES)
def test_weather_window_lanes(handles, P, S, H, K, nd, rows, first, f64):
    hd = handles[(f64, nd)]
    weather = I.table(hd.T, rows=rows, nd=nd)
    w_off, ts, kinds = I.weather_parents(P, H, rows, first)
    src = dict(weather=weather, w_off_parent=w_off, timestep_parent=ts)
    n, n_child, L = P * S * H, P * K * S, hd.L
    for base, offsets in ((True, True), (False, False)):
        ins = I.guarded(src)
        word, word_ptr, add = I.draw_word(base)
        win, child = I.Guarded(shape=(n, nd), dtype=hd.T), I.Guarded(shape=(n_child,), dtype=np.int32)
        a = L.make_plan_args(L.PlanWeatherArgs, P, K, S, H, rows, ins["weather"].ptr, ins["w_off_parent"].ptr, ins["timestep_parent"].ptr,
                             I.sigma_array(), I.PHI, I.SEED, I.DRAW, word_ptr, win.ptr, child.ptr if offsets else None)
        I.launch(hd, "glgym_plan_weather", a)
        assert word is None or word.read()[0] == I.BASE
        I.assert_only_read(ins, src)
        exp, exp_child = I.weather_reference(P, K, S, H, weather, w_off, ts, I.PHI, I.SEED, I.DRAW + add)
        got = win.read()
        wrong = I.bits(got) != I.bits(exp)
        assert not wrong.any(), f"{wrong.sum()} window entries differ, first (row, column) = {np.argwhere(wrong)[:6].tolist()}; parents {kinds}"
        if offsets:
            assert np.array_equal(child.read(), exp_child)
        else:
            assert child.untouched()
    assert P == 1 or "negative" in kinds                                        # w_off + timestep + h < 0 is really there
