"""Host checks of the inputs that tests/test_gpu_vecnorm.py and tests/test_gpu_weather.py feed the kernels
(tests/ancillary_inputs.py): the references are themselves accurate to a tenth of the tolerances the kernels are held to, and
every weather case is one the host loader accepts -- so a GPU failure on these inputs is the kernel's."""
import numpy as np
import pytest

import ancillary_inputs as A
from oracle.vecnorm_oracle import RunningMeanStd


def _longdouble_update(mean, var, count, obs):
    """RunningMeanStd.update in np.longdouble with two-pass batch moments."""
    ld = np.longdouble
    bm, bv = A.two_pass_moments(obs)
    n = ld(obs.shape[0])
    mean, var, count = np.asarray(mean, dtype=ld), np.asarray(var, dtype=ld), ld(count)
    delta, tot = bm - mean, count + n
    m2 = var * count + bv * n + np.square(delta) * count * n / tot
    return mean + delta * n / tot, m2 / tot, tot


def test_ill_conditioned_columns_are_within_the_oracles_own_precision():
    """Every ill-conditioned case, cold and warm: the fp64 oracle (np.mean / np.var, SB3's update) against a longdouble two-pass
    computation, as a fraction of the tolerance the kernel is held to, and at most a tenth of it.  Seen: mean 1.4e-7, variance
    7.2e-7, rows 1.7e-7 of their tolerances (the printout has each case)."""
    worst = {"mean": 0.0, "var": 0.0, "obs": 0.0}
    eps = 1e-8
    for B in A.ILL_BATCHES:
        obs = A.ill_batch(B)
        assert obs.dtype == np.float32 and obs.shape == (B, len(A.ILL_COLUMNS))
        assert np.all(obs[:, A.ILL_CONST_COL] == obs[0, A.ILL_CONST_COL])
        for warm in (False, True):
            rms = RunningMeanStd(shape=(obs.shape[1],))
            if warm:
                rms.mean, rms.var, rms.count = A.ill_warm_stats(obs)
            m0, v0, c0 = rms.mean.copy(), rms.var.copy(), rms.count
            rms.update(obs.astype(np.float64))
            m, v, c = _longdouble_update(m0, v0, c0, obs)
            assert abs(float(c) - rms.count) < 0.1 * A.VN_COUNT_ATOL
            rows = (obs.astype(np.float64) - rms.mean) / np.sqrt(rms.var + eps)
            rows_ld = (obs.astype(np.longdouble) - m) / np.sqrt(v + np.longdouble(eps))
            ratios = {"mean": A.tol_ratio(rms.mean, m, *A.VN_TOL["mean"]), "var": A.tol_ratio(rms.var, v, *A.VN_TOL["var"]),
                      "obs": A.tol_ratio(np.clip(rows, -10, 10), np.clip(rows_ld, -10, 10), *A.VN_TOL["obs"])}
            print(f"B={B} warm={warm}: oracle vs longdouble two-pass, fraction of tolerance: " +
                  ", ".join(f"{k} {r:.2e}" for k, r in ratios.items()))
            for k, r in ratios.items():
                worst[k] = max(worst[k], r)
            if warm:                                              # the constant column keeps a zero variance
                assert rms.var[A.ILL_CONST_COL] <= A.VN_TOL["var"][1]
    print("largest fraction of tolerance:", ", ".join(f"{k} {r:.2e}" for k, r in worst.items()))
    assert all(r <= 0.1 for r in worst.values()), worst


def test_vecnorm_batches_reach_the_clip_and_the_eval_rows_sit_exactly_on_it():
    from oracle.vecnorm_oracle import VecNormalizeOracle
    for B, dim in A.VN_SHAPES:
        if B < 7 or B * dim > 600000:
            continue
        clip = A.vn_clip_obs(B)
        orc = VecNormalizeOracle(B, dim, clip_obs=clip)
        hit_hi = hit_lo = False
        for call in range(A.VN_N_CALLS):
            obs, rew, done = A.vn_batch(B, dim, call)
            assert obs.dtype == np.float32 and np.all(np.isfinite(obs)) and done[B - 1] and done[0]
            o, _ = orc.step(obs.astype(np.float64), rew, done)
            hit_hi |= bool((o == np.float32(clip)).any())
            hit_lo |= bool((o == np.float32(-clip)).any())
        assert hit_hi and hit_lo, (B, dim)
        sc = np.abs(obs).max(axis=0)
        assert dim < 3 or sc.max() / sc.min() > 50.0, (B, dim)      # columns of very different scales
    eps = 1e-8
    for B, dim in A.VN_MODE_SHAPES:
        mean, var, _ = A.vn_eval_stats(dim, eps)
        assert np.all(var + eps == 4.0)
        clip = 10.0
        obs = A.vn_eval_batch(B, dim, clip)
        z = (obs.astype(np.float64) - mean) / np.sqrt(var + eps)
        assert np.all(z[0] == clip) and np.all(z[1] == -clip)       # exactly on the clip
        assert np.all(z[2] > clip) and np.all(z[3] < clip) and np.all(z[4] > -clip) and np.all(z[5] < -clip)


@pytest.mark.parametrize("dt", A.W_INTERVALS)
def test_weather_cases_are_ones_the_host_loader_accepts(dt):
    cases = A.weather_cases(dt)
    assert {c["rad"] for c in cases} == set(A.W_RADIATION) and {c["start"] for c in cases} == set(A.W_STARTS)
    assert {c["jitter"] for c in cases} == {False, True}
    seen_stress = set()
    for c in cases:
        cols = A.weather_raw(c)
        time = cols[0]
        assert len(time) == c["n"] and np.all(np.diff(time) > 0)
        n_tr, ratio = A.ramp_length(time)
        assert n_tr == int(3600 / dt) and (n_tr == 1 or n_tr % 2 == 0), A.case_id(c)
        if c["jitter"]:                          # otherwise the ramp length is a coin toss between host and device
            assert abs(ratio - round(ratio)) > 1e-9, A.case_id(c)
            assert np.abs(np.diff(time) - dt).max() > 0.01 * dt
        else:
            assert np.all(np.diff(time) == dt)
        assert -30.0 <= cols[2].min() and cols[2].max() <= 45.0
        seen_stress.update(c["stress"])
        knots = A.weather_knots(*cols)           # runs without raising
        assert np.all(np.isfinite(knots))
        for n_out in A.n_out_list(c["n"]):
            out, raw0 = A.weather_host(time, knots, n_out)
            assert out.shape == (n_out, 10) and np.all(np.isfinite(out))
            # the iGlob clean-up threshold is not straddled: no interpolated value sits within a decade of 1e-10 (the
            # rounding residue of a zero is ~1e-13)
            assert not np.any((raw0 > 1e-11) & (raw0 < 1e-9)), (A.case_id(c), n_out)
        if not c["jitter"]:                      # n_out = n_raw on a uniform grid evaluates AT the knots
            assert np.array_equal(np.linspace(time[0], time[-1], c["n"]), time)
            out, raw0 = A.weather_host(time, knots, c["n"])
            out[:, 0] = raw0                     # ... where scipy's cubic of interval k returns y[k] itself
            assert np.array_equal(out[:-1], knots[:-1]), A.case_id(c)
    assert seen_stress == set(A.W_STRESS)
    all_n = {c["n"] for d in A.W_INTERVALS for c in A.weather_cases(d)}
    assert all_n == set(A.W_N_RAW)


def test_weather_radiation_patterns_do_what_their_names_say():
    """Ramps are written where the case means them to be and nowhere else: 'edges' leaves every flag at 0 / 1, 'dropouts' and
    'pulses' produce ramp values, 'night' and 'always' are constant."""
    for dt in A.W_INTERVALS[:4]:                 # at 3 600 s the ramp has length one: nothing to see
        for c in A.weather_cases(dt):
            cols = A.weather_raw(c)
            knots = A.weather_knots(*cols)
            flag = knots[:, 8]
            frac = bool(np.any((flag > 0) & (flag < 1)))
            if c["rad"] == "night":
                assert np.all(flag == 0) and np.all(knots[:, 7] == 0)
            elif c["rad"] == "always":
                assert np.all(flag == 1)
            elif c["rad"] == "edges":
                assert not frac and flag[0] == 0 and flag[-1] == 0 and flag[len(flag) // 2] == 1
            elif c["rad"] == "dropouts" and c["n"] >= 255 and dt <= 900:
                assert frac
