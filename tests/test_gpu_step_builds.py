"""Every build of the env-step kernel (csrc/gl_step_select.hpp: 53 one-lane-per-environment fp32 builds, 28 four-lanes-per-environment
ones) launched through the C ABI at ragged batches -- B = 65 with ld = 80, and B = 1 -- and compared with references that are not
kernels: the oracle's restatement of the scheme for the state, the reference project's reward restated for reward and info, the
observation reference of tests/envlayer_inputs.py.  Cases, inputs and references: tests/step_build_inputs.py (checked on the CPU by
tests/test_step_build_inputs_host.py).  Which build ran is read back with glgym_last_step_build, so that a case cannot pass on another
build's results.  Every buffer is a guarded one with NaN / 0xFF where the test put no data.

Bounds.  State: tests/test_gpu_fuzz.py's metric and bounds (1e-11 fp64, 5e-6 fp32), which were set on the glgym_evalF kernels running
the same integrator; STATE_BOUND below says where a (dtype, scheme) departs from them and why.  A build whose error stands out from
its siblings of the same dtype, scheme and verify mode by more than 4x their median fails test_no_build_stands_out_from_its_siblings.
Applied control: tests/test_gpu_refenv.py's 1e-7 / 1e-15.  Reward and info at the kernel's own state: fp64 1e-6
(test_step_kernel_matches_env_oracle); fp32 4x what the fp32 quad default-parameter build of the same scheme -- the one
tests/test_gpu_refenv.py ties to the reference environment -- shows on the same rows (existing tests saw that spread between fp32 builds'
operation orders: 2e-7 .. 1e-6 in test_two_waves_per_simd_build_matches_one_wave_build).  In fp32 that figure is about 1e-4 in every build:
the reference's revenue comes from the stored fruit dry matter, quantised at 0.03 mg m-2.  So the reward is also compared with the
reference's revenue replaced by the kernel's revenue row (bounded the same way, about 1e-5), and the revenue row with the stored
difference to one spacing of the dtype at x[25] -- a bound from the number format.  x[27], timestep, done and the FAILED bit are
exact.  Siblings -- epilogue builds against the plain build and the unfused sequence, PAIR against the sequential ladder, B = 1 against
row 0 of B = 65 -- are compared bit for bit.

Not reached: the fp64 quad builds have ODE_pipe compiled in and select it at run time; every case runs them on the default ODE (the
same run-time branch of glgym_evalF's fp64 builds is tied to the oracle by tests/test_gpu_evalf_builds.py, the evalF census).  The
one-lane ODE_pipe build runs with all 65 rows refined and is compared with the level of the one-lane rk4 builds of the default ODE
(siblings()).  The fp32 verified rk2 runs measure 3.9e-6 .. 4.0e-6 of the 5e-6 bound in every family alike: little margin.

With GLGYM_STEP_CENSUS=<path> in the environment the measured figures of every case run are written there (profiles/step_build_census.txt
is such a file)."""
import ctypes as C
import os

import numpy as np
import pytest

import envlayer_inputs as E
import step_build_inputs as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return S.stepselect_host(tmp_path_factory.mktemp("stepselecthost"))


U_BOUND = {False: 1e-7, True: 1e-15}
REWARD_BOUND_F64 = 1e-6
REWARD_FACTOR_F32 = 4.0
GAIN_K = 1e-6 / 0.065 * 1.6                  # EUR per mg m-2 of fruit dry matter (rewards.py:173-184 with TomatoEnv.yml's dmfm, fruit_price)
STAND_OUT = 4.0
# (f64, scheme) -> bound on the state error; tests/test_gpu_fuzz.py's unless a line below says otherwise
STATE_BOUND = {(f64, s): (1e-11 if f64 else 5e-6) for f64 in (False, True) for s in S.SCHEMES}

SEED_RESET = 0x9E3779B97F4A7C15
# Launches and measurements are kept for the session, keyed by everything that defines them: a build's plain launch is also the sibling
# of its epilogue builds, the yardstick of the fp32 reward bound and a line of the census, and is made once whichever test asks first.
_runs, _measured = {}, {}


def _vec(values, B, dtype):
    """[B] values in an [LD] vector whose tail is 0xFF."""
    out = np.frombuffer(b"\xff" * (S.LD * np.dtype(dtype).itemsize), dtype=dtype).copy()
    out[:B] = np.asarray(values)[:B]
    return out


def run(c, B, raw=None, nan_row=None, entry=None, ladder=None, bdf=False):
    """One launch of case c's recipe on the first B rows (raw / entry / ladder override the recipe for the sibling launches) -> dict of
    host arrays: every buffer before and after, the build record, return codes.  Cached: a sibling is launched once."""
    raw = c.raw if raw is None else raw
    entry = c.entry if entry is None else entry
    ladder = c.ladder_parallel if ladder is None else ladder
    key = (c.id, B, raw, nan_row, entry, ladder, bdf)
    if key in _runs:
        return _runs[key]
    from gl_gym_amd import _lib as L
    h = S.host_inputs(c, raw)
    hd = E.Handle(c.f64, S.DT, nd=c.nd, params=h["p"])
    lib, T = hd.lib, hd.T
    sch, n_sub, _, _ = S.SCHEMES[c.scheme]
    for rc in (lib.glgym_set_scheme(hd.h, sch), lib.glgym_set_n_sub(hd.h, n_sub), lib.glgym_set_layout(hd.h, c.layout),
               lib.glgym_set_occupancy(hd.h, c.occupancy), lib.glgym_set_ladder_parallel(hd.h, ladder),
               lib.glgym_set_model_variant(hd.h, L.ODE_PIPE if c.pipe else L.ODE), lib.glgym_set_step_integrator(hd.h, 1 if bdf else 0)):
        assert rc == L.OK, hd.error()
    out10 = (C.c_int32 * 10)()
    assert lib.glgym_last_step_build(hd.h, out10) == L.EINVAL                    # no step yet
    x0 = h["x"][:B].copy()
    if nan_row is not None:
        x0[nan_row, 2] = np.nan
    before = dict(x=E.soa(x0, S.LD, T), u=E.soa(h["u_prev"][:B], S.LD, T), weather=np.ascontiguousarray(h["weather"], dtype=T),
                  w_off=_vec(h["w_off"], B, np.int32), timestep=_vec(h["timestep"], B, np.int32),
                  start_day=_vec(h["start_day"], B, np.float32), episode=_vec(h["episode"], B, np.int32),
                  start_rows=h["start_rows"], start_days=h["start_days"])
    if raw:
        before["control"] = E.soa(h["control"][:B], S.LD, T)
    else:
        before["action"] = np.ascontiguousarray(h["action"][:B], dtype=np.float32)
    if c.crop:
        before["crop"] = E.soa(h["crop"][:B], S.LD, T)
    g = {k: E.Guarded(v) for k, v in before.items()}
    g.update(reward=E.Guarded(shape=(S.LD,), dtype=T), info=E.Guarded(shape=(11, S.LD), dtype=T), done=E.Guarded(shape=(S.LD,), dtype=np.uint8),
             flags=E.Guarded(shape=(S.LD,), dtype=np.int32), metrics=E.Guarded(np.zeros((L.METRIC_REPLICAS, L.METRIC_STRIDE), dtype=np.float32)),
             obs=E.Guarded(shape=(S.LD, S.OBS_DIM), dtype=np.float32), term_obs=E.Guarded(shape=(S.LD, S.OBS_DIM), dtype=np.float32),
             obs_again=E.Guarded(shape=(S.LD, S.OBS_DIM), dtype=np.float32))
    ptr = lambda k: g[k].ptr if k in g else None                                  # noqa: E731
    a = L.make_step_args(B, S.LD, ptr("x"), ptr("u"), ptr("action"), ptr("control"), ptr("weather"), S.N_ENV, ptr("w_off"), ptr("timestep"),
                         ptr("crop"), S.N_TERMINAL, ptr("reward"), ptr("info"), ptr("done"), ptr("metrics"), ptr("flags"))

    def obs_args(obs, mask=None, term=None):
        return L.ObsArgs(B, S.LD, ptr("x"), ptr("u"), ptr("weather"), S.N_ENV, ptr("w_off"), ptr("timestep"), ptr("start_day"), S.NP_FORECAST,
                         ptr(obs), mask, term)

    ra = L.ResetArgs(B, S.LD, None, ptr("x"), ptr("u"), ptr("timestep"), ptr("weather"), S.N_ENV, ptr("w_off"), ptr("start_rows"),
                     ptr("start_days"), len(h["start_rows"]), ptr("start_day"), ptr("episode"), SEED_RESET)
    st, fused_out, rcs = hd.stream(), C.c_int32(-1), []
    hd.sync()
    if entry == "step":
        rcs.append(lib.glgym_step(hd.h, C.byref(a), st))
    elif entry == "step_obs":
        oa = obs_args("obs")
        rcs.append(lib.glgym_step_obs(hd.h, C.byref(a), C.byref(oa), st))
    elif entry == "step_obs_reset":
        oa = obs_args("obs", None, ptr("term_obs"))
        rcs.append(lib.glgym_step_obs_reset(hd.h, C.byref(a), C.byref(oa), C.byref(ra), st, C.byref(fused_out)))
    else:
        assert entry == "unfused"                    # glgym_step, glgym_obs, glgym_reset over `done`, masked glgym_obs with term_obs
        oa, om = obs_args("obs"), obs_args("obs", ptr("done"), ptr("term_obs"))
        ra.mask = ptr("done")
        rcs += [lib.glgym_step(hd.h, C.byref(a), st), lib.glgym_obs(hd.h, C.byref(oa), st), lib.glgym_reset(hd.h, C.byref(ra), st),
                lib.glgym_obs(hd.h, C.byref(om), st)]
    try:
        hd.sync()
    except RuntimeError as e:                        # a device fault: nothing more is launched in this session
        pytest.exit(f"device error after {key}: {e}", returncode=3)
    if L.EHIP in rcs:
        pytest.exit(f"HIP error in {key}: {hd.error()}", returncode=3)
    assert all(rc == L.OK for rc in rcs), (rcs, hd.error())
    assert lib.glgym_last_step_build(hd.h, out10) == L.OK, hd.error()
    if entry == "step_obs":                          # glgym_obs on the resulting state, for the epilogue's rows to be compared with
        oa2 = obs_args("obs_again")
        assert lib.glgym_obs(hd.h, C.byref(oa2), st) == L.OK, hd.error()
        hd.sync()
    r = dict(before=before, after={k: v.read() for k, v in g.items()}, build=tuple(out10), fused_out=fused_out.value, B=B, inputs=h,
             n_simd=4 * hd.t.cuda.get_device_properties(0).multi_processor_count, entry=entry, raw=raw)
    hd.close()
    _runs[key] = r
    return r


def live(r, name):
    """[B, ...] view of an output in float64 (integers as they are): SoA buffers transposed."""
    a, B = r["after"][name], r["B"]
    a = a[:, :B].T if a.ndim == 2 and name not in ("obs", "term_obs", "obs_again") else a[:B]
    return a.astype(np.float64) if a.dtype.kind == "f" else a


def same_bits(r1, r2, names, rows=None, rows2=None):
    for n in names:
        a, b = r1["after"][n], r2["after"][n]
        soa = a.ndim == 2 and n not in ("obs", "term_obs", "obs_again")
        pick = lambda v, rr, B: (v[:, :B] if rr is None else v[:, rr]) if soa else (v[:B] if rr is None else v[rr])      # noqa: E731
        assert np.array_equal(E.bits(pick(a, rows, r1["B"])), E.bits(pick(b, rows if rows2 is None else rows2, r2["B"]))), n


OUTPUTS = ("x", "u", "timestep", "reward", "info", "done", "flags")


def check_build(c, r, host, raw):  # noqa: F811
    B = r["B"]
    want = c.build if r["entry"] != "unfused" else c.build[:6] + (0, c.build[7])
    fused = S.FUSED[want[6]]
    assert r["build"] == want + (S.grid(c, B), fused), (c.id, B, r["build"])
    row = np.array([S.select_inputs(c, B, r["n_simd"], raw)], dtype=np.int32)
    if r["entry"] == "unfused":
        row[0, 11:14] = 0
    sel = np.full((1, 11), -7, dtype=np.int32)
    host.stepselect_batch(1, row.ctypes.data, sel.ctypes.data)
    assert sel[0].tolist() == [0, *r["build"]], (c.id, B, sel[0].tolist(), r["build"])
    if r["entry"] == "step_obs_reset":
        assert r["fused_out"] == (1 if fused == 2 else 0)


def check_memory(c, r):
    """Guards were checked by Guarded.read.  Padding columns and the inputs are bit-identical to before; every live output is written."""
    B, before, after = r["B"], r["before"], r["after"]
    resets = r["entry"] in ("step_obs_reset", "unfused")
    for k, v in before.items():
        if k in ("x", "u", "timestep") or (resets and k in ("w_off", "start_day", "episode")):
            pad_b, pad_a = (v[:, B:], after[k][:, B:]) if v.ndim == 2 else (v[B:], after[k][B:])
            assert np.array_equal(E.bits(pad_b), E.bits(pad_a)), ("padding", k)
        else:
            assert np.array_equal(E.bits(v), E.bits(after[k])), ("input written", k)
    for k in ("reward", "done", "flags"):
        kb = E.bits(after[k])
        assert np.all(kb[B:] == np.iinfo(kb.dtype).max), ("written beyond B", k)
        assert not np.any(kb[:B] == np.iinfo(kb.dtype).max), ("live entry not written", k)
    ib = E.bits(after["info"])
    assert np.all(ib[:, B:] == np.iinfo(ib.dtype).max) and not np.any(ib[:, :B] == np.iinfo(ib.dtype).max), "info"
    assert np.all(np.isin(after["done"][:B], (0, 1))) and np.all(after["flags"][:B] >= 0)
    ob = E.bits(after["obs"])
    if r["entry"] == "step":
        assert g_untouched(after["obs"])
    else:
        assert np.all(ob[B:] == 0xFFFFFFFF) and not np.any(ob[:B] == 0xFFFFFFFF), "obs rows"
    tb = E.bits(after["term_obs"])
    if resets:
        done = after["done"][:B].astype(bool)
        assert np.all(tb[B:] == 0xFFFFFFFF) and np.all(tb[:B][~done] == 0xFFFFFFFF) and not np.any(tb[:B][done] == 0xFFFFFFFF), "term_obs rows"
    else:
        assert g_untouched(after["term_obs"])
    m = after["metrics"].astype(np.float64).sum(axis=0)
    assert m[7] == B and m[3] == int(np.sum((after["flags"][:B] & 128) != 0))           # n_env_steps, n_ode_fail


def g_untouched(a):
    return bool(np.all(a.reshape(-1).view(np.uint8) == 0xFF))


def pre_reset_state(c, r):
    """x / u / timestep as the step left them: the launch's own, with the rows an auto-reset has re-initialised since taken from the
    plain (EPI 0) sibling -- with which the launch is compared bit for bit on everything the reset does not touch."""
    x, u, ts = live(r, "x"), live(r, "u"), live(r, "timestep").copy()
    if r["entry"] in ("step_obs_reset", "unfused"):
        sib = run(S.BY_BUILD[c.build[:6] + (0, c.build[7])], r["B"], raw=r["raw"])
        done = live(r, "done").astype(bool)
        x[done], u[done], ts[done] = live(sib, "x")[done], live(sib, "u")[done], live(sib, "timestep")[done]
    return x, u, ts


def measure(c, raw=None):
    """State and reward errors of case c at B = 65 against the references -> dict (cached)."""
    raw = c.raw if raw is None else raw
    if (c.id, raw) in _measured:
        return _measured[(c.id, raw)]
    r = run(c, S.N_ENV, raw=raw)
    h = r["inputs"]
    x, u, ts = pre_reset_state(c, r)
    ref, _, refined, failed = S.state_reference(h["x"], u, h["weather"], h["p"], h["crop"], c.scheme, c.pipe, verify=raw)
    err = S.state_error(x, ref, h["x"])
    rr, ri, span = S.reward_reference(h["x"], x, u, h["p"])
    m = dict(state=float(err.max()), state_row=int(err.argmax()), reward=S.reward_error(live(r, "reward"), live(r, "info"), rr, ri, span),
             revenue=live(r, "info")[:, 1], revenue_ref=ri[:, 1], x25=np.maximum(np.abs(x[:, 25]), np.abs(h["x"][:, 25])),
             ref=ref, failed=failed, x=x, u=u, ts=ts, refined=int((refined > 0).sum()))
    _measured[(c.id, raw)] = m
    return m


def reward_bound(c, raw=None):
    """-> ((bound on |d reward|, on the info metric, on |d reward| with the kernel's own revenue), where they come from)."""
    if c.f64:
        return (REWARD_BOUND_F64,) * 3, "1e-6 (test_step_kernel_matches_env_oracle)"
    yard = S.BY_BUILD[(S.QUAD, 0, 0, 1, 0, S.SCHEMES[c.scheme][0], 0, 1)]
    v = measure(yard)["reward"]
    return tuple(REWARD_FACTOR_F32 * q for q in v), f"4 x {v[0]:.2e} / {v[1]:.2e} / {v[2]:.2e} of {yard.id}"


def siblings(c, raw):
    """The cases of c's dtype and scheme that have a run in this verify mode.  The ODE_pipe build is alone with its right-hand side: it is
    held to the level of the one-lane handle-parameter rk4 builds of the default ODE (the same kernel but for the pipe equation), on its
    own inputs -- all 65 rows refined (tests/test_step_build_inputs_host.py) -- and does not count among their siblings."""
    if c.pipe:
        return [d for d in S.CASES if d.build[0] == S.ONE_LANE and d.scheme == c.scheme and not d.pipe and d.params == c.params and not d.crop]
    return [d for d in S.CASES if d.f64 == c.f64 and d.scheme == c.scheme and not d.pipe and (d.raw == raw or (raw and S.verified_twin(d)))]


def check_against_references(c, r, m, raw):
    B, h = r["B"], r["inputs"]
    T = np.float64 if c.f64 else np.float32
    # control, clock, terminal
    if raw:
        assert np.array_equal(m["u"], h["control"]), "raw controls are applied unclipped, bit for bit"
    else:
        want_u = S.applied_control(h["u_prev"], h["action"], c.f64)
        assert np.max(np.abs(m["u"] - want_u)) <= U_BOUND[c.f64], np.max(np.abs(m["u"] - want_u))
        assert np.all(m["u"][S.CLIP_HIGH_ROW] == 1.0) and np.all(m["u"][S.CLIP_LOW_ROW] == 0.0)
    assert np.array_equal(m["ts"], h["timestep"] + 1)
    assert np.array_equal(live(r, "done"), S.done_reference(h["timestep"])) and live(r, "done").sum() == len(S.DONE_ROWS)
    assert np.array_equal(m["x"][:, 27], S.exact_clock(h["timestep"]).astype(T).astype(np.float64)), "x[27] is exact"
    flags = live(r, "flags")
    assert np.array_equal((flags & 128) != 0, m["failed"]) and not m["failed"].any()
    if raw:
        assert np.all(((flags >> 8) & 7) >= 1), "a verified step makes at least one extra attempt on every row"
    # state
    bound = STATE_BOUND[(c.f64, c.scheme)]
    print(f"step build {c.id}{' verified' if raw else ''}: worst scaled |state - oracle| = {m['state']:.2e} (row {m['state_row']}, bound {bound:.1e}), "
          f"{m['refined']} of {B} rows refined")
    assert m["state"] < bound, (c.id, raw, m["state"], m["state_row"])
    # reward and info at the kernel's own state
    rb, why = reward_bound(c, raw)
    print(f"step build {c.id}{' verified' if raw else ''}: worst |reward - reference| = {m['reward'][0]:.2e} (bound {rb[0]:.2e}), "
          f"info {m['reward'][1]:.2e} (bound {rb[1]:.2e}), reward with the kernel's revenue {m['reward'][2]:.2e} (bound {rb[2]:.2e}): {why}")
    assert all(v <= b for v, b in zip(m["reward"], rb)), (c.id, raw, m["reward"], rb)
    # The revenue row against the stored fruit dry matter: the kernel takes it from its own increment del, and stores x1 = fl(x0 + del),
    # so (x1 - x0) and del differ by at most half a spacing of T at x[25] (a whole one is allowed), times the price per mg; plus the
    # rounding of the product itself (4 eps).  A bound from the number format alone.
    slack = GAIN_K * np.spacing(m["x25"].astype(T)).astype(np.float64) + 4 * np.finfo(T).eps * np.abs(m["revenue_ref"])
    assert np.all(np.abs(m["revenue"] - m["revenue_ref"]) <= slack), float(np.max(np.abs(m["revenue"] - m["revenue_ref"]) / slack))


def check_observations(c, r, m):
    """Epilogue builds: the rows are glgym_obs's on the resulting state bit for bit and lie within the observation bounds of the reference."""
    h, B = r["inputs"], r["B"]
    if r["entry"] == "step_obs":
        same = np.array_equal(E.bits(r["after"]["obs"][:B]), E.bits(r["after"]["obs_again"][:B]))
        assert same, "the epilogue's rows differ from glgym_obs on the same state"
        x, u, ts, w_off, sday = live(r, "x"), live(r, "u"), live(r, "timestep"), h["w_off"][:B], h["start_day"][:B]
    else:
        x, u, ts, w_off, sday = live(r, "x"), live(r, "u"), live(r, "timestep"), live(r, "w_off"), r["after"]["start_day"][:B]
        done = live(r, "done").astype(bool)
        term = E.obs_reference(m["x"][:B], m["u"][:B], h["weather"], h["w_off"][:B], m["ts"][:B], h["start_day"][:B], S.NP_FORECAST,
                               E.MODULE_LISTS["default"], S.DT)
        np.testing.assert_allclose(live(r, "term_obs")[done], term[done], rtol=E.OBS_RTOL, atol=E.OBS_ATOL)
        assert np.all(ts[done] == 0) and np.all(u[done] == 0)
    want = E.obs_reference(x, u, h["weather"], w_off, ts, sday, S.NP_FORECAST, E.MODULE_LISTS["default"], S.DT)
    np.testing.assert_allclose(live(r, "obs"), want, rtol=E.OBS_RTOL, atol=E.OBS_ATOL)


def check_siblings(c, r, host):  # noqa: F811
    B, epi = r["B"], c.build[6]
    if epi:
        plain = run(S.BY_BUILD[c.build[:6] + (0, c.build[7])], B)
        done = r["after"]["done"][:B].astype(bool)
        rows = None if epi == 8 else np.nonzero(~done)[0]
        same_bits(r, plain, ("x", "u", "timestep"), rows)
        same_bits(r, plain, ("reward", "info", "done", "flags"))
    if epi == 24:
        un = run(c, B, entry="unfused")
        check_build(c, un, host, c.raw)
        check_memory(c, un)
        same_bits(r, un, OUTPUTS + ("obs", "w_off", "start_day", "episode"))
        same_bits(r, un, ("term_obs",), np.nonzero(done)[0])
        assert np.array_equal(r["after"]["episode"][:B], r["before"]["episode"][:B] + done)        # the reset did start episodes
    if c.build[0] == S.QUAD_PAIR:
        seq = run(c, B, ladder=0)
        assert seq["build"][:8] == (S.QUAD,) + c.build[1:]
        same_bits(r, seq, OUTPUTS)


def check_failed_row(c, r):
    """A second launch with a NaN in one row's air temperature: that row fails (done, FAILED, state unchanged), no other row notices."""
    B = r["B"]
    row = S.NAN_ROW if B > 1 else 0
    n = run(c, B, nan_row=row)
    assert n["after"]["done"][row] == 1 and n["after"]["flags"][row] & 128
    if c.entry == "step_obs_reset":
        assert n["after"]["timestep"][row] == 0 and n["after"]["episode"][row] == n["before"]["episode"][row] + 1      # failed, then reset
    else:
        assert np.array_equal(E.bits(n["after"]["x"][:, row]), E.bits(n["before"]["x"][:, row])), "a failed row's state must stay as it was"
    others = np.array([i for i in range(B) if i != row], dtype=int)
    if len(others):
        same_bits(n, r, OUTPUTS + (("obs",) if c.entry != "step" else ()) + (("term_obs", "w_off", "start_day", "episode") if c.entry == "step_obs_reset" else ()),
                  others)


@pytest.mark.parametrize("c", S.CASES, ids=[c.id for c in S.CASES])
def test_build(c, host):  # noqa: F811
    full = None
    for B in S.BATCHES:
        r = run(c, B)
        check_build(c, r, host, c.raw)
        check_memory(c, r)
        if B == S.N_ENV:
            full = r
            m = measure(c)
            check_against_references(c, r, m, c.raw)
            if c.entry != "step":
                check_observations(c, r, m)
        else:                                       # a row does not depend on the lanes around it
            same_bits(r, full, OUTPUTS + (("obs",) if c.entry != "step" else ()), np.array([0]), np.array([0]))
        check_siblings(c, r, host)
        check_failed_row(c, r)
    if S.verified_twin(c):                          # once with raw controls: a verified step on the sequential ladder
        v = run(c, S.N_ENV, raw=True)
        check_build(c, v, host, True)
        check_memory(c, v)
        check_against_references(c, v, measure(c, raw=True), True)


def test_bdf_env_step_records_no_build():
    """glgym_set_step_integrator(BDF): none of the 81 builds runs; the record says family -1."""
    c = S.BY_BUILD[(S.QUAD, 1, 0, 0, 1, S.LS5, 0, 1)]
    r = run(c, 1, bdf=True)
    assert r["build"] == (-1, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert r["after"]["flags"][0] & 2048 and r["after"]["timestep"][0] == r["before"]["timestep"][0] + 1


def test_no_build_stands_out_from_its_siblings():
    """The census: every case's figures (measured here for whatever the session has not run yet), each build's state error against the
    median of its siblings of the same dtype, scheme and verify mode."""
    lines, bad = [], []
    for c in S.CASES:
        for raw in ((c.raw, True) if S.verified_twin(c) else (c.raw,)):
            m = measure(c, raw)
            sib = [measure(d, raw)["state"] for d in siblings(c, raw) if d.id != c.id]
            med = float(np.median(sib)) if sib else float("nan")
            rb, why = reward_bound(c, raw)
            lines.append(f"{c.id:34s} {'verified' if raw else 'plain':8s} state {m['state']:.2e} (row {m['state_row']:2d}; siblings' median {med:.2e}; "
                         f"bound {STATE_BOUND[(c.f64, c.scheme)]:.1e})  reward {m['reward'][0]:.2e} (bound {rb[0]:.2e})  info {m['reward'][1]:.2e} (bound {rb[1]:.2e})  "
                         f"reward with own revenue {m['reward'][2]:.2e} (bound {rb[2]:.2e}) = {why}  "
                         f"refined rows {m['refined']}")
            if sib and m["state"] > STAND_OUT * med:
                bad.append(lines[-1])
    print("\n".join(lines))
    path = os.environ.get("GLGYM_STEP_CENSUS")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert not bad, "\n".join(bad)
