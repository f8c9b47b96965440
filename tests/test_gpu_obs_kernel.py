"""glgym_obs (obs_kernel) against envlayer_inputs.obs_reference, called through ctypes on caller-owned buffers: ragged batches in which
every environment has its own state, window and clocks, every forecast length up to the kernel's limit, six module lists, the three row
clamps, clocks on whole revolutions, a 300 s handle, masked mode with terminal observations, the grid-stride loop (in a child process
started with GLGYM_OBS_BLOCKS=2) and the refusals.  Pass-through columns are compared bit for bit, computed columns at the bound of
tests/test_gpu_refenv.py; all buffers carry guards (envlayer_inputs.Guarded)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":                    # the grid-stride child: no conftest here
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "greenlight-gym2_amd"), os.path.join(_root, "tests")]

import envlayer_inputs as E

pytestmark = pytest.mark.gpu

PAD = 5                                       # ld = B + PAD
FIELDS = ("B", "ld", "x", "u", "weather", "weather_rows", "w_off", "timestep", "start_day", "Np", "obs", "mask", "term_obs")


@pytest.fixture(scope="module")
def handles():
    hs = {(False, 900.0): E.Handle(False), (True, 900.0): E.Handle(True), (False, 300.0): E.Handle(False, 300.0)}
    yield hs
    for h in hs.values():
        h.close()


def set_modules(hd, mods, Np):
    arr = (C.c_int32 * len(mods))(*mods)
    assert hd.lib.glgym_set_obs_modules(hd.h, arr, len(mods)) == 0
    dim = hd.lib.glgym_obs_dim(hd.h, Np)
    assert dim == E.obs_layout(mods, Np)[1]
    return dim


def run_obs(hd, c, Np, mods, mask=None, prev=None, with_term=False, override=None, expect=0):
    """One glgym_obs call on the inputs of case `c` -> (obs [B, dim], term_obs [B, dim] or None), guards checked.  `prev`: what the
    observation buffer holds before the call (0xFF bytes otherwise)."""
    B = len(c["timestep"])
    ld, dim = B + PAD, set_modules(hd, mods, Np)
    src = dict(x=E.soa(c["x"], ld, hd.T), u=E.soa(c["u"], ld, hd.T), weather=np.asarray(c["weather"], dtype=hd.T),
               w_off=c["w_off"], timestep=c["timestep"], start_day=c["start_day"])
    ins = {k: E.Guarded(v) for k, v in src.items()}
    obs = E.Guarded(prev) if prev is not None else E.Guarded(shape=(B, dim), dtype=np.float32)
    term = E.Guarded(shape=(B, dim), dtype=np.float32) if with_term else None
    mk = E.Guarded(mask) if mask is not None else None
    val = dict(B=B, ld=ld, weather_rows=c["weather"].shape[0], Np=Np, obs=obs.ptr, mask=mk.ptr if mk else None,
               term_obs=term.ptr if term else None, **{k: g.ptr for k, g in ins.items()})
    val.update(override or {})
    a = hd.L.ObsArgs(*[val[f] for f in FIELDS])
    hd.sync()
    rc = hd.lib.glgym_obs(hd.h, C.byref(a), hd.stream())
    hd.sync()
    assert rc == expect, (rc, hd.error())
    for k, g in ins.items():                                                     # the inputs are read-only
        assert np.array_equal(E.bits(g.read()), E.bits(np.ascontiguousarray(src[k]))), k
    return obs.read(), (term.read() if term else None)


def reference(hd, c, Np, mods):
    ref = E.obs_reference(E.rounded(c["x"], hd.f64), E.rounded(c["u"], hd.f64), E.rounded(c["weather"], hd.f64), c["w_off"],
                          c["timestep"], c["start_day"], Np, mods, hd.dt)
    E.assert_rows_distinct(ref)
    return ref


def check_rows(got, ref, Np, mods, rows=slice(None), what=""):
    """Rows `rows` of the block against the reference: copies bit for bit, computed columns at the project's bound."""
    got, ref = got[rows], ref[rows]
    assert not np.isnan(got).any(), f"{what}: a NaN (padding or a row nobody wrote) reached the output"
    pt = E.obs_passthrough(mods, Np)
    bad = E.bits(got[:, pt]) != E.bits(ref[:, pt].astype(np.float32))
    assert not bad.any(), f"{what}: {bad.sum()} pass-through entries differ from float32(input), first in rows {np.nonzero(bad.any(axis=1))[0][:8]}"
    if (~pt).any():
        err = np.abs(got[:, ~pt] - ref[:, ~pt]) / (E.OBS_ATOL + E.OBS_RTOL * np.abs(ref[:, ~pt]))
        print(f"{what}: computed columns at {err.max():.3g} of the tolerance")
        np.testing.assert_allclose(got[:, ~pt], ref[:, ~pt], rtol=E.OBS_RTOL, atol=E.OBS_ATOL, err_msg=what)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("B", E.OBS_BATCHES)
def test_ragged_batches_every_env_its_own_inputs(handles, B, f64):
    hd, Np, mods = handles[(f64, 900.0)], 3, E.MODULE_LISTS["default"]
    c = E.obs_case(B, Np)
    got, _ = run_obs(hd, c, Np, mods)
    check_rows(got, reference(hd, c, Np, mods), Np, mods, what=f"B={B}")


NP_LISTS = [(Np, name) for Np in E.OBS_NP for name in E.MODULE_LISTS if not (Np == 0 and name == "forecast_only")]


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("Np,name", NP_LISTS, ids=[f"Np{n}-{m}" for n, m in NP_LISTS])
def test_forecast_lengths_and_module_lists(handles, Np, name, f64):
    """B = 33: two full strips and a ragged one, with every edge of envlayer_inputs.OBS_KINDS in the first strip."""
    hd, mods = handles[(f64, 900.0)], E.MODULE_LISTS[name]
    kinds = tuple(k for k in E.OBS_KINDS if not (name == "forecast_only" and k == "beyond"))
    c = E.obs_case(33, Np, kinds=kinds)
    got, _ = run_obs(hd, c, Np, mods)
    check_rows(got, reference(hd, c, Np, mods), Np, mods, what=f"Np={Np} {name}")


def test_handle_with_300_s_steps(handles):
    hd, Np, mods = handles[(False, 300.0)], 3, E.MODULE_LISTS["default"]
    c = E.obs_case(33, Np, dt=300.0)
    assert c["timestep"][list(c["kind"]).index("day_whole")] == 288
    got, _ = run_obs(hd, c, Np, mods)
    ref = reference(hd, c, Np, mods)
    check_rows(got, ref, Np, mods, what="dt=300")
    ref900 = E.obs_reference(E.rounded(c["x"], False), E.rounded(c["u"], False), E.rounded(c["weather"], False), c["w_off"],
                             c["timestep"], c["start_day"], Np, mods, 900.0)
    assert np.abs(ref900 - ref).max() > 0.1                                      # the clocks really depend on the handle's dt


def previous_rows(B, dim):
    """What the observation buffer holds before a masked call: finite, no two entries alike."""
    return (1000.0 + 0.5 * np.arange(B * dim, dtype=np.float32)).reshape(B, dim)


def check_masked(got, term, prev, ref, m, Np, mods, what):
    on = m.astype(bool)
    if on.any():
        check_rows(got, ref, Np, mods, rows=on, what=what)
    assert np.array_equal(E.bits(got[~on]), E.bits(prev[~on])), f"{what}: an unmasked observation row was written"
    if term is not None:
        assert np.array_equal(E.bits(term[on]), E.bits(prev[on])), f"{what}: term_obs is not the previous content of the masked rows"
        assert np.all(E.bits(term[~on]) == 0xFFFFFFFF), f"{what}: an unmasked term_obs row was written"


MASKED = [("zeros", True), ("ones", True), ("ones", False), ("corners", True), ("random", True)]


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,with_term", MASKED, ids=[f"{k}-{'term' if t else 'noterm'}" for k, t in MASKED])
def test_masked_mode(handles, kind, with_term, f64):
    hd, B, Np, mods = handles[(f64, 900.0)], 33, 3, E.MODULE_LISTS["permuted"]
    c, m = E.obs_case(B, Np), E.mask_of(kind, B)
    prev = previous_rows(B, E.obs_layout(mods, Np)[1])
    got, term = run_obs(hd, c, Np, mods, mask=m, prev=prev, with_term=with_term)
    check_masked(got, term, prev, reference(hd, c, Np, mods), m, Np, mods, f"mask {kind}")
    if kind == "zeros":
        assert np.all(E.bits(term) == 0xFFFFFFFF)


def grid_stride_child():
    """B = 100 = seven strips on the two blocks GLGYM_OBS_BLOCKS=2 allows: full mode, and masked mode with one whole strip unmasked."""
    assert os.environ.get("GLGYM_OBS_BLOCKS") == "2"
    hd, B, Np, mods = E.Handle(False), 100, 3, E.MODULE_LISTS["default"]
    c = E.obs_case(B, Np)
    ref = reference(hd, c, Np, mods)
    got, _ = run_obs(hd, c, Np, mods)
    check_rows(got, ref, Np, mods, what="grid-stride, full mode")
    m, prev = E.mask_of("strip_off", B), previous_rows(B, E.obs_layout(mods, Np)[1])
    got, term = run_obs(hd, c, Np, mods, mask=m, prev=prev, with_term=True)
    check_masked(got, term, prev, ref, m, Np, mods, "grid-stride, masked mode")
    hd.close()
    print("grid-stride child: ok")


def test_grid_stride_loop_in_a_child_process():
    """GLGYM_OBS_BLOCKS is read once per process: a fresh child runs this file's grid_stride_child with the cap at two blocks."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, GLGYM_OBS_BLOCKS="2"), capture_output=True,
                       text=True, timeout=180)
    assert r.returncode == 0 and "grid-stride child: ok" in r.stdout, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])


NULLS = ("x", "u", "weather", "w_off", "timestep", "start_day", "obs")
REFUSALS = [("weather_rows", 0), ("weather_rows", -1), ("ld", 32), ("B", 0), ("Np", 129), ("Np", -1)] + [(f, None) for f in NULLS]


@pytest.mark.parametrize("field,value", REFUSALS, ids=[f"{f}={v}" for f, v in REFUSALS])
def test_refusals_write_nothing(handles, field, value):
    hd, B, Np, mods = handles[(False, 900.0)], 33, 3, E.MODULE_LISTS["default"]
    c = E.obs_case(B, Np)
    got, term = run_obs(hd, c, Np, mods, mask=None, with_term=True, override={field: value}, expect=hd.L.EINVAL)
    assert np.all(E.bits(got) == 0xFFFFFFFF) and np.all(E.bits(term) == 0xFFFFFFFF)
    assert "glgym_obs" in hd.error()
    if field == "weather_rows":
        assert "weather_rows" in hd.error()


def test_fused_entry_points_refuse_an_empty_weather_table(handles):
    """glgym_step_obs and glgym_step_obs_reset check the observation and reset blocks before anything is launched."""
    hd, L, B = handles[(False, 900.0)], handles[(False, 900.0)].L, 16
    buf = E.Guarded(shape=(64 * B,), dtype=np.float32)
    p = buf.ptr
    for rows_obs, rows_reset in ((0, 5), (-1, 5), (5, 0)):
        oa = L.ObsArgs(B, B, p, p, p, rows_obs, p, p, p, 0, p, None, None)
        ra = L.ResetArgs(B, B, None, p, p, p, p, rows_reset, p, None, None, 0, None, None, 0)
        sa = L.make_step_args(B, B)
        if rows_reset > 0:
            assert hd.lib.glgym_step_obs(hd.h, C.byref(sa), C.byref(oa), None) == L.EINVAL
            assert "weather_rows" in hd.error() and "observation" in hd.error()
        assert hd.lib.glgym_step_obs_reset(hd.h, C.byref(sa), C.byref(oa), C.byref(ra), None, None) == L.EINVAL
        assert "weather_rows" in hd.error() and "glgym_step_obs_reset" in hd.error()
    hd.sync()
    assert buf.untouched()


if __name__ == "__main__":
    grid_stride_child()
