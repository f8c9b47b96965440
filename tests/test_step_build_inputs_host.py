"""CPU checks of the step-kernel build census's table, inputs and references (tests/step_build_inputs.py): the table is the build list of
csrc/gl_step_select.hpp, every recipe selects its build, the oracle integrates every row in every mode the census uses, and the rows
are what the census needs them to be (distinct, some refined and some not, `done` rows, clipping rows)."""
import numpy as np
import pytest

import envlayer_inputs as E
import step_build_inputs as S


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return S.stepselect_host(tmp_path_factory.mktemp("stepselecthost"))


def test_the_table_is_the_build_list(host):
    n = host.stepselect_builds(None, 0)
    listed = np.zeros((n, 8), dtype=np.int32)
    assert host.stepselect_builds(listed.ctypes.data, n) == n
    assert len(S.CASES) == 81 and len({c.build for c in S.CASES}) == 81 and len({c.id for c in S.CASES}) == 81
    assert {c.build for c in S.CASES} == {tuple(r) for r in listed.tolist()}
    assert sum(c.build[0] == S.ONE_LANE for c in S.CASES) == 53
    assert all(c.scheme == "rk4" for c in S.CASES if c.pipe)
    assert S.BY_BUILD[(0, 0, 1, 1, 0, S.RK3, 8, 1)].id == "one-f32-crop-def-rk3-epi8-occ1"


@pytest.mark.parametrize("n_simd", [1024, 256])
def test_every_recipe_selects_its_build(host, n_simd):
    runs = [(c, B, raw) for c in S.CASES for B in S.BATCHES for raw in ((c.raw, True) if S.verified_twin(c) else (c.raw,))]
    rows = np.array([S.select_inputs(c, B, n_simd, raw) for c, B, raw in runs], dtype=np.int32)
    out = np.full((len(rows), 11), -7, dtype=np.int32)
    host.stepselect_batch(len(rows), rows.ctypes.data, out.ctypes.data)
    for (c, B, raw), got in zip(runs, out.tolist()):
        assert got == [0, *c.build, S.grid(c, B), S.FUSED[c.build[6]]], (c.id, B, raw, got)
    assert S.grid(S.BY_BUILD[(0, 0, 0, 1, 0, S.LS5, 0, 1)], 65) == 2           # a full wavefront and one with a single live lane
    assert S.grid(S.BY_BUILD[(1, 0, 0, 1, 0, S.LS5, 0, 1)], 65) == 5           # 260 lanes
    assert S.grid(S.BY_BUILD[(2, 0, 0, 1, 0, S.LS5, 0, 1)], 65) == 9           # 520 lanes


def test_rows():
    b = S.base()
    E.assert_rows_distinct(b["X"][:, :27])
    E.assert_rows_distinct(np.float32(b["X"][:, :27]))                       # as an fp32 handle stores them, too
    E.assert_rows_distinct(np.concatenate([b["U"], b["D"]], axis=1))           # (the calm tuples share weather rows among themselves)
    E.assert_rows_distinct(b["action"])
    assert len(set(b["timestep"].tolist())) >= S.N_ENV - 2 and np.array_equal(b["w_off"] + b["timestep"], np.arange(S.N_ENV))
    done = S.done_reference(b["timestep"])
    assert sorted(np.nonzero(done)[0].tolist()) == sorted(S.DONE_ROWS) and done[:64].sum() == 3 and done[64] == 1 and done[0] == 0
    assert not done[S.NAN_ROW]
    assert len(np.unique(b["CROP"], axis=0)) >= 10                             # the noisy crop blocks of the fuzz tuples
    for f64 in (False, True):
        raw = np.asarray(b["u_prev"]) + b["action"].astype(np.float64) * 0.1
        u = S.applied_control(b["u_prev"], b["action"], f64)
        assert np.all(u[S.CLIP_HIGH_ROW] == 1.0) and np.all(raw[S.CLIP_HIGH_ROW] > 1.0)
        assert np.all(u[S.CLIP_LOW_ROW] == 0.0) and np.all(raw[S.CLIP_LOW_ROW] < 0.0)
        inside = (raw > 1e-3) & (raw < 1 - 1e-3)
        assert inside.sum() > 200 and np.all((u[inside] > 0) & (u[inside] < 1))
    w14 = S.weather_table(14)
    assert np.array_equal(w14[:, :10], b["D"]) and np.all(w14[:, 10] == 45.0) and np.all(w14[:, 11:] == 0.0)


def test_oracle_integrates_every_row_in_every_mode(oracle):
    """No failed row for any (scheme, verify, crop, parameter block, storage dtype, control path) the census uses; in the unverified
    runs every scheme has refined rows next to rows at the nominal count, among the fuzz rows or the calm ones."""
    modes = {}
    for c in S.CASES:
        for raw in ((c.raw, True) if S.verified_twin(c) else (c.raw,)):
            modes.setdefault((c.scheme, raw, c.crop, c.params, c.f64, c.pipe), c)
    for (scheme, raw, crop, params, f64, pipe), c in modes.items():
        h = S.host_inputs(c, raw)
        u = h["control"] if raw else S.applied_control(h["u_prev"], h["action"], f64)
        ref, retries, refined, failed = S.state_reference(h["x"], u, h["weather"], h["p"], h["crop"], scheme, pipe, verify=raw)
        assert not failed.any(), (scheme, raw, crop, params, f64, pipe, np.nonzero(failed)[0])
        assert np.all(np.isfinite(ref))
        assert (refined > 0).any()
        # The one mode without a nominal row is ODE_pipe (one-f32-pipe-rk4-epi0-occ1): tracking the 45 C pipe column of
        # tests/test_gpu_step_reset.py weather(14) refines all 65 rows, so that build runs without refined and nominal lanes side by side.
        if not raw:
            assert (refined == 0).any() != pipe, (scheme, crop, params, f64, pipe, int((refined > 0).sum()))
