"""CPU checks of the evalF build census's table, inputs and references (tests/evalf_build_inputs.py): the table is the evalF build list of
csrc/gl_step_select.hpp, every recipe selects its build with the expected grid, the oracle integrates every row in every mode the
census uses, and the rows are what the census needs them to be: refined and nominal rows side by side in the unverified runs, rows
accepted beyond the first and beyond the second rung of the ladder in the verified ones (so that the PAIR builds run their second round)."""
import numpy as np
import pytest

import envlayer_inputs as E
import evalf_build_inputs as V
import step_build_inputs as S


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return S.stepselect_host(tmp_path_factory.mktemp("stepselecthost"))


def test_the_table_is_the_build_list(host):
    n = host.evalfselect_builds(None, 0)
    listed = np.zeros((n, 5), dtype=np.int32)
    assert host.evalfselect_builds(listed.ctypes.data, n) == n
    assert len(V.BUILD_CASES) == 29 and len({c.build for c in V.BUILD_CASES}) == 29
    assert {c.build for c in V.BUILD_CASES} == {tuple(r) for r in listed.tolist()}
    assert len(V.CASES) == 31 and len({c.id for c in V.CASES}) == 31
    extra = [c for c in V.CASES if c not in V.BUILD_CASES]
    assert sorted(c.build for c in extra) == [(V.QUAD, 1, 0, 1, V.RK4), (V.QUAD_PAIR, 1, 0, 1, V.RK4)] and all(c.pipe for c in extra)
    assert all(c.scheme == "rk4" for c in V.CASES if c.pipe)
    assert V.BY_ID["one-f32-crop-rk3"].build == (V.ONE_LANE, 0, 1, 0, V.RK3) and V.BY_ID["pair-f64-rk4-runpipe"].nd == 14
    # modes: PAIR verified only; everything else unverified, and verified on the sequential ladder
    for c in V.CASES:
        ms = V.modes(c)
        if c.build[0] == V.QUAD_PAIR:
            assert [(m.name, m.ladder_parallel) for m in ms] == [("verified", 1)]
        else:
            assert [(m.name, m.verify, m.ladder_parallel) for m in ms] == [("plain", V.VERIFY_NEVER, 1), ("verified", V.VERIFY_AUTO, 0)]
            if c.build[0] == V.ONE_LANE and not c.crop:
                assert all(m.layout == V.LAYOUT_ONE for m in ms)
    assert len(V.RUNS) == 2 * 31 - 9


@pytest.mark.parametrize("n_simd", [1024, 256])
def test_every_recipe_selects_its_build(host, n_simd):
    runs = [(c, m, B) for c, m in V.RUNS for B in V.BATCHES]
    rows = np.array([V.select_inputs(c, m, B, n_simd) for c, m, B in runs], dtype=np.int32)
    out = np.full((len(rows), 7), -7, dtype=np.int32)
    host.evalfselect_batch(len(rows), rows.ctypes.data, out.ctypes.data)
    for (c, m, B), got in zip(runs, out.tolist()):
        assert got == [0, *V.expected_build(c, B), V.grid(c, B)], (c.id, m.name, B, got)
        if B > 1:
            assert V.expected_build(c, B) == c.build
    assert V.BATCHES == (65, 1)
    assert [V.grid(V.BY_ID[i], 65) for i in ("one-f32-ls5", "quad-f32-ls5", "pair-f32-ls5")] == [2, 5, 9]    # one live row in the last wavefront
    assert [V.grid(V.BY_ID[i], 1) for i in ("one-f32-ls5", "quad-f64-crop-ls5", "pair-f64-ls5")] == [1, 1, 1]


def test_rows():
    for f64 in (False, True):
        for scheme in V.SCHEMES:
            X, U, D, CROP = V.rows(f64, scheme)
            E.assert_rows_distinct(E.rounded(X[:, :27], f64))
            E.assert_rows_distinct(np.concatenate([U, D], axis=1))
            assert len(np.unique(CROP, axis=0)) >= 10
            assert all(i % 2 == 1 for i in V.REPLACED.get((f64, scheme), {}))
    b = S.base()
    assert np.array_equal(V.rows(True, "ls5")[0][::2], b["X"][::2])                    # the far-off rows are never replaced
    c = V.BY_ID["quad-f64-crop-rk4"]
    h = V.host_inputs(c)
    assert h["P"].shape == (65, 208) and np.array_equal(h["P"][:, 128:162], h["crop"])
    rest = np.delete(h["P"], np.s_[128:162], axis=1)
    assert np.all(rest == rest[0]) and np.array_equal(rest[0], np.delete(h["p"], np.s_[128:162]))   # shared outside the crop block
    for cc in V.CASES:                                                                 # the double-to-T load is exact
        hh = V.host_inputs(cc)
        if not cc.f64:
            for k in ("x", "u", "d", "crop"):
                if hh[k] is not None:
                    assert np.array_equal(hh[k], hh[k].astype(np.float32).astype(np.float64)), (cc.id, k)
        assert hh["d"].shape == (65, cc.nd)
    assert V.EXCLUDED_ROWS == 0
    x = V.host_inputs(V.BY_ID["one-f32-rk4"])["x"]
    t = V.tiny_of(x)
    assert np.array_equal((x + t).astype(np.float32), x.astype(np.float32)) and np.all((x + t != x) == (x != 0))


def test_rows_are_what_the_census_needs(oracle):
    """No failed row anywhere.  Unverified, per (dtype, scheme, parameter route): at least 8 rows refined by the stability control and
    at least 8 at the nominal count -- but for ODE_pipe, whose 45 C pipe column refines all 65 rows (as in the step census).
    Verified, per (dtype, scheme): a row accepted beyond the first rung and a row beyond the second."""
    seen = set()
    beyond = {}
    for c, m in V.RUNS:
        key = (c.f64, c.scheme, c.crop, c.pipe, m.name)
        if key in seen:
            continue
        seen.add(key)
        ref, retries, refined, failed = V.reference(c, m)
        assert not failed.any(), (key, np.nonzero(failed)[0])
        assert np.all(np.isfinite(ref))
        if m.name == "plain":
            n_ref, n_nom = int((refined > 0).sum()), int((refined == 0).sum())
            if c.pipe:
                assert n_ref == 65, (key, n_ref)
            else:
                assert n_ref >= 8 and n_nom >= 8, (key, n_ref, n_nom)
        else:
            b = beyond.setdefault((c.f64, c.scheme), [0, 0])
            b[0] = max(b[0], int((retries >= 1).sum()))
            b[1] = max(b[1], int((retries >= 2).sum()))
            if not c.crop:                                   # the route the PAIR builds run
                assert (retries >= 1).any() and (retries >= 2).any(), (key, np.bincount(retries))
    assert len(beyond) == 8 and all(v[0] >= 1 and v[1] >= 1 for v in beyond.values()), beyond
