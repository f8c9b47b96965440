"""The kernels on held-out OFF-TRAJECTORY one-step maps against a truth that no integrator of the project produced (VERDICT weak item 4):
tests/golden/holdout_stress.npz, 1 025 tuples of oracle/studies/stress_sc.py's five kinds -- one row into a seventeenth wavefront -- with
the reference's verdict per tuple recorded on the CPU (tests/test_holdout_stress_fixture.py checks the fixture, the fp32 margin and the
judging code).  tests/test_gpu_fuzz.py and the two build censuses show that the kernels compute the scheme on such inputs; this shows
whether what they compute is right, and that the BDF integrator -- never run off a fixture trajectory before -- follows its CPU port
there, where its Newton iteration starts at the exchange laws' kinks.

Explicit integrators, ls5 at throughput (n_sub 128, window 2) and parity (192, window 1), unverified and verified, one glgym_evalF call
per build through the C ABI (tests/test_gpu_evalf_builds.py::call: sentinel-filled output between guard rows, inputs checked unwritten,
the session stopped on GLGYM_EHIP or a device error; the build that ran is read back).  Per-row parameter blocks (a third of the rows
carry a crop block) reach the fp64 crop build and the fp32 one-lane crop build with all 1 025 rows; the fp32 four-lane build and the two
PAIR builds exist for a shared block only (csrc/gl_step_select.hpp), so they run the rows that carry no crop block.
  fp64: every row's verdict (real / floor / clean at 1e-4 K) equals the recorded oracle verdict, and the state is within
        tests/test_gpu_fuzz.py's 1e-11 of the recorded oracle state.
  fp32: judged at 2e-4 K; the real offenders are a subset of the configuration's allowed set, fixed on the CPU from reference code alone.
BDF through glgym_evalF at 1e-6 and 1e-8: the same bits on an fp64 and an fp32 handle, tests/test_gpu_bdf.py::compare against the recorded
CPU-port rows, the error against the truth within 1.25 x the CPU port's, no real offender where the port has none, a second call the same.
The env-step route (rows 0 ... 129 through TomatoVecEnv.step_raw_control): fp64, fp32 in both layouts, and BDF env-steps.

With GLGYM_HOLDOUT_STRESS=<path> in the environment every measured figure is written there (profiles/holdout_stress.txt is such a file)."""
import ctypes as C
import os

import numpy as np
import pytest

import envlayer_inputs as E
import evalf_build_inputs as V
from conftest import STATE_NAMES
from test_gpu_bdf import compare
from test_gpu_evalf_builds import call
from test_holdout_stress_fixture import CONFIGS, FLOOR, REAL, VERIFIED, allowed, param_blocks, state_difference, verdicts
from test_jump_fixture import sce

pytestmark = pytest.mark.gpu

ENV_ROWS = 130                                   # 65 x 2: a ragged last wavefront at one, four and eight lanes per environment
_lines, _cache = [], {}
# variant -> (fp64, rows "all" / "plain", layout, ladder_parallel, family expected, crop build expected)
VARIANTS = {"f64": (True, "all", V.LAYOUT_AUTO, 0, V.QUAD, 1), "f32-one": (False, "all", V.LAYOUT_ONE, 0, V.ONE_LANE, 1),
            "f32-quad": (False, "plain", V.LAYOUT_AUTO, 0, V.QUAD, 0),
            "f64-pair": (True, "plain", V.LAYOUT_AUTO, 1, V.QUAD_PAIR, 0), "f32-pair": (False, "plain", V.LAYOUT_AUTO, 1, V.QUAD_PAIR, 0)}
EXPLICIT = [(c, v) for c in range(4) for v in VARIANTS if c in VERIFIED or not v.endswith("pair")]


def note(line):
    print(line)
    _lines.append(line)


def data(golden):
    if "data" not in _cache:
        g = golden("holdout_stress")
        p0 = golden("params_default")["p"].astype(np.float64)
        _cache["data"] = (g, golden("holdout_stress_bdf"), p0, param_blocks(g, p0))
    return _cache["data"]


def evalf(golden, key, f64, rows, first, layout=V.LAYOUT_AUTO, ladder_parallel=0, verify=V.VERIFY_AUTO, integrator=0, stats=False):
    """One glgym_evalF call on the given rows (cached by key): per-row blocks where a row among them carries a crop block."""
    from gl_gym_amd import _lib as L
    if key in _cache:
        return _cache[key]
    g, b, p0, P = data(golden)
    per_row = bool(g["crop_flag"][rows].any())
    r = call(f64, "ls5", V.Mode("holdout", verify, ladder_parallel, layout), g["X"][rows], g["U"][rows], g["D"][rows],
             P[rows] if per_row else None, len(rows) if per_row else 1, params=p0, integrator=integrator, first=first)
    hd = r.pop("hd")
    if stats:
        s = np.zeros((len(rows), L.NSOLVER_STAT), dtype=np.int32)
        assert hd.lib.glgym_get_solver_stats(hd.h, len(rows), s.ctypes.data_as(C.POINTER(C.c_int32))) == L.OK, hd.error()
        r["stats"] = s
    hd.close()
    assert r["rc"] == L.OK, (key, r["rc"], r["msg"])                       # the reference fails on no row
    assert np.all(np.isfinite(r["out"])), (key, np.flatnonzero(~np.isfinite(r["out"]).all(axis=1))[:8])
    _cache[key] = r
    return r


def explicit(golden, c, variant):
    from gl_gym_amd import _lib as L
    g = data(golden)[0]
    f64, which, layout, ladder, family, crop = VARIANTS[variant]
    n_sub, window, verify = g["configs"][c].tolist()
    rows = np.arange(len(g["X"])) if which == "all" else np.flatnonzero(~g["crop_flag"])

    def first(hd):
        assert hd.lib.glgym_set_n_sub(hd.h, n_sub) == L.OK and hd.lib.glgym_set_window(hd.h, window) == L.OK, hd.error()
    r = evalf(golden, ("explicit", c, variant), f64, rows, first, layout, ladder, V.VERIFY_AUTO if verify else V.VERIFY_NEVER)
    lanes = {V.ONE_LANE: 1, V.QUAD: 4, V.QUAD_PAIR: 8}[family]
    assert r["record"] == (family, int(f64), crop, int(f64), 0, V.LS5, -(-lanes * len(rows) // 64), len(rows)), (CONFIGS[c], variant, r["record"])
    return r, rows


def offenders(g, got, rows, abs_floor):
    v = verdicts(got, g["X_tight"][rows], abs_floor)
    es = sce(got, g["X_tight"][rows])
    e = es.max(axis=1)
    real = rows[v == REAL]
    states = [STATE_NAMES[int(j)] for j in es[v == REAL].argmax(axis=1)]
    return v, e, real, (f"max {e.max():.2e} (row {int(rows[e.argmax()])}), real {len(real)} by kind {np.bincount(g['kind'][real], minlength=5).tolist()} "
                        f"rows {real.tolist()} worst states {states}, at the floor {int((v == FLOOR).sum())}")


@pytest.mark.parametrize("c,variant", EXPLICIT, ids=[f"{CONFIGS[c]}-{v}" for c, v in EXPLICIT])
def test_explicit_integrators_against_the_truth(golden, c, variant):
    g = data(golden)[0]
    r, rows = explicit(golden, c, variant)
    f64 = VARIANTS[variant][0]
    v, e, real, text = offenders(g, r["out"], rows, 1e-4 if f64 else 2e-4)
    if f64:
        diff = state_difference(r["out"], g["X_oracle"][c][rows], g["X"])
        want = verdicts(g["X_oracle"][c][rows], g["X_tight"][rows])
        note(f"evalF {CONFIGS[c]:20s} {variant:8s} {len(rows):4d} rows: {text}; verdicts differing from the oracle's {int((v != want).sum())}, "
             f"worst scaled |state - oracle| {diff.max():.2e} (row {int(rows[diff.argmax()])})")
        assert np.array_equal(v, want), (CONFIGS[c], variant, rows[v != want].tolist())
        assert diff.max() <= 1e-11, (CONFIGS[c], variant, float(diff.max()), int(rows[diff.argmax()]))
    else:
        ok = allowed(g, c)
        outside = [int(i) for i in real if not ok[i]]
        note(f"evalF {CONFIGS[c]:20s} {variant:8s} {len(rows):4d} rows: {text}; allowed set {int(ok[rows].sum())} rows "
             f"(m32 {g['m32'][c]:.2e}), offenders outside it {outside}")
        assert not outside, (CONFIGS[c], variant, outside, e[np.isin(rows, outside)].tolist())


@pytest.mark.parametrize("c", VERIFIED, ids=[CONFIGS[c] for c in VERIFIED])
def test_pair_ladder_equals_the_sequential_ladder(golden, c):
    """include/glgym.h glgym_set_ladder_parallel: the same bits.  fp64: the plain rows of the all-rows call (crop build, per-row blocks
    equal to the handle's on these rows) against the PAIR build; fp32: the four-lane build against the PAIR build."""
    g = data(golden)[0]
    plain = np.flatnonzero(~g["crop_flag"])
    for a, b in (("f64", "f64-pair"), ("f32-quad", "f32-pair")):
        (ra, rows_a), (rb, rows_b) = explicit(golden, c, a), explicit(golden, c, b)
        assert np.array_equal(rows_b, plain)
        assert np.array_equal(E.bits(ra["out"][np.isin(rows_a, plain)]), E.bits(rb["out"])), (CONFIGS[c], a, b)


def bdf_call(golden, t, f64, again=False):
    from gl_gym_amd import _lib as L
    g, b = data(golden)[:2]
    tol = float(b["tols"][t])

    def first(hd):
        assert hd.lib.glgym_set_tolerances(hd.h, tol, tol, 10000) == L.OK, hd.error()
    r = evalf(golden, ("bdf", t, f64, again), f64, np.arange(len(g["X"])), first, integrator=L.INTEGRATORS["bdf"], stats=True)
    assert r["record"] == (-1, 0, 0, 0, 0, 0, 0, len(g["X"]))
    return r


@pytest.mark.parametrize("t", [0, 1], ids=["1e-6", "1e-8"])
def test_bdf_against_its_cpu_port_and_the_truth(golden, oracle, t):
    g, b = data(golden)[:2]
    XT, R, SR = g["X_tight"], b["X_bdf"][t], b["bdf_stats"][t].astype(np.int64)
    r = bdf_call(golden, t, True)
    G, S = r["out"], r["stats"].astype(np.int64)
    r32, again = bdf_call(golden, t, False), bdf_call(golden, t, True, again=True)
    assert np.array_equal(E.bits(r32["out"]), E.bits(G)) and np.array_equal(r32["stats"], r["stats"])       # an fp32 handle: the same bits
    assert np.array_equal(E.bits(again["out"]), E.bits(G)) and np.array_equal(again["stats"], r["stats"])   # a second call: the same bits
    same = np.all(S == SR, axis=1)
    e_gpu, e_cpu = oracle.scaled_rel_err(G, XT), oracle.scaled_rel_err(R, XT)
    v, e, real, text = offenders(g, G, np.arange(len(G)), 1e-4)
    real_cpu = np.flatnonzero(verdicts(R, XT) == REAL)
    other = np.flatnonzero(~same)
    note(f"evalF BDF rtol = atol = {b['tols'][t]:g}: {text}; statistics identical to the CPU port's on {int(same.sum())} of {len(G)} rows "
         f"(share {same.mean():.4f}; the others by kind {np.bincount(g['kind'][other], minlength=5).tolist()}), difference from the port on those "
         f"{(oracle.scaled_rel_err(G[same], R[same]) if same.any() else 0.0):.2e}, on all {oracle.scaled_rel_err(G, R):.2e}; error against the truth "
         f"GPU {e_gpu:.2e}, CPU port {e_cpu:.2e}; RHS evaluations per row mean {S[:, 1].mean():.0f} max {S[:, 1].max()} (CPU port mean "
         f"{SR[:, 1].mean():.0f} max {SR[:, 1].max()})")
    compare(oracle, G, S, R, SR, f"holdout_stress BDF {b['tols'][t]:g}")
    assert e_gpu <= 1.25 * e_cpu, (e_gpu, e_cpu)
    assert set(real.tolist()) <= set(real_cpu.tolist()), real.tolist()


def env_step(golden, dtype, rows, crop, layout=None, integrator="explicit"):
    """Rows `rows` of the fixture as one batch through TomatoVecEnv.step_raw_control (tests/test_gpu_stress.py's set-up; the rows' crop
    blocks as a hand-set per-env block where crop is set) -> new states (the clock column taken from the truth: an env-step sets it
    from its step counter), step_flags, done, (scheme, n_sub, window), the build that ran (glgym_last_step_build)."""
    import torch
    from gl_gym_amd import _lib as L
    from gl_gym_amd.tomato_env import TomatoVecEnv
    g, b, p0, P = data(golden)
    X, U, D = g["X"][rows], g["U"][rows], g["D"][rows]
    B = len(rows)
    env = TomatoVecEnv(B, weather=np.repeat(D, 4, axis=0), params=p0, dtype=dtype, season_length=0.02, pred_horizon=0, auto_reset=False,
                       uncertainty_scale=0.1 if crop else 0.0, integrator=integrator)
    env.reset()
    if layout is not None:
        env.set_layout(layout)
    if crop:
        env.freeze_crop_noise = True
        env.crop_T[:, :B].copy_(torch.as_tensor(np.ascontiguousarray(g["P_crop"][rows].T), dtype=env.tdtype, device=env.device))
    env.w_off_t.copy_(torch.arange(B, dtype=torch.int32, device=env.device) * 4)
    env.x.copy_(torch.as_tensor(X, dtype=env.tdtype, device=env.device))
    settings = (env.scheme, env.n_sub, env.window)
    obs, r, done, infos = env.step_raw_control(U)
    fl = env.step_flags_t.cpu().numpy().copy()
    x = env.x.double().cpu().numpy().copy()
    x[:, 27] = g["X_tight"][rows][:, 27]
    rec = (C.c_int32 * 10)()
    L.check(env._lib.glgym_last_step_build(env._h, rec), "glgym_last_step_build")
    env.close()
    return x, fl, np.asarray(done), settings, tuple(rec)


@pytest.mark.parametrize("variant", ["f64", "f32-one", "f32-auto", "bdf"])
def test_env_step_route(golden, variant):
    from gl_gym_amd import _lib as L
    g, b = data(golden)[:2]
    head = np.arange(ENV_ROWS)
    if variant == "f32-auto":                                    # no fp32 four-lane build takes per-env crop blocks
        rows, crop = head[~g["crop_flag"][head]], False
    else:
        rows, crop = head, True
    f64 = variant in ("f64", "bdf")
    x, fl, done, settings, build = env_step(golden, "float64" if f64 else "float32", rows, crop, layout={"f32-one": "one", "f32-auto": "auto"}.get(variant),
                                     integrator="bdf" if variant == "bdf" else "explicit")
    assert not (fl & L.SF_FAILED).any() and not done.any(), (variant, rows[(fl & L.SF_FAILED) != 0].tolist())
    assert (fl >= 0).all()
    # family, f64, per-env crop blocks compiled in: so that a variant cannot pass on another build's results
    assert build[:3] == {"f64": (V.QUAD, 1, 1), "f32-one": (V.ONE_LANE, 0, 1), "f32-auto": (V.QUAD_PAIR, 0, 0), "bdf": (-1, 0, 0)}[variant], build
    if variant == "bdf":
        ref = bdf_call(golden, 0, True)
        assert np.array_equal(E.bits(x[:, :27]), E.bits(ref["out"][rows][:, :27])), "BDF env-step against glgym_evalF's BDF rows"
        assert np.all(fl & L.SF_BDF) and np.array_equal(fl >> 16, ref["stats"][rows][:, 0])
        v, e, real, text = offenders(g, x, rows, 1e-4)
        note(f"env-step BDF 1e-6, rows 0 ... {ENV_ROWS - 1}: {text}; bit-identical to glgym_evalF's BDF rows")
        assert set(real.tolist()) <= set(rows[verdicts(b["X_bdf"][0][rows], g["X_tight"][rows]) == REAL].tolist())
        return
    c = 3 if f64 else 1                                           # the handle's default preset: fp64 parity, fp32 throughput; raw controls: verified
    assert settings == (("ls5", 192, 1) if f64 else ("ls5", 128, 0)) and g["configs"][c].tolist() == ([192, 1, 1] if f64 else [128, 2, 1])
    v, e, real, text = offenders(g, x, rows, 1e-4 if f64 else 2e-4)
    if f64:
        want = verdicts(g["X_oracle"][c][rows], g["X_tight"][rows])
        diff = state_difference(x[:, :27], g["X_oracle"][c][rows][:, :27], g["X"][:, :27])
        note(f"env-step {variant:8s} ({CONFIGS[c]}), {len(rows)} rows: {text}; worst scaled |state - oracle| {diff.max():.2e}; extra attempts "
             f"{np.bincount((fl >> 8) & 7).tolist()}")
        assert np.array_equal(v, want), rows[v != want].tolist()
        assert diff.max() <= 1e-11, (float(diff.max()), int(rows[diff.argmax()]))
        assert np.array_equal(fl & 0xffff, g["flags"][c][rows] & 0xffff), rows[(fl & 0xffff) != (g["flags"][c][rows] & 0xffff)].tolist()
    else:
        ok = allowed(g, c)
        outside = [int(i) for i in real if not ok[i]]
        note(f"env-step {variant:8s} ({CONFIGS[c]}), {len(rows)} rows: {text}; offenders outside the allowed set {outside}; extra attempts "
             f"{np.bincount((fl >> 8) & 7).tolist()}")
        assert not outside, (variant, outside)


def test_measurements_file():
    """Last in the file: what the tests above measured, to GLGYM_HOLDOUT_STRESS if it is set."""
    path = os.environ.get("GLGYM_HOLDOUT_STRESS")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(_lines) + "\n")
