"""GPU tests of rng="numpy": the per-environment PCG64 streams on the device (csrc/glgym_rng.hip) against NumPy generators that follow
the reference's flow on the host -- reset: choice(years), choice(days) (tomato_env.py:236-241); every step: 34 uniforms
(tomato_env.py:118, noise.py:16-22), also at uncertainty_scale 0; environment b seeded with seed + b (RL/utils.py:39).
Every comparison of random numbers, start rows, start days, crop blocks and generator states is EXACT.  (NumPy 2.2.6 when written.)"""
import numpy as np
import pytest

from conftest import GOLDEN, scaled_err

pytestmark = pytest.mark.gpu

N_YEARS, N_DAYS = 3, 20


def np_gen(seed):               # gymnasium.utils.seeding.np_random
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))


def host_crop_blocks(gens, p32, scale):
    """parametric_crop_uncertainty for every generator -> float32 [B, 34] (noise.py:16-22: float32 block += float64 noise * block,
    evaluated in float64 and rounded; p144 = p141 / p142 in float32; tests/test_np_stream_host.py holds this against the fixture)."""
    noise = np.stack([g.uniform(-scale / 2, scale / 2, size=34) for g in gens])
    p = p32[128:162].astype(np.float64)
    out = (p[None, :] + noise * p[None, :]).astype(np.float32)
    out[:, 16] = out[:, 13] / out[:, 14]
    return out


def short_season_env(B, dtype, scale, seed, **kw):
    """60 starts on a 3 x 20 grid, episodes of N + 1 = 10 steps: three episodes fit in 30 steps."""
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    w = synthetic_weather(n_rows=2000)
    rows = 16 * np.arange(N_YEARS * N_DAYS) + 3
    days = (np.arange(N_YEARS * N_DAYS) % N_DAYS) * 7.0 + 11.0
    env = TomatoVecEnv(B, weather=w, dtype=dtype, season_length=0.1, pred_horizon=0.05, start_rows=rows, start_days=days,
                       uncertainty_scale=scale, seed=seed, rng="numpy", start_grid=(N_YEARS, N_DAYS), **kw)
    assert env.N == 9 and env.Np == 4
    return env, rows, days.astype(np.float32)


def host_reset_draw(gens, which, rows, days, w_off, start_day):
    for b in which:
        iy, idd = gens[b].choice(np.arange(N_YEARS)), gens[b].choice(np.arange(N_DAYS))
        w_off[b], start_day[b] = rows[iy * N_DAYS + idd], days[iy * N_DAYS + idd]


@pytest.mark.parametrize("scale", [0.2, 0.0])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("B", [1000, 4096])
def test_streams_follow_numpy_through_three_episodes(B, dtype, scale):
    """7. / 8. crop blocks, start rows, start days at every step and the final generator states; scale 0 exercises advance(34)."""
    import torch
    seed = 666
    env, rows, days = short_season_env(B, dtype, scale, seed, auto_reset=True)
    gens = [np_gen(seed + b) for b in range(B)]
    assert env.get_rng_state() == [g.bit_generator.state for g in gens]
    w_off, start_day = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.float32)
    env.reset_tensor()
    host_reset_draw(gens, range(B), rows, days, w_off, start_day)
    assert np.array_equal(env.w_off_t.cpu().numpy(), w_off) and np.array_equal(env.start_day_t.cpu().numpy(), start_day)
    assert len(np.unique(w_off)) == N_YEARS * N_DAYS if B >= 1000 else True           # the whole grid is reached
    tg = torch.Generator(device=env.device)
    tg.manual_seed(5)
    n_done, mismatches = 0, 0
    assert (env.crop_T is None) == (scale == 0.0)
    for k in range(31):
        _, _, done_t, _ = env.step_tensor(torch.rand(B, 6, generator=tg, device=env.device) * 2 - 1)
        done = done_t.cpu().numpy().astype(bool)
        if scale > 0:
            want = host_crop_blocks(gens, env.p, scale)
            got = env.crop_T[:, :B].t().double().cpu().numpy()
            mismatches += int((got != want.astype(np.float64)).sum())
        else:
            for g in gens:
                g.uniform(-0.0, 0.0, size=34)
        assert done.all() == done.any() and done.all() == (k % 10 == 9), k               # episodes of N + 1 = 10 steps, none cut short
        host_reset_draw(gens, np.nonzero(done)[0], rows, days, w_off, start_day)
        n_done += int(done.sum())
        mismatches += int((env.w_off_t.cpu().numpy() != w_off).sum()) + int((env.start_day_t.cpu().numpy() != start_day).sum())
    assert n_done == 3 * B and mismatches == 0, (n_done, mismatches)
    assert env.get_rng_state() == [g.bit_generator.state for g in gens]
    assert env.metrics()["n_ode_fail"] == 0
    env.close()


# Fixture leg (c) chained over its eight steps with the crop blocks of the fixture copied into crop_T by hand before every step
# (rng="philox", freeze_crop_noise; state and controls free-running), measured on an MI355X with the kernels of the commit before
# this mode existed: (max scaled state error, scaled error of the 7 state-derived observations, |d reward|, |d EPI / revenue|).
CHAINED_TEACHER_FORCED = {
    ("explicit", "float64"): (2.2607e-06, 1.1040e-06, 1.3146e-06, 3.3321e-09),
    ("explicit", "float32"): (1.9277e-05, 6.6551e-06, 8.0425e-06, 2.9322e-08),
    ("bdf", "float64"): (1.4911e-05, 1.6604e-06, 1.0052e-05, 3.0772e-09),
    ("bdf", "float32"): (1.4917e-05, 1.6964e-06, 9.9922e-06, 3.3035e-09),
}


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("integrator", ["explicit", "bdf"])
def test_fixture_leg_c_free_running_from_seed_668(golden, integrator, dtype):
    """9. The reference's real TomatoEnv after reset(seed=668) with uncertainty_scale = 0.2, eight steps (tests/golden/refenv_1day.npz
    leg (c)): ONE environment built with rng="numpy", seed=668, fed the fixture's actions and nothing else -- no teacher forcing.  The
    crop blocks must equal un_p bit for bit; state, observation, reward and info are held against the fixture within 1.1 x what the
    same eight chained steps read when the fixture's blocks are copied in by hand (CHAINED_TEACHER_FORCED): the blocks being
    identical, any excess would be a defect of the stream path, not integration error.
    Measured on an MI355X (state / obs / reward / EPI-revenue): teacher-forced chained = the table above, all inside the one-step bounds
    of tests/test_gpu_refenv.py:88-98 (1e-4 / 2e-4 / 2e-4 / 3e-6); this mode: the same figures to every printed digit
    (explicit fp64 2.2607e-06 / 1.1040e-06 / 1.3146e-06 / 3.3321e-09, explicit fp32 1.9277e-05 / 6.6551e-06 / 8.0425e-06 / 2.9322e-08,
    bdf fp64 1.4911e-05 / 1.6604e-06 / 1.0052e-05 / 3.0772e-09, bdf fp32 1.4917e-05 / 1.6964e-06 / 9.9922e-06 / 3.3035e-09)."""
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd._lib import INFO_KEYS
    g = golden("refenv_1day")
    U, X, OBS, R, INFO, P = (g[f"un_{k}"] for k in ("u", "x", "obs", "reward", "info", "p"))
    assert len(U) == 8 and P.shape == (8, 208)
    env = TomatoVecEnv(1, weather=g["weather"], params=g["p"], dtype=dtype, season_length=1, pred_horizon=0.5, start_rows=[0],
                       start_days=[0.0], auto_reset=False, uncertainty_scale=0.2, rng="numpy", seed=668, integrator=integrator)
    obs0 = env.reset()
    np.testing.assert_allclose(obs0[0], OBS[0], rtol=2e-6, atol=2e-6)
    xs, obs_l, r_l, info_l, u_l = [], [], [], [], []
    for k in range(8):
        obs, r, done, infos = env.step(g["un_actions"][k:k + 1])
        assert np.array_equal(env.crop_T[:, 0].double().cpu().numpy(), P[k, 128:162]), k            # bit for bit
        assert not done.any()
        xs.append(env.x.double().cpu().numpy()[0].copy()); obs_l.append(obs[0].copy()); r_l.append(float(r[0]))
        info_l.append([infos[0][q] for q in INFO_KEYS]); u_l.append(env.u.double().cpu().numpy()[0].copy())
    xs, obs, r, info, u = map(np.array, (xs, obs_l, r_l, info_l, u_l))
    gen = np_gen(668)
    for _ in range(8):
        gen.uniform(-0.1, 0.1, size=34)
    assert env.get_rng_state() == [gen.bit_generator.state]
    ref = OBS[1:9]
    sc = np.maximum(np.abs(ref[:, :7]), 1e-3 * np.abs(ref[:, :7]).max(axis=0))
    e_x, e_obs = scaled_err(xs, X[1:9]), float(np.max(np.abs(obs[:, :7] - ref[:, :7]) / sc))
    e_r, e_info = float(np.max(np.abs(r - R))), float(np.max(np.abs(info[:, 0:2] - INFO[:, 0:2])))
    print(f"leg (c) free-running {integrator} {dtype}: state {e_x:.4e}, obs {e_obs:.4e}, reward {e_r:.4e}, EPI/revenue {e_info:.4e}")
    b_x, b_obs, b_r, b_info = (1.1 * v for v in CHAINED_TEACHER_FORCED[(integrator, dtype)])
    np.testing.assert_allclose(u, U, rtol=0, atol=1e-7 if dtype == "float32" else 1e-15)
    assert e_x <= b_x and e_obs <= b_obs and e_r <= b_r and e_info <= b_info, (e_x, e_obs, e_r, e_info)
    # what does not depend on the integration keeps the tolerances of the one-step test (tests/test_gpu_refenv.py:92, 97)
    np.testing.assert_allclose(obs[:, 7:], ref[:, 7:], rtol=3e-6, atol=3e-6)
    np.testing.assert_allclose(info[:, 2:7], INFO[:, 2:7], rtol=2e-6, atol=1e-9)
    env.close()


def test_captured_step_graph_draws_the_same_stream():
    """10. ten replayed steps of a captured graph = ten eager steps from the same seed: crop blocks, start draws, final states."""
    import torch
    B, seed = 256, 4242
    runs = []
    for captured in (False, True):
        env, _, _ = short_season_env(B, "float32", 0.2, seed, auto_reset=True)
        env.reset_tensor()
        before = env.get_rng_state()
        step = env.capture_step_graph() if captured else env.step_tensor
        assert env.get_rng_state() == before                   # the warm-up's draws were put back
        tg = torch.Generator(device=env.device)
        tg.manual_seed(9)
        crops, starts, n_done = [], [], 0
        for k in range(10):
            _, _, done_t, _ = step(torch.rand(B, 6, generator=tg, device=env.device) * 2 - 1)
            crops.append(env.crop_T[:, :B].cpu().numpy().copy())
            starts.append((env.w_off_t.cpu().numpy().copy(), env.start_day_t.cpu().numpy().copy()))
            n_done += int(done_t.sum())
        assert n_done == B                                     # the auto-reset's draws are inside the captured sequence
        runs.append((crops, starts, env.get_rng_state(), env.x.cpu().numpy().copy()))
        env.close()
    (c0, s0, st0, x0), (c1, s1, st1, x1) = runs
    for k in range(10):
        assert np.array_equal(c0[k], c1[k]) and np.array_equal(s0[k][0], s1[k][0]) and np.array_equal(s0[k][1], s1[k][1]), k
    assert st0 == st1 and np.array_equal(x0, x1)
    gens = [np_gen(seed + b) for b in range(B)]                # and both are NumPy's: 2 choices, 10 x 34 uniforms, 2 choices
    for g in gens:
        g.choice(np.arange(N_YEARS)), g.choice(np.arange(N_DAYS))
        g.uniform(-0.1, 0.1, size=340)
        g.choice(np.arange(N_YEARS)), g.choice(np.arange(N_DAYS))
    assert st1 == [g.bit_generator.state for g in gens]


def test_default_generator_did_not_move():
    """11. rng="philox" (the default): crop blocks over 20 steps against the Philox4x32-10 definition to the one-ulp allowance of
    tests/test_gpu_parity.py (fma contraction of p + noise * p), start draws equal to a restatement of reset_kernel's draw."""
    import torch
    from test_controller_and_noise import expected_crop_noise, philox4x32_10
    from gl_gym_amd.tomato_env import TomatoVecEnv
    from gl_gym_amd.utils import synthetic_weather
    B, seed = 48, 4242
    rows = 16 * np.arange(7) + 3
    env = TomatoVecEnv(B, weather=synthetic_weather(n_rows=2000), dtype="float32", season_length=0.1, pred_horizon=0.05,
                       start_rows=rows, uncertainty_scale=0.2, seed=seed, auto_reset=True)
    assert env.rng == "philox" and env.rng_state_t is None and env.start_grid is None
    with pytest.raises(Exception):
        env.get_rng_state()
    env.reset_tensor()
    episode = np.zeros(B, dtype=np.int64)

    def start_draw(which):
        for b in which:
            r = philox4x32_10([b, int(episode[b]), 0x5EED, 0], [seed & 0xFFFFFFFF, seed >> 32])
            want[b] = rows[r[0] % len(rows)]
            episode[b] += 1
    want = np.zeros(B, dtype=np.int64)
    start_draw(range(B))
    assert np.array_equal(env.w_off_t.cpu().numpy(), want)
    tg = torch.Generator(device=env.device)
    tg.manual_seed(1)
    for k in range(20):
        _, _, done_t, _ = env.step_tensor(torch.rand(B, 6, generator=tg, device=env.device) * 2 - 1)
        crop = env.crop_T[:, :B].cpu().numpy()
        exp = expected_crop_noise(env.p[128:162], B, 0.2, seed, k)
        rel = np.abs(crop - exp) / np.abs(exp)
        drawn = np.arange(34) != 16
        assert np.max(rel[drawn]) < 1.3e-7, (k, float(np.max(rel[drawn])))
        # p144 = p141 / p142 is derived: exactly the float32 quotient of the device's own two entries, hence within the two one-ulp
        # inputs' propagation plus its own rounding (3 x 2^-23) of the definition's
        assert np.array_equal(crop[16], crop[13] / crop[14]) and np.max(rel[16]) < 3 * 1.1921e-7, (k, float(np.max(rel[16])))
        start_draw(np.nonzero(done_t.cpu().numpy())[0])
        assert np.array_equal(env.w_off_t.cpu().numpy(), want), k
        assert np.array_equal(env.start_day_t.cpu().numpy(), (want * 900.0 / 86400).astype(np.float32))
    assert episode.min() == 3
    env.close()


def test_seeding_checkpoint_and_single_env_view():
    """reset_tensor(seed) / seed() / set_seed() reseed; a reset without a seed continues the stream; get / set_rng_state checkpoint
    a run; TomatoEnv.reset(seed=s) is the reference env's reset(seed=s); env_index_offset shifts a shard's seeds."""
    import torch
    from gl_gym_amd.tomato_env import TomatoEnv
    from gl_gym_amd.utils import synthetic_weather
    B = 100
    env, rows, days = short_season_env(B, "float32", 0.2, 7, auto_reset=False, env_index_offset=1000)
    assert env.get_rng_state() == [np_gen(7 + 1000 + b).bit_generator.state for b in range(B)]
    for reseed in (lambda: env.reset_tensor(seed=11), lambda: (env.seed(11), env.reset_tensor()), lambda: (env.set_seed(11), env.reset_tensor())):
        reseed()
        gens = [np_gen(11 + 1000 + b) for b in range(B)]
        w_off, sd = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.float32)
        host_reset_draw(gens, range(B), rows, days, w_off, sd)
        assert np.array_equal(env.w_off_t.cpu().numpy(), w_off) and env.get_rng_state() == [g.bit_generator.state for g in gens]
    env.reset_tensor()                                      # no seed: the streams go on (gymnasium.Env.reset(seed=None))
    host_reset_draw(gens, range(B), rows, days, w_off, sd)
    assert np.array_equal(env.w_off_t.cpu().numpy(), w_off) and np.array_equal(env.start_day_t.cpu().numpy(), sd)
    a = torch.zeros(B, 6, device=env.device)
    env.step_tensor(a)
    ckpt, crop_next = env.get_rng_state(), None
    env.step_tensor(a)
    crop_next = env.crop_T.clone()
    env.step_tensor(a)
    env.set_rng_state(ckpt)
    env.step_tensor(a)
    assert torch.equal(env.crop_T, crop_next)
    with pytest.raises(ValueError):
        env.set_rng_state(ckpt[:5])
    env.close()
    from gl_gym_amd.tomato_env import TomatoVecEnv
    for bad in (dict(rng="numpy", start_grid=(2, 2)), dict(rng="pcg64")):
        with pytest.raises(ValueError):
            TomatoVecEnv(4, start_rows=[0, 16, 32], season_length=0.1, **bad)
    one = TomatoEnv(weather=synthetic_weather(n_rows=400), season_length=0.1, pred_horizon=0.05, uncertainty_scale=0.2, rng="numpy")
    one.reset(seed=668)
    one.step(np.zeros(6, dtype=np.float32))
    g = np_gen(668)
    want = host_crop_blocks([g], one.p, 0.2)[0]
    assert np.array_equal(one.vec.crop_T[:, 0].double().cpu().numpy(), want.astype(np.float64))
    one.reset()                                             # continues: the next block is NumPy's next 34 draws
    one.step(np.zeros(6, dtype=np.float32))
    assert np.array_equal(one.vec.crop_T[:, 0].double().cpu().numpy(), host_crop_blocks([g], one.p, 0.2)[0].astype(np.float64))
    one.close()


def test_make_vec_env_walks_the_references_seeded_starts(tmp_path, golden):
    """make_vec_env(..., seed=s, rng="numpy"): environment b is the reference's rank b -- reset(s + b) inside make_env
    (RL/utils.py:39), then the caller's reset() draws again; the start grid is (len(years), len(days)) of the config."""
    from gl_gym_amd.make_env import load_env_params, make_vec_env
    g = golden("weather_bleiswijk2009")
    cols = [str(c) for c in g["small_raw_cols"]]
    raw = np.concatenate([g["small_raw"], g["small_raw"]])
    raw[:, cols.index("time")] = 300.0 * np.arange(len(raw))
    wdir = tmp_path / "weather" / "Testville"
    wdir.mkdir(parents=True)
    with open(wdir / "GL2009.csv", "w") as f:
        f.write(",".join(cols) + "\n")
        for r in raw:
            f.write(",".join(repr(float(v)) for v in r) + "\n")
    (tmp_path / "TomatoEnv.yml").write_text((GOLDEN / "TomatoEnvSmall.yml").read_text().replace("WEATHER_DIR", str(tmp_path / "weather")))
    base, spec = load_env_params("TomatoEnv", str(tmp_path))
    B, seed = 64, 666
    env = make_vec_env("TomatoEnv", base, spec, seed=seed, n_envs=B, dtype="float32", rng="numpy")
    v = env.venv
    assert v.rng == "numpy" and v.start_grid == (1, 2)
    gens = [np_gen(seed + b) for b in range(B)]
    first = np.array([(g_.choice([2009]), g_.choice([0, 1]))[1] for g_ in gens], dtype=np.float32)
    assert np.array_equal(v.start_day_t.cpu().numpy(), first)
    env.reset()
    second = np.array([(g_.choice([2009]), g_.choice([0, 1]))[1] for g_ in gens], dtype=np.float32)
    assert np.array_equal(v.start_day_t.cpu().numpy(), second) and len(np.unique(second)) == 2
    assert v.get_rng_state() == [g_.bit_generator.state for g_ in gens]
    env.close()
