"""Soft actor-critic on the GPU: glgym_sac_rows, glgym_sac_rows_grad, glgym_sac_batch, glgym_sac_loss, glgym_polyak (include/glgym.h),
gl_gym_amd.sac.squashed_sample, ReplayCollector and SAC.

What can be exact is compared bit for bit with the host instantiation of csrc/gl_sac.hpp (tests/sachost/sachost.cpp): the sampling indices,
the gathered rows, the backward pass, every output and sum of the two loss stages, the Polyak update.  What is not: the noise (Box-Muller in
double), std = exp, tanh and the log term go through the device's libm, which is not the host's -- eps, eps2, std, tanh and corr are compared
with NumPy's double results within one float32 ulp, and everything that follows from them exactly GIVEN the device's own values (the host
build takes them as inputs).  Every output buffer has guard rows behind its last row and guard bytes around it (0xFF); an optional output
that is not asked for and every output of a refused call must come back untouched."""
import ctypes as C

import numpy as np
import pytest

import envlayer_inputs as E
from test_gpu_collect import stack_of
from test_sac_host import (ALL_LOSS_OUT, BATCH_OUT, BATCH_REFUSALS, BLOCK, GRAD_REFUSALS, GUARD, IN_DIMS, LOSS_OUT, LOSS_REFUSALS, MAX_BLOCKS, MB_, NU,
                           POLYAK_COUNTS, P_, ROWS_OUT, ROWS_REFUSALS, UNIFORM_OUT, LossCase, RingCase, RowsCase, batch_args, batch_output_shapes,
                           build_host, grad_args, host_batch, host_grad, host_loss, host_rows, host_u, loss_args, loss_output_shapes, loss_rows,
                           np_clamp_ls, np_eps64, np_index, np_polyak, np_uniform, polyak_args, polyak_tensors, rows_args, rows_output_shapes,
                           same_bits, same_u32, set_path, within_one_f32_ulp)

pytestmark = pytest.mark.gpu
CAP_M = BLOCK * MAX_BLOCKS + 77                               # just past the grid's cap: the first 77 lanes of block 0 take a second row
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, CAP_M]
f = np.float32


@pytest.fixture(scope="module")
def hd():
    h = E.Handle(False)
    yield h
    h.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("sachost_gpu") / "libsachost.so")


def guarded_outputs(shapes):
    return {k: E.Guarded(shape=(s[0] + GUARD,) + tuple(s[1:]), dtype=dt) for k, (s, dt) in shapes.items()}


def read_outputs(outs, n_rows, written):
    """{name: rows < n} of the outputs in `written`; asserts every guard, and that the other outputs were not touched."""
    got = {}
    for k, g in outs.items():
        v = g.read()
        if k in written:
            n = n_rows[k] if isinstance(n_rows, dict) else n_rows
            assert np.all(v[n:].view(np.uint8) == 0xFF), f"a guard row of {k} was written"
            got[k] = v[:n]
        else:
            assert np.all(v.view(np.uint8) == 0xFF), f"{k} was written"
    return got


def same_named(got, want, names, n=None):
    for k in names:
        assert same_bits(got[k], want[k] if n is None else want[k][:n[k] if isinstance(n, dict) else n]), k


def launch(hd, fn, a):
    hd.sync()
    rc = fn(hd.h, C.byref(a), hd.stream())
    hd.sync()
    assert rc == 0, (rc, hd.error())


# ---- 1. the squashed Gaussian, forward -------------------------------------------------------------------------------------------------
class DeviceRows:
    def __init__(self, case):
        self.case = case
        self.inputs = {k: E.Guarded(v) for k, v in case.arrays().items()}
        self.outs = guarded_outputs(rows_output_shapes(case.M, case.in_dim))

    def args(self, want=ROWS_OUT, draw_base_ptr=None, **kw):
        return rows_args(self.case, lambda k: self.inputs[k].ptr, {k: self.outs[k].ptr for k in want}, draw_base=draw_base_ptr, **kw)

    def read(self, written):
        for g in self.inputs.values():
            g.read()
        return read_outputs(self.outs, self.case.M, written)


def run_rows(hd, case, want=ROWS_OUT, draw_base=None, **kw):
    dr = DeviceRows(case)
    base = None if draw_base is None else E.Guarded(np.array([draw_base], dtype=np.uint64))
    launch(hd, hd.lib.glgym_sac_rows, dr.args(want, None if base is None else base.ptr, **kw))
    return dr.read(want)


def check_rows(host, case, got, keys, step, D, seed, sigma=0.0, det=0, **kw):
    """The device's noise and transcendentals within one ulp of NumPy's, everything else the host build's given them."""
    M = case.M
    e, e2, std, a, l = (got[k] for k in ("eps", "eps2", "std", "tanh", "corr"))
    assert (not e.any()) if det else within_one_f32_ulp(e, np_eps64(keys, step, 0, D, seed))
    assert within_one_f32_ulp(e2, np_eps64(keys, step, 2, D, seed)) if sigma > 0 else not e2.any()
    u, cc = host_u(host, case, std, a, eps=e, deterministic=det)
    ok = np.isfinite(u)
    assert within_one_f32_ulp(std, np.exp(np_clamp_ls(case.log_std_in).astype(np.float64)))
    assert within_one_f32_ulp(a[ok], np.tanh(u[ok].astype(np.float64))) and within_one_f32_ulp(l[ok], np.log(cc[ok].astype(np.float64)))
    ref = host_rows(host, case, given=dict(eps=e, eps2=e2, std=std, tanh=a, corr=l), step=step, seed=seed, draw_index=D, sigma=sigma, deterministic=det, **kw)
    same_named(got, ref, ROWS_OUT, M)


@pytest.mark.parametrize("M", SIZES)
def test_rows_against_the_host_build(hd, host, M):
    seed, step, row0 = 0xABCDEF0123, 3, 17
    keys = row0 + np.arange(M)
    for in_dim in (IN_DIMS if M < CAP_M else IN_DIMS[:1]):
        case = RowsCase(M, in_dim, seed=M % 97)
        for sigma, det in ((0.05, 0), (0.0, 0), (0.3, 1)) if M < CAP_M else ((0.05, 0),):
            kw = dict(step=step, seed=seed, draw_index=5, row0=row0, sigma=sigma, deterministic=det)
            got = run_rows(hd, case, draw_base=9, **kw)
            check_rows(host, case, got, keys, step, 14, seed, sigma, det, row0=row0)       # D = draw_index + *draw_base
            assert (np.abs(got["action_env"]) <= 1).all()
    lean = ("action_env", "logp")
    same_named(run_rows(hd, case, want=lean, draw_base=9, **kw), got, lean)              # the optional outputs left out
    same_named(run_rows(hd, case, draw_base=9, **kw), got, ROWS_OUT)                     # the same call again: identical bits
    uni = run_rows(hd, case, want=UNIFORM_OUT, uniform=1, step=step, seed=seed, draw_index=14, row0=row0)
    want = np_uniform(keys, step, 14, seed)
    assert same_u32(uni["action"], want) and same_u32(uni["action_env"], want) and same_u32(uni["action_slot"], want) and same_u32(uni["obs_out"], case.obs)


def test_extreme_inputs_give_a_legal_executed_action(hd, host):
    M = 64
    c = RowsCase(M)
    c.mean_in[0], c.mean_in[1], c.mean_in[2], c.mean_in[3, 2] = np.nan, np.inf, -np.inf, np.nan
    c.log_std_in[4], c.log_std_in[5], c.log_std_in[6], c.log_std_in[7] = -20, 2, -np.inf, np.inf
    c.log_std_in[8], c.log_std_in[9, 1] = np.nan, np.nan
    for sigma in (0.0, 0.05):
        got = run_rows(hd, c, sigma=sigma, seed=4)
        env = got["action_env"]
        assert (np.abs(env) <= 1).all() and same_u32(env, got["action_slot"])
        assert (env[0] == -1).all() and env[3, 2] == -1 and np.isnan(got["action"][0]).all()
        assert sigma > 0 or ((env[1] == 1).all() and (env[2] == -1).all())
        check_rows(host, c, got, np.arange(M), 0, 0, 4, sigma)


# ---- 2. the backward pass ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_rows_grad_against_the_host_build(hd, host, M):
    rng = np.random.default_rng(M)
    case = RowsCase(M, seed=M % 89)
    fw = run_rows(hd, case, seed=6)
    inputs = dict(grad_action=rng.normal(size=(M, NU)).astype(f), grad_logp=rng.normal(size=M).astype(f), eps=fw["eps"], std=fw["std"], tanh=fw["tanh"],
                  log_std_in=case.log_std_in)
    dev = {k: E.Guarded(v) for k, v in inputs.items()}
    outs = guarded_outputs(dict(grad_mean=((M, NU), np.float32), grad_log_std=((M, NU), np.float32)))
    a = grad_args(M, lambda k: dev[k].ptr, {k: v.ptr for k, v in outs.items()})
    launch(hd, hd.lib.glgym_sac_rows_grad, a)
    for g in dev.values():
        g.read()
    got = read_outputs(outs, M, ("grad_mean", "grad_log_std"))
    same_named(got, host_grad(host, inputs), ("grad_mean", "grad_log_std"), M)
    launch(hd, hd.lib.glgym_sac_rows_grad, a)
    same_named(read_outputs(outs, M, ("grad_mean", "grad_log_std")), got, ("grad_mean", "grad_log_std"))


# ---- 3. sampling from the ring -------------------------------------------------------------------------------------------------------------
class DeviceBatch:
    def __init__(self, case, M):
        self.case, self.M = case, M
        self.inputs = {k: E.Guarded(v) for k, v in case.arrays().items()}
        self.outs = guarded_outputs(batch_output_shapes(M, case.in_dim))

    def args(self, head, n_valid, draw_base_ptr=None, **kw):
        return batch_args(self.case, self.M, head, n_valid, lambda k: self.inputs[k].ptr, {k: v.ptr for k, v in self.outs.items()}, draw_base=draw_base_ptr, **kw)

    def read(self, written):
        for g in self.inputs.values():
            g.read()
        return read_outputs(self.outs, self.M, written)


def run_batch(hd, case, M, head, n_valid, written=BATCH_OUT, draw_base=None, **kw):
    db = DeviceBatch(case, M)
    base = None if draw_base is None else E.Guarded(np.array([draw_base], dtype=np.uint64))
    launch(hd, hd.lib.glgym_sac_batch, db.args(head, n_valid, None if base is None else base.ptr, want_index="index_out" in written, **kw))
    return db.read(written)


@pytest.mark.parametrize("M", SIZES)
def test_batch_against_the_host_build(hd, host, M):
    kw = dict(seed=0xABCDEF0123, draw_index=5, draw_base=9)
    S, B, head, n_valid = 5, 37, 3, 4                            # the valid slots 3, 4, 0, 1 wrap; slot 2 holds the newest observation only
    for in_dim in (IN_DIMS if M < CAP_M else IN_DIMS[1:2]):
        case = RingCase(S, B, in_dim, seed=M % 97)
        got = run_batch(hd, case, M, head, n_valid, **kw)
        same_named(got, host_batch(host, case, M, head, n_valid, **kw), BATCH_OUT, M)
        row = got["index_out"]
        slot = row // B
        assert (((slot - head) % S) < n_valid).all() and same_u32(got["mb_next_obs"][:, 0], (((slot + 1) % S) * B + row % B).astype(f))
        if M <= 1023:
            assert np.array_equal(row, np_index(M, S, B, head, n_valid, 14, 0xABCDEF0123)[0])
    lean = tuple(k for k in BATCH_OUT if k != "index_out")
    same_named(run_batch(hd, case, M, head, n_valid, written=lean, **kw), got, lean)
    same_named(run_batch(hd, case, M, head, n_valid, **kw), got, BATCH_OUT)              # the same call again: identical bits
    if M == 257:
        for S2, B2, h2, n2 in ((3, 5, 0, 1), (3, 5, 2, 2), (4, 1, 3, 3), (2, 65537, 0, 1)):
            c2 = RingCase(S2, B2, 3)
            same_named(run_batch(hd, c2, M, h2, n2, seed=7), host_batch(host, c2, M, h2, n2, seed=7), BATCH_OUT, M)


# ---- 4. the loss stages ----------------------------------------------------------------------------------------------------------------------
class DeviceLoss:
    def __init__(self, case):
        from gl_gym_amd import _lib as L
        self.case = case
        self.inputs = {k: E.Guarded(v) for k, v in case.arrays().items()}
        self.outs = guarded_outputs(loss_output_shapes(case.M))
        self.ws = E.Guarded(shape=(L.SAC_LOSS_WS_BYTES // 8,), dtype=np.float64)

    def args(self, stage, **kw):
        return loss_args(self.case.M, stage, lambda k: self.inputs[k].ptr, {k: v.ptr for k, v in self.outs.items()}, self.ws.ptr, **kw)

    def read(self, written):
        for g in self.inputs.values():
            g.read()
        self.ws.read()
        return read_outputs(self.outs, loss_rows(self.case.M), written)


def run_loss(hd, case, stage, want=None, **kw):
    dl = DeviceLoss(case)
    launch(hd, hd.lib.glgym_sac_loss, dl.args(stage, want=want, **kw))
    return dl.read(LOSS_OUT[stage] if want is None else want)


@pytest.mark.parametrize("M", SIZES)
def test_loss_against_the_host_build(hd, host, M):
    case = LossCase(M, seed=M % 97)
    for stage in (0, 1):
        for cfg in (dict(), dict(gamma=0.5, target_entropy=-3.25)):
            got = run_loss(hd, case, stage, **cfg)
            same_named(got, host_loss(host, case, stage, **cfg), LOSS_OUT[stage], loss_rows(M))
        same_named(run_loss(hd, case, stage, **cfg), got, LOSS_OUT[stage])               # the same call again: identical bits
    lean = ("grad_q1", "grad_q2", "stats")
    same_named(run_loss(hd, case, 0, want=lean), host_loss(host, case, 0), lean, loss_rows(M))
    if M == 257:                                                                        # NaN follows fminf
        case.q1_next[5], case.q1_next[6], case.q2_next[6], case.logp[7], case.q1[8] = np.nan, np.nan, np.nan, np.nan, np.nan
        for stage in (0, 1):
            bad = run_loss(hd, case, stage)
            same_named(bad, host_loss(host, case, stage), LOSS_OUT[stage], loss_rows(M))
            assert np.isnan(bad["stats"][0])
        y = run_loss(hd, case, 0)["target_out"]
        assert np.isfinite(y[5]) and np.isnan(y[6]) and np.isnan(y[7])


# ---- 5. Polyak -------------------------------------------------------------------------------------------------------------------------------
def device_polyak(ts, ss):
    import torch
    dt, ds = [E.Guarded(t.base) for t in ts], [E.Guarded(s.base) for s in ss]       # the whole arrays; the 257-element pair starts at element 1
    off = [4 if len(t) == 257 else 0 for t in ts]
    table = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda:0")  # noqa: E731
    dst, src = table([g.ptr + o for g, o in zip(dt, off)]), table([g.ptr + o for g, o in zip(ds, off)])
    cnt = table([len(t) for t in ts])
    return dt, ds, dst, src, cnt


def test_polyak_against_numpy(hd):
    for tau, max_count in ((0.0135, 1025), (0.5, 7), (1.0, 0)):                          # max_count only sizes the grid
        ts, ss = polyak_tensors()
        assert [len(t) for t in ts] == POLYAK_COUNTS and ts[3].ctypes.data % 8 == 4
        dt, ds, dst, src, cnt = device_polyak(ts, ss)
        a = polyak_args(len(ts), dst.data_ptr(), src.data_ptr(), cnt.data_ptr(), max_count, tau)
        launch(hd, hd.lib.glgym_polyak, a)
        for t, s, g, gs in zip(ts, ss, dt, ds):
            now, n = g.read(), len(t)
            o = 1 if n == 257 else 0
            assert same_u32(now[o:o + n], np_polyak(t, s, tau)), (tau, n)
            assert same_u32(now[:o], t.base[:o]) and same_u32(now[o + n:], t.base[o + n:]) and same_u32(gs.read(), s.base)
        if tau == 0.5:                                                                   # twice: the update of the update
            launch(hd, hd.lib.glgym_polyak, a)
            assert same_u32(dt[4].read()[:1025], np_polyak(np_polyak(ts[4], ss[4], tau), ss[4], tau))


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
POINTERS = {"mean_in", "log_std_in", "obs", "obs_out", "action", "action_env", "action_slot", "logp", "eps", "eps2", "std", "tanh", "corr", "grad_action",
            "grad_logp", "grad_mean", "grad_log_std", "reward", "done", "mb_obs", "mb_next_obs", "mb_action", "mb_reward", "mb_done", "index_out",
            "q1", "q2", "q1_next", "q2_next", "alpha", "log_alpha", "grad_q1", "grad_q2", "target_out", "grad_log_alpha", "stats", "workspace"}


def test_refusals_launch_nothing(hd):
    """Every refusal returns GLGYM_EINVAL with its text and leaves every output as it was.  The argument blocks point at real device buffers
    throughout: a table entry's k-th megabyte stands for the k-th buffer of the block."""
    L = hd.L

    def remap(path, value, order):
        if path in POINTERS and isinstance(value, int):
            k, rest = divmod(value - P_, MB_)
            return order[k].ptr + rest
        return value

    def sweep(name, make, refusals, order, read_nothing, read_all):
        fn = getattr(hd.lib, name)
        for path, value, word in refusals:
            a = make()
            set_path(a, path, remap(path, value, order))
            hd.sync()
            assert fn(hd.h, C.byref(a), hd.stream()) == L.EINVAL, (name, path, value)
            assert word in hd.lib.glgym_last_error() and name.encode() in hd.lib.glgym_last_error(), (path, hd.error())
        hd.sync()
        read_nothing()
        launch(hd, fn, make())                                   # ... and the block they were derived from is good
        read_all()

    dr = DeviceRows(RowsCase(130, 23))
    sweep("glgym_sac_rows", lambda: dr.args(sigma=0.05), ROWS_REFUSALS,
          [dr.inputs[k] for k in ("mean_in", "log_std_in", "obs")] + [dr.outs[k] for k in ROWS_OUT], lambda: dr.read(()), lambda: dr.read(ROWS_OUT))
    rng = np.random.default_rng(1)
    gi = {k: E.Guarded(rng.normal(size=(130,) if k == "grad_logp" else (130, NU)).astype(f)) for k in ("grad_action", "grad_logp", "eps", "std", "tanh", "log_std_in")}
    go = guarded_outputs(dict(grad_mean=((130, NU), np.float32), grad_log_std=((130, NU), np.float32)))
    sweep("glgym_sac_rows_grad", lambda: grad_args(130, lambda k: gi[k].ptr, {k: v.ptr for k, v in go.items()}), GRAD_REFUSALS,
          list(gi.values()) + list(go.values()), lambda: read_outputs(go, 130, ()), lambda: read_outputs(go, 130, tuple(go)))
    db = DeviceBatch(RingCase(4, 130, 23), 200)
    sweep("glgym_sac_batch", lambda: db.args(1, 3), BATCH_REFUSALS, [db.inputs[k] for k in ("obs", "action", "reward", "done")] + [db.outs[k] for k in BATCH_OUT],
          lambda: db.read(()), lambda: db.read(BATCH_OUT))
    for stage in (0, 1):
        dl = DeviceLoss(LossCase(130, seed=4))
        order = [dl.inputs[k] for k in ("q1", "q2", "logp", "q1_next", "q2_next", "reward", "done", "alpha", "log_alpha")] + \
                [dl.outs[k] for k in ALL_LOSS_OUT] + [dl.ws]
        sweep("glgym_sac_loss", lambda: dl.args(stage, want=ALL_LOSS_OUT), LOSS_REFUSALS[stage], order,
              lambda: (dl.read(()), dl.ws.untouched()), lambda: dl.read(LOSS_OUT[stage]))


# ---- 7. graph capture ----------------------------------------------------------------------------------------------------------------------
def test_every_entry_point_in_one_captured_graph(hd, host):
    """The five calls captured once; the replay after the device draw word moved on gives the next sample and the host build's results."""
    import torch
    M, S, B, in_dim, seed = 200, 5, 37, 23, 11
    rc, ring, lc = RowsCase(M, in_dim, seed=2), RingCase(S, B, in_dim, seed=3), LossCase(M, seed=5)
    dr, db, dl = DeviceRows(rc), DeviceBatch(ring, M), DeviceLoss(lc)
    rng = np.random.default_rng(3)
    up = {k: E.Guarded(rng.normal(size=s).astype(f)) for k, s in (("grad_action", (M, NU)), ("grad_logp", (M,)))}
    go = guarded_outputs(dict(grad_mean=((M, NU), np.float32), grad_log_std=((M, NU), np.float32)))
    ts, ss = polyak_tensors()
    dt, ds, dst, src, cnt = device_polyak(ts, ss)
    base_t = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    a_rows = dr.args(draw_base_ptr=base_t.data_ptr(), seed=seed, draw_index=3, step=1, sigma=0.05)
    saved = dict(eps=dr.outs["eps"], std=dr.outs["std"], tanh=dr.outs["tanh"], log_std_in=dr.inputs["log_std_in"], **up)
    a_grad = grad_args(M, lambda k: saved[k].ptr, {k: v.ptr for k, v in go.items()})
    a_batch = db.args(3, 4, base_t.data_ptr(), seed=seed, draw_index=3)
    a_loss = loss_args(M, 0, lambda k: {"reward": db.outs["mb_reward"], "done": db.outs["mb_done"], "logp": dr.outs["logp"]}.get(k, dl.inputs[k]).ptr,
                       {k: v.ptr for k, v in dl.outs.items()}, dl.ws.ptr)
    a_pol = polyak_args(len(ts), dst.data_ptr(), src.data_ptr(), cnt.data_ptr(), 1025, 0.25)

    def every():
        for fn, a in ((hd.lib.glgym_sac_rows, a_rows), (hd.lib.glgym_sac_rows_grad, a_grad), (hd.lib.glgym_sac_batch, a_batch),
                      (hd.lib.glgym_sac_loss, a_loss), (hd.lib.glgym_polyak, a_pol)):
            assert fn(hd.h, C.byref(a), hd.stream()) == 0, hd.error()

    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        every()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        every()
    hd.sync()
    first_index = db.read(BATCH_OUT)["index_out"].copy()
    first_eps = dr.read(ROWS_OUT)["eps"].copy()
    assert np.array_equal(first_index, np_index(M, S, B, 3, 4, 3, seed)[0])               # D = 3 + 0
    base_t.fill_(5)                                              # the device word moves on between replays
    for o in list(dr.outs.values()) + list(db.outs.values()) + list(dl.outs.values()) + list(go.values()):
        o.t[E.GUARD:E.GUARD + o.n] = 0xFF
    graph.replay()
    hd.sync()
    got_r, got_b, got_l = dr.read(ROWS_OUT), db.read(BATCH_OUT), dl.read(LOSS_OUT[0])
    assert np.array_equal(got_b["index_out"], np_index(M, S, B, 3, 4, 8, seed)[0]) and not np.array_equal(got_b["index_out"], first_index)
    same_named(got_b, host_batch(host, ring, M, 3, 4, seed=seed, draw_index=3, draw_base=5), BATCH_OUT, M)
    assert not (got_r["eps"] == first_eps).any()
    check_rows(host, rc, got_r, np.arange(M), 1, 8, seed, 0.05)
    inputs = dict(grad_action=up["grad_action"].read(), grad_logp=up["grad_logp"].read(), eps=got_r["eps"], std=got_r["std"], tanh=got_r["tanh"],
                  log_std_in=rc.log_std_in)
    same_named(read_outputs(go, M, tuple(go)), host_grad(host, inputs), tuple(go), M)
    lc.reward, lc.done, lc.logp = got_b["mb_reward"].copy(), got_b["mb_done"].copy(), got_r["logp"].copy()
    same_named(got_l, host_loss(host, lc, 0), LOSS_OUT[0], loss_rows(M))
    # the eager run and the replay (the capture itself runs nothing): the targets were updated twice
    assert same_u32(dt[4].read()[:1025], np_polyak(np_polyak(ts[4], ss[4], 0.25), ss[4], 0.25))


# ---- 8. squashed_sample through autograd ---------------------------------------------------------------------------------------------------
def test_squashed_sample_gradients_against_the_host_build(hd, host):
    import torch
    from gl_gym_amd import squashed_sample
    M = 257
    case = RowsCase(M, seed=8)
    dev = "cuda:0"
    mean = torch.as_tensor(case.mean_in, device=dev).requires_grad_()
    log_std = torch.as_tensor(case.log_std_in, device=dev).requires_grad_()
    ga, gl = torch.randn(M, NU, device=dev), torch.randn(M, device=dev)
    action, logp = squashed_sample(mean, log_std, handle=hd.h, seed=21, step=2, draw_index=4, row0=100)
    ((action * ga).sum() + (logp * gl).sum()).backward()
    hd.sync()
    fw = run_rows(hd, case, seed=21, step=2, draw_index=4, row0=100)
    assert same_u32(action.detach().cpu().numpy(), fw["action"]) and same_u32(logp.detach().cpu().numpy(), fw["logp"])
    want = host_grad(host, dict(grad_action=ga.cpu().numpy(), grad_logp=gl.cpu().numpy(), eps=fw["eps"], std=fw["std"], tanh=fw["tanh"], log_std_in=case.log_std_in))
    assert same_u32(mean.grad.cpu().numpy(), want["grad_mean"][:M]) and same_u32(log_std.grad.cpu().numpy(), want["grad_log_std"][:M])


# ---- 9. ReplayCollector and SAC ------------------------------------------------------------------------------------------------------------
def elementwise_nets(device, D):
    """An actor and two critics with parameters but without a reduction over a GEMM's k, so that two evaluations agree bit for bit."""
    import torch

    class Actor(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Parameter(torch.full((NU,), 1e-2)), torch.nn.Parameter(torch.zeros(NU))
            self.c = torch.nn.Parameter(torch.full((NU,), -1.0))

        def forward(self, obs):
            return torch.tanh(obs[:, :NU] * self.a + self.b) * 1.5, self.c + 0.1 * torch.tanh(obs[:, NU:2 * NU] * self.a)

    class Critic(torch.nn.Module):
        def __init__(self, k):
            super().__init__()
            self.w = torch.nn.Parameter(torch.full((NU,), 0.1 * (k + 1)))
            self.v = torch.nn.Parameter(torch.full((NU,), 0.01))
            self.b = torch.nn.Parameter(torch.zeros(1))

        def forward(self, obs, action):
            return (action * self.w).sum(-1) + (torch.tanh(obs[:, :NU]) * self.v).sum(-1) + self.b

    return Actor().to(device), Critic(0).to(device), Critic(1).to(device)


@pytest.mark.parametrize("wrapped", [False, True], ids=["bare", "stack"])
def test_collector_fills_the_ring_as_a_numpy_replay(wrapped):
    """5 steps into a ring of 4 slots (it wraps), 64 environments: the ring equals a replay of the recorded observations, executed actions,
    rewards and dones, and head / n_valid name the slots whose successor is written."""
    import torch
    from gl_gym_amd import ReplayCollector
    B, S = 64, 4
    env = stack_of("float32", wrapped, B)
    actor = elementwise_nets(env.device, env.obs_dim)[0]
    col = ReplayCollector(env, actor, S, seed=3, action_noise_sigma=0.05)
    rec = dict(obs=[], act=[], rew=[], done=[])
    real_step = env.step_tensor

    def recording_step(actions_t, *a, **k):
        rec["act"].append(actions_t.cpu().numpy().copy())
        out = real_step(actions_t, *a, **k)
        rec["obs"].append(out[0].cpu().numpy().copy())
        rec["rew"].append(out[1].float().cpu().numpy().copy())
        rec["done"].append(out[2].cpu().numpy().copy())
        return out

    env.step_tensor = recording_step
    obs0 = col.reset(seed=5).cpu().numpy().copy()
    col.collect(2, explore="uniform")
    assert (col.pos, col.filled, col.head, col.n_valid) == (2, 2, 0, 2)
    col.collect(3)
    torch.cuda.synchronize()
    assert (col.pos, col.filled, col.head, col.n_valid, col.num_timesteps) == (1, 4, 2, 3, 5 * B)
    obs_seq = [obs0] + rec["obs"]                                 # obs_seq[k]: the observation step k acted on
    want = {k: np.zeros(tuple(v.shape), dtype=v.cpu().numpy().dtype) for k, v in col.ring.items()}
    for k in range(5):
        s = k % S
        want["observations"][s], want["actions"][s], want["rewards"][s], want["dones"][s] = obs_seq[k], rec["act"][k], rec["rew"][k], rec["done"][k]
    want["observations"][5 % S] = obs_seq[5]
    for k, v in col.ring.items():
        assert np.array_equal(E.bits(v.cpu().numpy()), E.bits(want[k])), k
    acts = np.stack(rec["act"])
    assert (np.abs(acts) <= 1).all() and np.isfinite(acts).all()
    assert same_u32(acts[0], np_uniform(np.arange(B), 0, 0, 5)) and same_u32(acts[1], np_uniform(np.arange(B), 1, 0, 5))   # keyed by (reset's seed, env, step)
    env.close()


def make_sac(env, seed=21, **kw):
    import torch
    from gl_gym_amd import SAC, ReplayCollector
    torch.manual_seed(0)
    actor, c1, c2 = elementwise_nets(env.device, env.obs_dim)
    col = ReplayCollector(env, actor, 4, seed=3, action_noise_sigma=0.05)
    col.reset(seed=5)
    col.collect(5, explore="uniform")
    a_opt = torch.optim.Adam(actor.parameters(), lr=1e-2)
    c_opt = torch.optim.Adam(list(c1.parameters()) + list(c2.parameters()), lr=1e-2)
    return SAC(col, c1, c2, a_opt, c_opt, batch_size=200, gamma=0.9631, tau=0.0135, seed=seed, **kw), actor, c1, c2


def test_update_mechanics_and_determinism():
    import torch
    from gl_gym_amd import SAC
    B = 64
    runs = []
    for _ in range(2):
        env = stack_of("float32", False, B)
        sac, actor, c1, c2 = make_sac(env)
        ring_before = {k: v.clone() for k, v in sac.collector.ring.items()}
        t0 = [p.detach().clone() for p in list(sac.target1.parameters()) + list(sac.target2.parameters())]
        la0 = float(sac.log_alpha.detach())
        stats = sac.update(2)
        torch.cuda.synchronize()
        st = stats.cpu().numpy()
        assert stats.shape == (2, 8) and stats.dtype == torch.float64 and np.isfinite(st).all() and (st[:, 7] == 200).all()
        assert int(sac.draw_t) == 2 and sac.n_updates == 2 and len(SAC.STATS) == 8
        for k, v in sac.collector.ring.items():
            assert torch.equal(v, ring_before[k]), k
        # log_alpha moves against the sign of mean(logp) + target_entropy: its gradient is -(that mean)
        first = sac.actor_stats_t[0].cpu().numpy()
        assert first[2] != 0 and np.sign(float(sac.log_alpha.detach()) - la0) == np.sign(first[2]) * -1 and abs(first[2] + (first[3] - 6.0)) < 1e-5
        # the target critics moved by exactly tau: two Polyak updates from the critics' values after each critic step are not at hand, so
        # redo the last one -- t2 = (1 - tau) t1 + tau s2 -- from a third update whose inputs are
        t1 = [p.detach().clone() for p in list(sac.target1.parameters()) + list(sac.target2.parameters())]
        sac.update(1)
        torch.cuda.synchronize()
        s = [p.detach().cpu().numpy() for p in list(c1.parameters()) + list(c2.parameters())]
        t2 = [p.detach().cpu().numpy() for p in list(sac.target1.parameters()) + list(sac.target2.parameters())]
        for a, b, c, d in zip(t0, t1, t2, s):
            assert same_u32(c, np_polyak(b.cpu().numpy(), d, 0.0135)) and not torch.equal(a, b)
        runs.append([p.detach().cpu().numpy().copy() for m in (actor, c1, c2, sac.target1, sac.target2) for p in m.parameters()] +
                    [sac.log_alpha.detach().cpu().numpy().copy(), st])
        env.close()
    for a, b in zip(*runs):                                       # two runs from the same seed and state: identical parameters
        assert np.array_equal(E.bits(a), E.bits(b))


def test_critic_loss_falls_on_a_fixed_batch():
    import torch
    env = stack_of("float32", False, 64)
    sac, actor, c1, c2 = make_sac(env)
    sac.batch()
    sac.refresh_alpha()
    for k in range(20):                                           # critic-only steps: the same batch, the same noise, the same targets
        sac.critic_step(sac.critic_stats_t[k])
    torch.cuda.synchronize()
    losses = sac.critic_stats_t[:20, 0].cpu().numpy()
    print("critic loss over 20 critic-only steps:", " ".join(f"{v:.5f}" for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    env.close()
