"""The PPO update on the GPU: glgym_ppo_batch, glgym_ppo_loss (include/glgym.h), gl_gym_amd.ppo.ppo_loss and gl_gym_amd.ppo.PPO.

What can be exact is compared bit for bit with the host instantiation of csrc/gl_ppo.hpp (tests/ppohost/ppohost.cpp): the permutation, the
gathered rows, the advantage statistics, and every output and sum of the loss.  The one thing that is not: the ratio is exp in double by
the device's libm, which is not the host's -- ratio_out is compared with np.exp in double within one float32 ulp, and everything that
follows from it is compared exactly GIVEN the device's own ratio (the host build takes it as an input).  Every output buffer has guard rows
behind its last row and guard bytes around it (0xFF); an optional output that is not asked for and every output of a refused call must
come back untouched.

Bound of the autograd comparison: each side is within 1e-4 of the largest |gradient| of the exact gradient (tests/test_ppo_host.py), so the
two float32 chains are within twice that of each other."""
import ctypes as C

import numpy as np
import pytest

import envlayer_inputs as E
from test_gpu_collect import stack_of
from test_ppo_host import (BATCH_PAIRS, BATCH_REFUSALS, BLOCK, GUARD, LOSS_CONFIGS, LOSS_OUT, LOSS_REFUSALS, MAX_BLOCKS, MB_, NU, P_, BatchCase,
                           LossCase, batch_args, batch_output_shapes, build_host, host_batch, host_loss, loss_args, loss_output_shapes,
                           np_adv_stats, np_perm, np_ratio64, same_f64, same_u32, set_path, within_one_f32_ulp)

pytestmark = pytest.mark.gpu
IN_DIMS = [1, 23, 24]
CAP_M = BLOCK * MAX_BLOCKS + 77                               # just past the grid's cap: the first 77 lanes of block 0 take a second row
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, CAP_M]


@pytest.fixture(scope="module")
def hd():
    h = E.Handle(False)
    yield h
    h.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("ppohost_gpu") / "libppohost.so")


def guarded_outputs(shapes):
    return {k: E.Guarded(shape=(s[0] + GUARD,) + tuple(s[1:]), dtype=dt) for k, (s, dt) in shapes.items()}


def read_outputs(outs, n_rows, written):
    """{name: rows < n} of the outputs in `written`; asserts every guard, and that the other outputs were not touched."""
    got = {}
    for k, g in outs.items():
        v = g.read()
        if k in written:
            n = n_rows[k]
            assert np.all(v[n:].view(np.uint8) == 0xFF), f"a guard row of {k} was written"
            got[k] = v[:n]
        else:
            assert np.all(v.view(np.uint8) == 0xFF), f"{k} was written"
    return got


class DeviceLoss:
    """The arrays of a LossCase on the device, each between guard bytes, guarded outputs and a workspace of exactly the stated size."""

    def __init__(self, case):
        from gl_gym_amd import _lib as L
        self.case = case
        self.inputs = {k: E.Guarded(v) for k, v in case.arrays().items()}
        self.outs = guarded_outputs(loss_output_shapes(case.M))
        self.ws = E.Guarded(shape=(L.PPO_LOSS_WS_BYTES // 8,), dtype=np.float64)

    def args(self, want_extra=True, **cfg):
        out = {k: v.ptr for k, v in self.outs.items() if want_extra or k not in ("ratio_out", "logp_out")}
        return loss_args(self.case.M, lambda k: self.inputs[k].ptr, out, self.ws.ptr, **cfg)

    def read(self, written=LOSS_OUT):
        M = self.case.M
        for g in self.inputs.values():
            g.read()
        self.ws.read()
        return read_outputs(self.outs, {k: {"grad_log_std": NU, "stats": 8}.get(k, M) for k in self.outs}, written)


def run_loss(hd, case, written=LOSS_OUT, **cfg):
    dl = DeviceLoss(case)
    a = dl.args(want_extra="ratio_out" in written, **cfg)
    hd.sync()
    rc = hd.lib.glgym_ppo_loss(hd.h, C.byref(a), hd.stream())
    hd.sync()
    assert rc == 0, (rc, hd.error())
    return dl.read(written)


def same_named(got, want, names, n_rows=None):
    for k in names:
        w = want[k] if n_rows is None else want[k][:n_rows.get(k, len(want[k]))]
        assert (same_f64 if got[k].dtype == np.float64 else same_u32 if got[k].dtype == np.float32 else np.array_equal)(got[k], w), k


def host_rows(outs, M):
    return {k: v[:{"grad_log_std": NU, "stats": 8, "adv_stats": 2}.get(k, M)] for k, v in outs.items()}


# ---- 1. the loss kernel against the host build -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", SIZES)
def test_loss_against_the_host_build(hd, host, M):
    case = LossCase(M, seed=M % 97)
    for cfg in (LOSS_CONFIGS if M < CAP_M else LOSS_CONFIGS[:1] + LOSS_CONFIGS[-1:]):
        if M == 1 and cfg.get("normalize", True):
            continue
        got = run_loss(hd, case, **cfg)
        assert within_one_f32_ulp(got["ratio_out"], np_ratio64(case)), cfg
        same_named(got, host_rows(host_loss(host, case, ratio_in=got["ratio_out"], **cfg), M), LOSS_OUT)
    lean = tuple(k for k in LOSS_OUT if k not in ("ratio_out", "logp_out"))
    cfg = LOSS_CONFIGS[-1]
    same_named(run_loss(hd, case, written=lean, **cfg), got, lean)                        # the optional outputs left out
    if M == 257:                                                                        # a NaN stays in its row
        case.mean[70, 2] = np.nan
        bad = run_loss(hd, case, **cfg)
        same_named(bad, host_rows(host_loss(host, case, ratio_in=bad["ratio_out"], **cfg), M), LOSS_OUT)
        others = np.arange(M) != 70
        assert np.isnan(bad["grad_mean"][70, 2]) and np.isnan(bad["stats"][4]) and same_u32(bad["grad_mean"][others], got["grad_mean"][others])


# ---- 2. the batch kernel against the host build ----------------------------------------------------------------------------------------
class DeviceBatch:
    def __init__(self, case, M):
        from gl_gym_amd import _lib as L
        self.case, self.M = case, M
        self.inputs = {k: E.Guarded(v) for k, v in case.arrays().items()}
        self.outs = guarded_outputs(batch_output_shapes(M, case.in_dim))
        self.ws = E.Guarded(shape=(L.PPO_BATCH_WS_BYTES // 8,), dtype=np.float64)

    def args(self, offset, draw_base_ptr=None, **kw):
        return batch_args(self.case, self.M, offset, lambda k: self.inputs[k].ptr, {k: v.ptr for k, v in self.outs.items()}, self.ws.ptr,
                          draw_base=draw_base_ptr, **kw)

    def read(self, written):
        for g in self.inputs.values():
            g.read()
        self.ws.read()
        return read_outputs(self.outs, {k: 2 if k == "adv_stats" else self.M for k in self.outs}, written)


ALL_BATCH = tuple(BATCH_PAIRS) + ("mb_index", "adv_stats")


def run_batch(hd, case, M, offset, written=ALL_BATCH, draw_base=None, **kw):
    db = DeviceBatch(case, M)
    base = None if draw_base is None else E.Guarded(np.array([draw_base], dtype=np.uint64))
    a = db.args(offset, None if base is None else base.ptr, want_index="mb_index" in written, want_stats="adv_stats" in written, **kw)
    hd.sync()
    rc = hd.lib.glgym_ppo_batch(hd.h, C.byref(a), hd.stream())
    hd.sync()
    assert rc == 0, (rc, hd.error())
    return db.read(written)


@pytest.mark.parametrize("M", SIZES)
def test_batch_against_the_host_build(hd, host, M):
    kw = dict(seed=0xABCDEF0123, draw_index=5, draw_base=9)
    offset = 37
    for in_dim in IN_DIMS:
        case = BatchCase(M + 300, in_dim, seed=M % 97)
        written = ALL_BATCH if M > 1 else tuple(k for k in ALL_BATCH if k != "adv_stats")
        got = run_batch(hd, case, M, offset, written=written, **kw)
        ref = host_rows(host_batch(host, case, M, offset, want_stats=M > 1, **kw), M)
        same_named(got, ref, written)
        idx = np_perm(case.N, 14, 0xABCDEF0123)[offset:offset + M]                      # D = draw_index + *draw_base
        assert np.array_equal(got["mb_index"], idx) and same_u32(got["mb_obs"], case.obs[idx])
        if M > 1:
            assert same_f64(got["adv_stats"], np_adv_stats(got["mb_adv"]))
    lean = tuple(BATCH_PAIRS)
    same_named(run_batch(hd, case, M, offset, written=lean, **kw), got, lean)            # the optional outputs left out
    if M == 257:                                                                        # the permutation does not depend on the split
        whole = run_batch(hd, case, case.N, 0, **kw)["mb_index"]
        assert np.array_equal(whole[offset:offset + M], got["mb_index"]) and np.array_equal(np.sort(whole), np.arange(case.N))
        assert np.array_equal(run_batch(hd, case, M, offset, seed=0xABCDEF0123, draw_index=14)["mb_index"], got["mb_index"])   # draw_base NULL: 0
        assert not np.array_equal(run_batch(hd, case, M, offset, seed=0xABCDEF0123, draw_index=15)["mb_index"], got["mb_index"])


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------
POINTERS = {"obs", "action", "logp", "advantage", "returns", "value", "mb_obs", "mb_action", "mb_logp", "mb_adv", "mb_ret", "mb_value", "mb_index",
            "adv_stats", "workspace", "mean", "log_std", "inv_std", "grad_mean", "grad_value", "grad_log_std", "stats", "ratio_out", "logp_out"}


def test_refusals_launch_nothing(hd):
    """Every refusal returns GLGYM_EINVAL with its text and leaves every output as it was.  The argument blocks point at real device buffers
    throughout: a table entry's k-th megabyte stands for the k-th buffer of the block."""
    L = hd.L
    case = BatchCase(520, 23)
    db = DeviceBatch(case, 130)
    order = [db.inputs[k] for k in ("obs", "action", "logp", "advantage", "returns", "value")] + \
            [db.outs[k] for k in ("mb_obs", "mb_action", "mb_logp", "mb_adv", "mb_ret", "mb_value", "mb_index", "adv_stats")] + [db.ws]

    def remap(path, value, order):
        if path in POINTERS and isinstance(value, int):
            k, rest = divmod(value - P_, MB_)
            return order[k].ptr + rest
        return value

    for path, value, word in BATCH_REFUSALS:
        a = db.args(260, seed=1)
        set_path(a, path, remap(path, value, order))
        hd.sync()
        assert hd.lib.glgym_ppo_batch(hd.h, C.byref(a), hd.stream()) == L.EINVAL, (path, value)
        assert word in hd.lib.glgym_last_error() and b"glgym_ppo_batch" in hd.lib.glgym_last_error(), (path, hd.error())
    hd.sync()
    db.read(())                                                  # nothing was written, no guard either
    assert db.ws.untouched()
    rc = hd.lib.glgym_ppo_batch(hd.h, C.byref(db.args(260, seed=1)), hd.stream())          # ... and the block they were derived from is good
    hd.sync()
    assert rc == 0, hd.error()
    db.read(ALL_BATCH)

    lc = LossCase(130, seed=4)
    dl = DeviceLoss(lc)
    order = [dl.inputs[k] for k in ("mean", "value", "log_std", "inv_std", "mb_action", "mb_logp", "mb_adv", "mb_ret", "mb_value", "adv_stats")] + \
            [dl.outs[k] for k in ("grad_mean", "grad_value", "grad_log_std", "stats", "ratio_out", "logp_out")] + [dl.ws]
    for path, value, word in LOSS_REFUSALS:
        a = dl.args(clip_range_vf=0.1)
        set_path(a, path, remap(path, value, order))
        hd.sync()
        assert hd.lib.glgym_ppo_loss(hd.h, C.byref(a), hd.stream()) == L.EINVAL, (path, value)
        assert word in hd.lib.glgym_last_error() and b"glgym_ppo_loss" in hd.lib.glgym_last_error(), (path, hd.error())
    hd.sync()
    dl.read(())
    assert dl.ws.untouched()
    rc = hd.lib.glgym_ppo_loss(hd.h, C.byref(dl.args(clip_range_vf=0.1)), hd.stream())
    hd.sync()
    assert rc == 0, hd.error()
    dl.read(LOSS_OUT)


# ---- 4. graph capture --------------------------------------------------------------------------------------------------------------------
def test_both_calls_in_one_captured_graph(hd, host):
    """glgym_ppo_batch into a minibatch and glgym_ppo_loss on it, captured once; the replay after the device draw word moved on gives the
    next permutation's minibatch and the host build's results for it."""
    import torch
    N, M, offset, in_dim, seed = 520, 200, 320, 23, 11
    bc = BatchCase(N, in_dim, seed=2)
    lc = LossCase(M, seed=5)                                    # its mean, value, log_std, inv_std are the heads' outputs; the rest is gathered
    db = DeviceBatch(bc, M)
    dl = DeviceLoss(lc)
    base_t = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    a = db.args(offset, base_t.data_ptr(), seed=seed, draw_index=3)
    gathered = dict(mb_action="mb_action", mb_logp="mb_logp", mb_adv="mb_adv", mb_ret="mb_ret", mb_value="mb_value", adv_stats="adv_stats")
    cfg = dict(clip_range_vf=0.15, ent_coef=0.01)
    g = loss_args(M, lambda k: db.outs[gathered[k]].ptr if k in gathered else dl.inputs[k].ptr, {k: v.ptr for k, v in dl.outs.items()}, dl.ws.ptr, **cfg)

    def both():
        assert hd.lib.glgym_ppo_batch(hd.h, C.byref(a), hd.stream()) == 0, hd.error()
        assert hd.lib.glgym_ppo_loss(hd.h, C.byref(g), hd.stream()) == 0, hd.error()

    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    hd.sync()
    first_index = db.read(ALL_BATCH)["mb_index"].copy()         # D = 3 + 0
    assert np.array_equal(first_index, np_perm(N, 3, seed)[offset:offset + M])
    base_t.fill_(5)                                              # the device word moves on between replays
    for o in list(db.outs.values()) + list(dl.outs.values()):
        o.t[E.GUARD:E.GUARD + o.n] = 0xFF
    graph.replay()
    hd.sync()
    got_b, got_l = db.read(ALL_BATCH), dl.read(LOSS_OUT)
    assert np.array_equal(got_b["mb_index"], np_perm(N, 8, seed)[offset:offset + M]) and not np.array_equal(got_b["mb_index"], first_index)
    same_named(got_b, host_rows(host_batch(host, bc, M, offset, seed=seed, draw_index=3, draw_base=5), M), ALL_BATCH)
    for k, src in gathered.items():                              # the host's loss on what the replay gathered
        setattr(lc, k, got_b[src].copy())
    assert within_one_f32_ulp(got_l["ratio_out"], np_ratio64(lc))
    same_named(got_l, host_rows(host_loss(host, lc, ratio_in=got_l["ratio_out"], **cfg), M), LOSS_OUT)


# ---- 5. ppo_loss through autograd ------------------------------------------------------------------------------------------------------
def test_ppo_loss_gradients_against_the_torch_loss_chain(hd):
    """Tanh nets 23-64-64-6 and 23-64-1 at M = 257: the parameter gradients behind ppo_loss against those of the float32 torch chain of
    examples/collect_rollouts.py (plus its entropy term) on the same minibatch."""
    import torch
    from gl_gym_amd import ppo_loss
    M, D, H, clip, vf_coef, ent_coef = 257, 23, 64, 0.2, 0.5, 0.01
    dev = "cuda:0"
    torch.manual_seed(0)
    lin, act = torch.nn.Linear, torch.nn.Tanh
    pi = torch.nn.Sequential(lin(D, H), act(), lin(H, H), act(), lin(H, 6)).to(dev)
    vf = torch.nn.Sequential(lin(D, H), act(), lin(H, 1)).to(dev)
    log_std = torch.nn.Parameter(torch.full((6,), -0.3, device=dev))
    params = list(pi.parameters()) + list(vf.parameters()) + [log_std]
    rng = np.random.default_rng(7)
    T = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float32), device=dev)  # noqa: E731
    obs = T(rng.normal(size=(M, D)))
    with torch.no_grad():
        mean0 = pi(obs)
        actions = (mean0 + log_std.exp() * T(rng.normal(size=(M, 6)))).contiguous()
        old_logp = ((-0.5 * ((actions - mean0) / log_std.exp()).pow(2) - log_std - 0.9189385).sum(-1) + T(rng.normal(size=M) * 0.3)).contiguous()
    adv, ret = T(rng.normal(size=M) * 2 + 0.3), T(rng.normal(size=M))
    adv_stats = torch.stack([adv.double().mean(), adv.double().std()])
    mb = dict(actions=actions, log_probs=old_logp, advantages=adv, returns=ret, values=None, adv_stats=adv_stats)

    loss = ppo_loss(pi(obs), vf(obs), log_std, mb, handle=hd.h, clip_range=clip, vf_coef=vf_coef, ent_coef=ent_coef)
    for p in params:
        p.grad = None
    loss.backward()
    mine = [p.grad.detach().cpu().numpy().astype(np.float64).copy() for p in params]
    loss_mine = float(loss.detach())

    for p in params:
        p.grad = None
    mean, value = pi(obs), vf(obs).squeeze(-1)
    noise = (actions - mean) / log_std.exp()
    logp = (-0.5 * noise.pow(2) - log_std - 0.9189385).sum(-1)
    ratio = (logp - old_logp).exp()
    a = (adv - adv.mean()) / (adv.std() + 1e-8)
    ref = -torch.min(ratio * a, ratio.clamp(1 - clip, 1 + clip) * a).mean() + vf_coef * (ret - value).pow(2).mean() \
        - ent_coef * (0.5 + 0.9189385 + log_std).sum()
    ref.backward()
    r = ratio.detach().cpu().numpy()
    assert ((r < 1 - clip).mean() > 0.05) and ((r > 1 + clip).mean() > 0.05)              # both clip bounds are at work
    ref_loss = float(ref.detach())
    assert abs(loss_mine - ref_loss) <= 2e-4 * max(1.0, abs(ref_loss))
    for p, g in zip(params, mine):
        want = p.grad.detach().cpu().numpy().astype(np.float64)
        err, big = np.abs(g - want).max(), np.abs(want).max()
        print(f"parameter {tuple(p.shape)}: max |difference| = {err:.3e}, largest |gradient| = {big:.3e}")
        assert big > 0 and err <= 2e-4 * big, tuple(p.shape)


# ---- 6. PPO.update() on a collector ----------------------------------------------------------------------------------------------------
def parametrised_elementwise_heads(device):
    """Heads with parameters but without a reduction, so that two evaluations of the same observations agree bit for bit whatever GEMM torch
    would pick: six means and a value as elementwise functions of observation columns."""
    import torch

    class Pi(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Parameter(torch.full((NU,), 1e-3)), torch.nn.Parameter(torch.zeros(NU))

        def forward(self, obs):
            return torch.tanh(obs[:, :NU] * self.a + self.b) * 1.5

    class Vf(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Parameter(torch.full((1,), 1e-3)), torch.nn.Parameter(torch.zeros(1))

        def forward(self, obs):
            return torch.tanh(obs[:, NU:NU + 1] * self.a + self.b)

    return Pi().to(device), Vf().to(device), torch.nn.Parameter(torch.full((NU,), -0.5, device=device))


@pytest.mark.parametrize("wrapped", [False, True], ids=["bare", "stack"])
def test_update_on_a_collector(hd, host, wrapped):
    import torch
    from gl_gym_amd import PPO, RolloutCollector, TorchHeads
    T, B, M, seed = 4, 130, 200, 21
    env = stack_of("float32", wrapped, B)
    pi, vf, log_std = parametrised_elementwise_heads(env.device)
    params = list(pi.parameters()) + list(vf.parameters()) + [log_std]
    col = RolloutCollector(env, T, TorchHeads(pi, vf, log_std), gamma=0.9631, gae_lambda=0.95, seed=3)
    col.reset(seed=5)
    col.collect()
    opt = torch.optim.Adam(params, lr=1e-2)
    ppo = PPO(col, opt, n_epochs=2, batch_size=M, clip_range=0.2, ent_coef=0.01, vf_coef=0.5, seed=seed)
    assert ppo.sizes == [200, 200, 120] and ppo.stats_t.shape == (2, 3, 8) and ppo.stats_t.dtype == torch.float64
    torch.cuda.synchronize()
    before = {k: v.cpu().numpy().copy() for k, v in col.buffer.items()}
    p0 = [p.detach().cpu().numpy().copy() for p in params]

    # the first minibatch, restated: permutation of draw 0, the heads on the gathered observations, the host build's loss
    N = T * B
    idx = np_perm(N, 0, seed)[:M]
    flat = lambda k: before[k].reshape(N, -1) if before[k].ndim == 3 else before[k].reshape(N)  # noqa: E731
    with torch.no_grad():
        obs0 = torch.as_tensor(flat("observations")[idx], device=env.device)
        mean0, value0 = pi(obs0).cpu().numpy(), vf(obs0).reshape(-1).cpu().numpy()
    lc = LossCase(M, seed=0)
    lc.mean, lc.value, lc.log_std = mean0, value0, log_std.detach().cpu().numpy().copy()
    lc.inv_std = torch.exp(-log_std.detach()).cpu().numpy()
    lc.mb_action, lc.mb_logp, lc.mb_adv, lc.mb_ret, lc.mb_value = (flat(k)[idx] for k in ("actions", "log_probs", "advantages", "returns", "values"))
    lc.adv_stats = np_adv_stats(lc.mb_adv)
    cfg = dict(clip_range=0.2, ent_coef=0.01, vf_coef=0.5)
    ratio = run_loss(hd, lc, **cfg)["ratio_out"]
    want = host_loss(host, lc, ratio_in=ratio, **cfg)["stats"][:8]

    stats = ppo.update()
    torch.cuda.synchronize()
    assert stats is ppo.stats_t and int(ppo.draw_t) == 2
    st = stats.cpu().numpy()
    assert same_f64(st[0, 0], want), (st[0, 0], want)
    assert np.isfinite(st).all() and st[..., 7].sum() == 2 * N and st[:, :, 7].tolist() == [[200, 200, 120]] * 2
    assert abs(st[0, 0, 6] - 1) < 1e-3 and st[1, 2, 6] != 1                              # ratio 1 before the first step, not after
    for p, q in zip(params, p0):
        now = p.detach().cpu().numpy()
        assert np.isfinite(now).all() and (now != q).any(), tuple(p.shape)
    for k, v in col.buffer.items():
        assert np.array_equal(E.bits(v.cpu().numpy()), E.bits(before[k])), k
    again = col.collect()                                        # the next rollout reads the updated modules
    torch.cuda.synchronize()
    assert np.isfinite(again["advantages"].cpu().numpy()).all() and not np.array_equal(again["actions"].cpu().numpy(), before["actions"])
    st2 = ppo.learn(1).cpu().numpy()
    assert np.isfinite(st2).all() and int(ppo.draw_t) == 4 and int(col.draw_base_t) == 3
    env.close()
