"""Recurrent PPO on the GPU: glgym_lstm_cell, glgym_lstm_cell_grad, glgym_seq_batch (include/glgym.h), gl_gym_amd.lstm_cell,
RecurrentCollector and RecurrentPPO.

What can be exact is compared bit for bit with the host instantiation of csrc/gl_lstm.hpp (tests/lstmhost/lstmhost.cpp): the gathered
sequences, the advantage statistics, the backward pass, and the forward pass GIVEN the device's own five activations (the host build takes
them as an input) -- exp and tanh in double are the device's libm, which is not the host's, so `act` is compared with NumPy's double
evaluation within one float32 ulp.  Every output buffer has guard rows behind its last row and guard bytes around it (0xFF); an optional
output that is not asked for and every output of a refused call must come back untouched.

Bounds of the float32-against-float64 comparisons: tests/test_rppo_host.py (step_bounds, sequence_bounds) derives for ONE float32 chain how
far it lies from the exact result; here the products are torch's on the device instead of NumPy's, a second float32 chain, so the bounds
are doubled.  For the collector the chain is the rollout from the last reset of the carried state: n_fwd = steps (D + H + 13)."""
import ctypes as C

import numpy as np
import pytest

import envlayer_inputs as E
from test_gpu_plan import make_env
from test_gpu_ppo import guarded_outputs, read_outputs, run_batch
from test_ppo_host import BATCH_PAIRS, NU, set_path
from test_rppo_host import (CELL_HS, CELL_MS, CELL_REFUSALS, FWD_OPS, GRAD_REFUSALS, MB_, P_, SEQ_GOOD, SEQ_REFUSALS, START_KINDS, U, CellCase,
                            SeqCase, SequenceCase, activations_ok, build_host, cell_args, cell_output_shapes, compare_sequence, grad_args,
                            grad_output_shapes, host_cell, host_cell_grad, host_seq, lstm64, same_f64, same_u32, seq_args, seq_output_shapes,
                            seq_rows, sequence_bounds)

pytestmark = pytest.mark.gpu
CAP_LANES = 256 * 2048 + 77                                   # just past the grid's cap: the first 77 lanes of block 0 take a second element


@pytest.fixture(scope="module")
def hd():
    h = E.Handle(False)
    yield h
    h.close()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("lstmhost_gpu") / "liblstmhost.so")


def same_named(got, want, names):
    for k in names:
        assert (same_f64 if got[k].dtype == np.float64 else same_u32 if got[k].dtype == np.float32 else np.array_equal)(got[k], want[k]), k


# ---- 1. the cell kernels against the host build ----------------------------------------------------------------------------------------
class DeviceCell:
    """The arrays of a CellCase on the device, each between guard bytes, and guarded outputs of both calls."""

    def __init__(self, case):
        self.case = case
        names = ("gx", "gh", "c_prev", "dh", "dc") + (() if case.start is None else ("start",))
        self.inputs = {k: E.Guarded(getattr(case, k)) for k in names}
        self.outs = guarded_outputs(cell_output_shapes(case.M, case.H))
        self.gouts = guarded_outputs(grad_output_shapes(case.M, case.H))

    def ptr(self, k):
        return self.inputs[k].ptr if k in self.inputs else None

    def forward(self, hd, want_act=True):
        c = self.case
        a = cell_args(c.M, c.H, self.ptr("gx"), self.ptr("gh"), self.ptr("c_prev"), self.ptr("start"), self.outs["h"].ptr, self.outs["c"].ptr,
                      self.outs["act"].ptr if want_act else None)
        hd.sync()
        rc = hd.lib.glgym_lstm_cell(hd.h, C.byref(a), hd.stream())
        hd.sync()
        assert rc == 0, (rc, hd.error())
        for g in self.inputs.values():
            g.read()
        return read_outputs(self.outs, dict(h=c.M, c=c.M, act=c.M), ("h", "c", "act") if want_act else ("h", "c"))

    def backward(self, hd, want_dc=True):
        c = self.case
        a = grad_args(c.M, c.H, self.ptr("dh"), self.ptr("dc") if want_dc else None, self.outs["act"].ptr, self.ptr("c_prev"), self.ptr("start"),
                      self.gouts["d_gx"].ptr, self.gouts["d_gh"].ptr, self.gouts["d_c_prev"].ptr)
        hd.sync()
        rc = hd.lib.glgym_lstm_cell_grad(hd.h, C.byref(a), hd.stream())
        hd.sync()
        assert rc == 0, (rc, hd.error())
        for g in self.inputs.values():
            g.read()
        return read_outputs(self.gouts, dict(d_gx=c.M, d_gh=c.M, d_c_prev=c.M), ("d_gx", "d_gh", "d_c_prev"))


def check_cell(hd, host, c, lean=True):
    M = c.M
    dev = DeviceCell(c)
    got = dev.forward(hd)
    assert activations_ok(c, got["act"], got["c"]), (M, c.H)
    ref = host_cell(host, c, act_in=got["act"])                                           # the host build on the device's own activations
    same_named(got, {k: v[:M] for k, v in ref.items()}, ("h", "c", "act"))
    for want_dc in (True, False):
        g = dev.backward(hd, want_dc)
        same_named(g, {k: v[:M] for k, v in host_cell_grad(host, c, got["act"], want_dc).items()}, ("d_gx", "d_gh", "d_c_prev"))
    if lean:                                                                            # act left out: untouched, h and c as before
        same_named(DeviceCell(c).forward(hd, want_act=False), got, ("h", "c"))
    return got


@pytest.mark.parametrize("H", CELL_HS)
@pytest.mark.parametrize("kind", START_KINDS)
def test_cell_against_the_host_build(hd, host, H, kind):
    for M in CELL_MS:
        check_cell(hd, host, CellCase(M, H, kind, seed=M), lean=M in (1, 257))


@pytest.mark.parametrize("H", [1, 4])
def test_cell_just_past_the_grid_cap(hd, host, H):
    """H = 1 takes one unit per lane, H = 4 (16-byte aligned buffers) four: CAP_LANES lanes either way."""
    check_cell(hd, host, CellCase(CAP_LANES, H, "mixed", seed=3), lean=False)


def test_cell_without_16_byte_alignment_takes_the_narrow_path(hd, host):
    """H % 4 == 0 but c_prev four bytes off a 16-byte boundary: the same results."""
    import torch
    c = CellCase(65, 64, "mixed", seed=9)
    dev = DeviceCell(c)
    want = dev.forward(hd)
    raw = torch.zeros(c.M * c.H + 4, dtype=torch.float32, device="cuda:0")
    raw[1:1 + c.M * c.H] = torch.as_tensor(c.c_prev.reshape(-1), device="cuda:0")
    assert (raw.data_ptr() + 4) % 16 != 0
    for o in dev.outs.values():
        o.t[E.GUARD:E.GUARD + o.n] = 0xFF
    a = cell_args(c.M, c.H, dev.ptr("gx"), dev.ptr("gh"), raw.data_ptr() + 4, dev.ptr("start"), dev.outs["h"].ptr, dev.outs["c"].ptr, dev.outs["act"].ptr)
    assert hd.lib.glgym_lstm_cell(hd.h, C.byref(a), hd.stream()) == 0, hd.error()
    hd.sync()
    same_named(read_outputs(dev.outs, dict(h=c.M, c=c.M, act=c.M), ("h", "c", "act")), want, ("h", "c", "act"))


def test_a_reset_row_keeps_nan_and_infinity_out(hd, host):
    for M, H in ((65, 3), (257, 64)):
        c = CellCase(M, H, "mixed", seed=5, poison=True)
        rows = np.flatnonzero(c.start)
        assert not np.isfinite(c.c_prev[rows]).all() and not np.isfinite(c.gh[rows]).all()
        got = check_cell(hd, host, c, lean=False)
        assert np.isfinite(got["h"]).all() and np.isfinite(got["c"]).all() and np.isfinite(got["act"]).all()
        clean = DeviceCell(CellCase(M, H, "mixed", seed=5)).forward(hd)
        same_named(got, clean, ("h", "c", "act"))


# ---- 2. the sequence gather against the host build ---------------------------------------------------------------------------------------
class DeviceSeq:
    def __init__(self, case, S):
        from gl_gym_amd import _lib as L
        self.case, self.S = case, S
        self.inputs = {k: E.Guarded(v) for k, v in case.arrays().items()}
        self.outs = guarded_outputs(seq_output_shapes(case, S))
        self.ws = E.Guarded(shape=(L.SEQ_BATCH_WS_BYTES // 8,), dtype=np.float64)

    def args(self, offset, draw_base_ptr=None, **kw):
        return seq_args(self.case, self.S, offset, lambda k: self.inputs[k].ptr, {k: v.ptr for k, v in self.outs.items()}, self.ws.ptr,
                        draw_base=draw_base_ptr, **kw)

    def read(self, written):
        for g in self.inputs.values():
            g.read()
        self.ws.read()
        return read_outputs(self.outs, seq_rows(self.case, self.S), written)


def run_seq(hd, case, S, offset, draw_base=None, want_index=True, want_stats=True, **kw):
    ds = DeviceSeq(case, S)
    base = None if draw_base is None else E.Guarded(np.array([draw_base], dtype=np.uint64))
    a = ds.args(offset, None if base is None else base.ptr, want_index=want_index, want_stats=want_stats, **kw)
    hd.sync()
    rc = hd.lib.glgym_seq_batch(hd.h, C.byref(a), hd.stream())
    hd.sync()
    assert rc == 0, (rc, hd.error())
    written = tuple(k for k in ds.outs if (k != "mb_index" or want_index) and (k != "adv_stats" or want_stats))
    return ds.read(written)


def check_seq(hd, host, c, S, offset, **kw):
    stats = c.L * S > 1
    got = run_seq(hd, c, S, offset, want_stats=stats, **kw)
    rows = seq_rows(c, S)
    ref = {k: v[:rows[k]] for k, v in host_seq(host, c, S, offset, want_stats=stats, **kw).items()}
    same_named(got, ref, tuple(got))
    return got


@pytest.mark.parametrize("in_dim", [1, 23, 24])
def test_seq_batch_against_the_host_build(hd, host, in_dim):
    kw = dict(seed=0xABCDEF0123, draw_index=5, draw_base=9)
    for B in (1, 3, 8):
        for Ln in (1, 2, 5):
            for n_chunk in (1, 3):
                c = SeqCase(n_chunk * Ln, B, Ln, in_dim, (0, 2, 4)[(B + Ln + n_chunk) % 3], seed=B + Ln)
                N = c.n_seq
                check_seq(hd, host, c, N, 0, **kw)
                if N > 1:
                    check_seq(hd, host, c, max(1, N // 2), N - max(1, N // 2), **kw)


@pytest.mark.parametrize("S", [1, 63, 64, 65, 257])
def test_seq_batch_minibatch_sizes(hd, host, S):
    c = SeqCase(6, 100, 2, 23, 4, seed=S)                          # 300 sequences, four states of unequal width
    got = check_seq(hd, host, c, S, 300 - S, seed=3, draw_index=1)
    lean = run_seq(hd, c, S, 300 - S, seed=3, draw_index=1, want_index=False, want_stats=False)       # the optional outputs left out
    same_named(lean, got, tuple(lean))
    if S == 64:                                                     # a ragged epoch: 64 + 64 + 64 + 64 + 44, every sequence once
        idx = [check_seq(hd, host, c, min(S, 300 - o), o, seed=3, draw_index=1)["mb_index"] for o in range(0, 300, S)]
        assert [len(i) for i in idx] == [64, 64, 64, 64, 44] and np.array_equal(np.sort(np.concatenate(idx)), np.arange(300))


def test_seq_batch_with_one_step_is_ppo_batch_on_the_device(hd):
    c = SeqCase(40, 25, 1, 23, 0, seed=4)
    for M, offset in ((257, 300), (1000, 0)):
        seq = run_seq(hd, c, M, offset, seed=8, draw_index=2, draw_base=1)
        flat = run_batch(hd, c, M, offset, seed=8, draw_index=2, draw_base=1)
        for k in list(BATCH_PAIRS) + ["mb_index", "adv_stats"]:
            assert np.array_equal(seq[k].view(np.uint8), flat[k].view(np.uint8)), k


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(hd):
    """Every refusal returns GLGYM_EINVAL with its text and leaves every output as it was.  The argument blocks point at real device
    buffers throughout: a table entry's k-th megabyte stands for the k-th buffer of the block."""
    L = hd.L

    def remap(value, order):
        if isinstance(value, int) and value >= P_:
            k, rest = divmod(value - P_, MB_)
            return order[k].ptr + rest
        return value

    c = CellCase(130, 64, "mixed", seed=1)
    dev = DeviceCell(c)
    order = [dev.inputs[k] for k in ("gx", "gh", "c_prev", "start")] + [dev.outs[k] for k in ("h", "c", "act")]
    good = lambda: cell_args(c.M, c.H, *(o.ptr for o in order))  # noqa: E731
    for path, value, word in CELL_REFUSALS:
        a = good()
        set_path(a, path, remap(value, order) if path not in ("M", "H", "struct_size") else value)
        assert hd.lib.glgym_lstm_cell(hd.h, C.byref(a), hd.stream()) == L.EINVAL, (path, value)
        assert word in hd.lib.glgym_last_error() and b"glgym_lstm_cell:" in hd.lib.glgym_last_error(), (path, hd.error())
    hd.sync()
    read_outputs(dev.outs, {}, ())
    assert hd.lib.glgym_lstm_cell(hd.h, C.byref(good()), hd.stream()) == 0, hd.error()     # ... and the block they were derived from is good
    hd.sync()
    read_outputs(dev.outs, dict(h=c.M, c=c.M, act=c.M), ("h", "c", "act"))

    order = [dev.inputs[k] for k in ("dh", "dc")] + [dev.outs["act"]] + [dev.inputs[k] for k in ("c_prev", "start")] + \
            [dev.gouts[k] for k in ("d_gx", "d_gh", "d_c_prev")]
    good = lambda: grad_args(c.M, c.H, *(o.ptr for o in order))  # noqa: E731
    for path, value, word in GRAD_REFUSALS:
        a = good()
        set_path(a, path, remap(value, order) if path not in ("M", "H", "struct_size") else value)
        assert hd.lib.glgym_lstm_cell_grad(hd.h, C.byref(a), hd.stream()) == L.EINVAL, (path, value)
        assert word in hd.lib.glgym_last_error() and b"glgym_lstm_cell_grad:" in hd.lib.glgym_last_error(), (path, hd.error())
    hd.sync()
    read_outputs(dev.gouts, {}, ())
    assert hd.lib.glgym_lstm_cell_grad(hd.h, C.byref(good()), hd.stream()) == 0, hd.error()
    hd.sync()
    read_outputs(dev.gouts, dict(d_gx=c.M, d_gh=c.M, d_c_prev=c.M), ("d_gx", "d_gh", "d_c_prev"))

    g = SEQ_GOOD
    sc = SeqCase(g["T"], g["B"], g["L"], g["in_dim"], 2)
    sc.state_dim = g["state_dim"]
    sc.state_src = [np.zeros((sc.n_seq, d), dtype=np.float32) for d in sc.state_dim]
    ds = DeviceSeq(sc, g["S"])
    order = [ds.inputs[k] for k in ("obs", "action", "logp", "advantage", "returns", "value", "episode_starts", "state_src0", "state_src1")] + \
            [ds.outs[k] for k in ("mb_obs", "mb_action", "mb_logp", "mb_adv", "mb_ret", "mb_value", "mb_start", "state_out0", "state_out1", "mb_index",
                                  "adv_stats")] + [ds.ws]
    scalars = ("struct_size", "T", "B", "L", "S", "offset", "in_dim", "n_state", "workspace_bytes")
    for path, value, word in SEQ_REFUSALS:
        a = ds.args(g["offset"], seed=1)
        plain = path in scalars or (isinstance(path, tuple) and path[0] == "state_dim")
        set_path(a, path, value if plain else remap(value, order))
        assert hd.lib.glgym_seq_batch(hd.h, C.byref(a), hd.stream()) == L.EINVAL, (path, value)
        assert word in hd.lib.glgym_last_error() and b"glgym_seq_batch:" in hd.lib.glgym_last_error(), (path, hd.error())
    hd.sync()
    ds.read(())
    assert ds.ws.untouched()
    assert hd.lib.glgym_seq_batch(hd.h, C.byref(ds.args(g["offset"], seed=1)), hd.stream()) == 0, hd.error()
    hd.sync()
    ds.read(tuple(ds.outs))


# ---- 4. lstm_cell through autograd -------------------------------------------------------------------------------------------------------
def test_lstm_cell_autograd_against_torchs_lstm_in_float64(hd):
    """The package's chain on the device -- one input product, then per step h W_hh^T and lstm_cell, backward through autograd -- against
    torch.nn.LSTM in float64 on the CPU stepped with sb3-contrib's masked state: every h, the last c, the gradients of W_ih, W_hh and the two
    biases within twice sequence_bounds; against the float64 run that ignores the starts the same comparison misses by more than 100x."""
    import torch
    from gl_gym_amd import lstm_cell
    sc = SequenceCase()
    dev = "cuda:0"
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    W_ih, W_hh, b_ih, b_hh = (T(x).requires_grad_() for x in (sc.W_ih, sc.W_hh, sc.b_ih, sc.b_hh))
    obs, starts = T(sc.obs), T(sc.starts)
    gx = torch.nn.functional.linear(obs.reshape(sc.Ln * sc.S, sc.D), W_ih, b_ih + b_hh).view(sc.Ln, sc.S, -1)
    h, c, hs = T(sc.h0), T(sc.c0), []
    for l in range(sc.Ln):
        h, c = lstm_cell(gx[l], torch.nn.functional.linear(h, W_hh), c, starts[l], handle=hd.h)
        hs.append(h)
    hs = torch.stack(hs)
    ((hs * T(sc.w_h)).sum() + (c * T(sc.w_c)).sum()).backward()
    torch.cuda.synchronize()
    got = dict(h=hs.detach().cpu().numpy().astype(np.float64), c_last=c.detach().cpu().numpy().astype(np.float64),
               grads={k: v.grad.cpu().numpy().astype(np.float64) for k, v in (("weight_ih", W_ih), ("weight_hh", W_hh), ("bias_ih", b_ih), ("bias_hh", b_hh))})
    ref = lstm64(sc)
    Ef, Eg = sequence_bounds(sc, ref)
    Ef, Eg = 2 * Ef, {k: 2 * v for k, v in Eg.items()}
    ratio = compare_sequence(got, ref, Ef, Eg)
    print(f"largest |device float32 - float64| / bound: {ratio}")
    assert max(ratio.values()) <= 1.0, ratio
    blind = compare_sequence(got, lstm64(sc, masked=False), Ef, Eg)
    print(f"the same with the starts ignored: {blind}")
    assert min(blind.values()) >= 100.0, blind
    # no gradient required: nothing is saved and the outputs are the same
    with torch.no_grad():
        h2, c2 = lstm_cell(gx[0].detach(), torch.nn.functional.linear(T(sc.h0), W_hh), T(sc.c0), starts[0], handle=hd.h)
    assert torch.equal(h2, hs[0].detach()) and not h2.requires_grad


# ---- 5. RecurrentCollector on a real environment ---------------------------------------------------------------------------------------
ARRANGEMENTS = ["separate", "shared", "actor_only"]
COL_T, COL_L, COL_B, COL_H = 8, 4, 8, 8
SEASON = 2.5 / 96.0                                           # N = 2: an episode is N + 1 = 3 steps of 900 s and ends inside the chunks of four


def make_heads(env, arrangement, seed=0):
    """LSTMs with |W_hh|_inf <= 1/4 and input weights scaled by the observation columns' sizes over a short rollout, so that the gates are not saturated; heads
    that are slices of their input (no reduction), with a trainable scale and offset."""
    import torch
    from gl_gym_amd import RecurrentHeads
    dev, D, H = env.device, env.obs_dim, COL_H
    gen = torch.Generator().manual_seed(seed)
    obs = env.reset_tensor(5)
    amax = obs.abs().amax(dim=0)
    still = torch.zeros(env.num_envs, NU, device=dev)
    for _ in range(2 * COL_T):                                     # the columns' sizes over a rollout of the tests' length, controls at rest
        amax = torch.maximum(amax, env.step_tensor(still)[0].abs().amax(dim=0))
    scale = (amax + 1.0).cpu()

    def lstm(k):
        m = torch.nn.LSTM(D, H)
        with torch.no_grad():
            m.weight_ih_l0.copy_((torch.rand(4 * H, D, generator=gen) * 2 - 1) * (1.5 / D ** 0.5) / scale[None, :])
            m.weight_hh_l0.copy_((torch.rand(4 * H, H, generator=gen) * 2 - 1) * (0.25 / H))
            m.bias_ih_l0.copy_((torch.rand(4 * H, generator=gen) - 0.5) * 0.4)
            m.bias_hh_l0.copy_((torch.rand(4 * H, generator=gen) - 0.5) * 0.4)
        return m.to(dev)

    class Slice(torch.nn.Module):
        def __init__(self, lo, hi, gain):
            super().__init__()
            self.lo, self.hi = lo, hi
            self.a, self.b = torch.nn.Parameter(torch.full((hi - lo,), gain)), torch.nn.Parameter(torch.zeros(hi - lo))

        def forward(self, x):
            return x[:, self.lo:self.hi] * self.a + self.b

    log_std = torch.nn.Parameter(torch.full((NU,), -0.5, device=dev))
    vf = Slice(6, 7, 1e-3 if arrangement == "actor_only" else 1.0).to(dev)
    return RecurrentHeads(lstm(0), Slice(0, NU, 1.5).to(dev), vf, log_std, lstm_vf=lstm(1) if arrangement == "separate" else None,
                          shared_lstm=arrangement == "shared")


def replay64(heads, name, obs, starts, h, c, use_starts=True):
    """The LSTM `name` in float64 on the CPU over buffer observations [T, B, D] with sb3-contrib's masked state from (h, c) -> the states
    in front of every step [T + 1], and the largest |a| and |c| met."""
    import torch
    m = heads.lstms[name]
    ref = torch.nn.LSTM(m.input_size, m.hidden_size).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in m.state_dict().items()})
    hs, cs, amax = [h], [c], 0.0
    with torch.no_grad():
        for k in range(obs.shape[0]):
            keep = 1.0 - torch.as_tensor(starts[k].astype(np.float64))[None, :, None] if use_starts else 1.0
            x = torch.as_tensor(obs[k].astype(np.float64))
            amax = max(amax, float((x @ ref.weight_ih_l0.T + ref.bias_ih_l0 + ref.bias_hh_l0).abs().max()) + 0.25)
            _, (h, c) = ref(x[None], (keep * h, keep * c))
            hs.append(h)
            cs.append(c)
    return hs, cs, max(1.0, amax, max(float(x.abs().max()) for x in cs))


def collector_of(arrangement, B=COL_B, seed=0):
    from gl_gym_amd import RecurrentCollector
    env = make_env(B, "float32", season_length=SEASON, auto_reset=True)
    heads = make_heads(env, arrangement, seed)
    col = RecurrentCollector(env, COL_T, heads, seq_len=COL_L, gamma=0.9631, gae_lambda=0.9167, seed=3)
    col.reset(seed=5)
    return env, heads, col


def snapshot(buf):
    out = {k: v.cpu().numpy().copy() for k, v in buf.items() if k != "lstm_states"}
    for n, st in buf["lstm_states"].items():
        for k, v in st.items():
            out[f"{n}_{k}"] = v.cpu().numpy().copy()
    return out


@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
def test_collector_carries_and_resets_the_state(arrangement):
    import torch
    env, heads, col = collector_of(arrangement)
    assert set(col.buffer["lstm_states"]) == ({"pi", "vf"} if arrangement == "separate" else {"pi"})
    runs = []
    for _ in range(2):
        col.collect()
        torch.cuda.synchronize()
        runs.append(snapshot(col.buffer))
    first, second = runs
    assert first["pi_h"].shape == (COL_T // COL_L, COL_B, COL_H) and not first["pi_h"][0].any() and not first["pi_c"][0].any()   # reset() zeroed it
    starts = np.concatenate([first["episode_starts"], second["episode_starts"]])
    assert (starts[0] == 1).all() and np.array_equal(starts[1:COL_T], first["dones"][:-1]) and np.array_equal(starts[COL_T], first["dones"][-1])
    inside = [k for k in range(2 * COL_T) if k % COL_L and starts[k].any()]
    assert len(inside) >= 2, "no episode starts inside a chunk: the season is not a few steps"
    obs = np.concatenate([first["observations"], second["observations"]])
    D, n_chunk = obs.shape[-1], COL_T // COL_L
    for name in heads.lstms:
        z = torch.zeros(1, COL_B, COL_H, dtype=torch.float64)
        stored_h = np.concatenate([first[f"{name}_h"], second[f"{name}_h"]])
        stored_c = np.concatenate([first[f"{name}_c"], second[f"{name}_c"]])
        worst = {}
        for use_starts in (True, False):
            hs, cs, A = replay64(heads, name, obs, starts, z, z, use_starts)
            # the chain behind the state in front of step k is at most k steps long (a start cuts it); two float32 chains: doubled
            err = 0.0
            for q in range(2 * n_chunk):
                k = q * COL_L
                bound = 2 * max(k, 1) * (D + COL_H + FWD_OPS) * A * U
                # stored raw: the state in front of step k BEFORE that step's reset
                err = max(err, float(np.abs(stored_h[q] - hs[k][0].numpy()).max()) / bound, float(np.abs(stored_c[q] - cs[k][0].numpy()).max()) / bound)
            worst[use_starts] = err
        print(f"{arrangement} / {name}: largest |stored - float64 replay| / bound = {worst[True]:.3e}; with the starts ignored {worst[False]:.3e}")
        assert worst[True] <= 1.0 and worst[False] >= 100.0, worst
    assert second["pi_h"][0].any()                                                        # the second collect() went on from the first
    assert np.isfinite(second["advantages"]).all() and np.abs(second["actions"]).max() > 0.1 and second["values"].std() > 0
    # a second, identically seeded run is bit-identical
    env2, _, col2 = collector_of(arrangement)
    for want in runs:
        col2.collect()
        torch.cuda.synchronize()
        got = snapshot(col2.buffer)
        for k, v in want.items():
            assert np.array_equal(E.bits(got[k]), E.bits(v)), k
    # reset() zeroes the carried state again
    col2.reset(seed=5)
    col2.collect()
    torch.cuda.synchronize()
    again = snapshot(col2.buffer)
    assert not again["pi_h"][0].any() and not again["pi_c"][0].any() and again["pi_h"][1].any()
    env.close()
    env2.close()


def test_actions_of_an_environment_do_not_depend_on_the_batch():
    """Environment b's noise is keyed by (seed, b, step, draw) and its state rows, ping-pong halves and chunk slots are its own: the first
    three environments of a batch of eight act as a batch of three, at every step.  From step 1 on the two rollouts need not see the same
    observations (the products of the two runs have different shapes, and the environment answers a last-bit difference of an action in
    its own way), so each run is taken by itself: the policy LSTM is replayed in float64 from the run's OWN observations and episode
    starts, the mean is pi_module's on it (a slice times 1.5), and the noise is recovered as e = (action - mean) / std.  The recovered noise
    of environment b must be the same in both runs.  Bound per run and step k: the float32 chain behind the state is at most k + 1 steps
    long (tests/test_rppo_host.py: (k + 1) (D + H + 13) A u), times 1.5 for the mean, plus the three float32 roundings of
    action = mean + std e on |action| <= Amax, all over std; the two runs' bounds add."""
    import torch
    runs = []
    for B in (8, 3):
        env, heads, col = collector_of("separate", B=B)
        col.collect()
        torch.cuda.synchronize()
        buf = snapshot(col.buffer)
        z = torch.zeros(1, B, COL_H, dtype=torch.float64)
        hs, _, A = replay64(heads, "pi", buf["observations"], buf["episode_starts"], z, z)
        std = float(np.exp(np.float64(np.float32(-0.5))))
        mean = np.stack([1.5 * hs[k + 1][0].numpy()[:, :NU] for k in range(COL_T)])                  # [T, B, 6]
        D = buf["observations"].shape[-1]
        a_max = float(np.abs(buf["actions"]).max())
        bound = np.array([(1.5 * (k + 1) * (D + COL_H + FWD_OPS) * A + 3 * a_max) * U / std for k in range(COL_T)])
        runs.append(dict(buf=buf, eps=(buf["actions"].astype(np.float64) - mean) / std, bound=bound))
        env.close()
    big, small = runs
    assert np.array_equal(E.bits(big["buf"]["observations"][0, :3]), E.bits(small["buf"]["observations"][0]))
    assert np.array_equal(big["buf"]["episode_starts"][:, :3], small["buf"]["episode_starts"]) and small["buf"]["episode_starts"][1:].any()
    diff = np.abs(big["eps"][:, :3] - small["eps"]).reshape(COL_T, -1).max(axis=1)
    bound = big["bound"] + small["bound"]
    print(f"largest |recovered noise difference| per step: {diff}\nbound per step: {bound}")
    assert (diff <= bound).all(), (diff, bound)
    # the check can see a wrong row: another environment's noise is of order 1 away, and the noise is noise (mean 0, deviation 1)
    assert np.abs(big["eps"][:, :3] - big["eps"][:, 3:6]).reshape(COL_T, -1).max(axis=1).min() > 100 * bound.max()
    assert abs(big["eps"].mean()) < 0.5 and 0.5 < big["eps"].std() < 1.5


# ---- 6. RecurrentPPO.update() ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
def test_update_on_a_collector(arrangement):
    import copy
    import torch
    from gl_gym_amd import RecurrentPPO
    env, heads, col = collector_of(arrangement)
    col.collect()
    params = heads.parameters()
    assert len(params) == {"separate": 13, "shared": 9, "actor_only": 9}[arrangement]
    modules = list(heads.lstms.values()) + [heads.pi_module, heads.vf_module]
    saved = [copy.deepcopy(m.state_dict()) for m in modules] + [heads._log_std_src.detach().clone()]

    def fresh():
        for m, sd in zip(modules, saved[:-1]):
            m.load_state_dict(sd)
        with torch.no_grad():
            heads._log_std_src.copy_(saved[-1])
        opt = torch.optim.Adam(params, lr=1e-2)
        return RecurrentPPO(col, opt, n_epochs=2, batch_size=6, clip_range=0.2, ent_coef=0.01, vf_coef=0.5, seed=21)

    ppo = fresh()
    N = (COL_T // COL_L) * COL_B
    assert ppo.N == N == 16 and ppo.sizes == [6, 6, 4] and ppo.stats_t.shape == (2, 3, 8) and ppo.stats_t.dtype == torch.float64
    torch.cuda.synchronize()
    before = snapshot(col.buffer)
    p0 = [p.detach().cpu().numpy().copy() for p in params]
    z = torch.zeros(1, COL_B, COL_H, dtype=torch.float64)
    A = replay64(heads, "pi", before["observations"], before["episode_starts"], z, z)[2]      # with the weights the rollout was collected with
    stats = ppo.update()
    torch.cuda.synchronize()
    st = stats.cpu().numpy().copy()
    assert stats is ppo.stats_t and int(ppo.draw_t) == 2
    assert np.isfinite(st).all() and st[:, :, 7].tolist() == [[6 * COL_L, 6 * COL_L, 4 * COL_L]] * 2
    # before the first optimiser step the ratio is 1 up to the two float32 chains: the collection's products are [B, D] x [D, 4H] step by
    # step, the update's one [L S, D] x [D, 4H], so the means differ by at most dm = 1.5 * 2 Ef (pi_module is a slice times 1.5) with
    # Ef = L (D + H + 13) A u, A from the float64 replay of the rollout; a log-probability by at most 6 z_max dm / std with |z| <= 6 and std = exp(-0.5), plus its own
    # 24 operations on terms below 10 (tests/test_ppo_host.py); the ratio is exp of that
    D = col.D
    dm = 1.5 * 2 * COL_L * (D + COL_H + FWD_OPS) * A * U
    dlogp = 6 * 6.0 * dm / np.exp(-0.5) + 24 * 10 * U
    print(f"{arrangement}: first minibatch max ratio - 1 = {st[0, 0, 6] - 1:.3e}, bound {np.expm1(dlogp):.3e}; last {st[1, 2, 6] - 1:.3e}")
    assert abs(st[0, 0, 6] - 1) <= np.expm1(dlogp) and st[1, 2, 6] != 1
    for p, q in zip(params, p0):
        now = p.detach().cpu().numpy()
        assert np.isfinite(now).all() and (now != q).any(), tuple(p.shape)
    after = snapshot(col.buffer)
    for k, v in before.items():
        assert np.array_equal(E.bits(after[k]), E.bits(v)), k
    # the same buffer, the same seed, the parameters and the optimiser as they were: the same statistics
    again = fresh().update()
    torch.cuda.synchronize()
    assert same_f64(again.cpu().numpy(), st)
    st2 = ppo.learn(1).cpu().numpy()
    assert np.isfinite(st2).all() and int(col.draw_base_t) == 2
    env.close()


# ---- 7. graph capture --------------------------------------------------------------------------------------------------------------------
def test_collect_and_update_in_one_captured_graph():
    """A collect() + update() pair captured once (after one eager pair on a side stream, which also creates Adam's device state) and replayed
    twice, against an identically seeded twin that runs three eager pairs: the same operations in the same order, so the statistics, the
    buffer and every parameter agree bit for bit.  The draw words are device tensors: every replay collects with fresh noise and shuffles anew."""
    import torch
    from gl_gym_amd import RecurrentPPO

    def setup():
        env, heads, col = collector_of("separate")
        opt = torch.optim.Adam(heads.parameters(), lr=1e-3, capturable=True)
        ppo = RecurrentPPO(col, opt, n_epochs=1, batch_size=6, clip_range=0.2, ent_coef=0.01, vf_coef=0.5, seed=21)
        return env, heads, col, ppo

    def pair(col, ppo):
        col.collect()
        ppo.update()

    env_a, heads_a, col_a, ppo_a = setup()
    for _ in range(3):
        pair(col_a, ppo_a)
    torch.cuda.synchronize()
    want_stats, want_buf = ppo_a.stats_t.cpu().numpy().copy(), snapshot(col_a.buffer)
    want_params = [p.detach().cpu().numpy().copy() for p in heads_a.parameters()]

    env_b, heads_b, col_b, ppo_b = setup()
    side = torch.cuda.Stream(device="cuda:0")
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pair(col_b, ppo_b)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair(col_b, ppo_b)
    torch.cuda.synchronize()
    assert int(col_b.draw_base_t) == 1 and int(ppo_b.draw_t) == 1                        # capturing ran nothing
    first = None
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        first = first if first is not None else snapshot(col_b.buffer)
    assert int(col_b.draw_base_t) == 3 and int(ppo_b.draw_t) == 3
    got_stats, got_buf = ppo_b.stats_t.cpu().numpy(), snapshot(col_b.buffer)
    assert not np.array_equal(first["actions"], got_buf["actions"])                       # the second replay is another rollout
    print("largest |statistics difference| graph - eager:", np.abs(got_stats - want_stats).max())
    assert np.isfinite(got_stats).all() and same_f64(got_stats, want_stats)
    for k, v in want_buf.items():
        assert np.array_equal(E.bits(got_buf[k]), E.bits(v)), k
    for p, q in zip(heads_b.parameters(), want_params):
        assert np.array_equal(E.bits(p.detach().cpu().numpy()), E.bits(q)), tuple(p.shape)
    env_a.close()
    env_b.close()
