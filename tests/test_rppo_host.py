"""CPU tests of recurrent PPO: csrc/gl_lstm.hpp (host instantiation, tests/lstmhost/lstmhost.cpp -- a lane is a pass of a loop) against
NumPy restatements written from the text of include/glgym.h; the cell against a single-layer torch.nn.LSTM in float64 stepped with
sb3-contrib's masked state; the refusals of glgym_lstm_cell / glgym_lstm_cell_grad / glgym_seq_batch through libglgym.so (no device: every
check precedes the handle) and of the Python classes.  The helpers below are also what tests/test_gpu_rppo.py compares the kernels with.

Bounds.
* forward GIVEN the five activations, backward, the gathered rows, the advantage statistics: EXACT.  Every step is a single correctly
  rounded operation in a fixed order, which NumPy performs in the same order.
* the five activations: within one float32 ulp of NumPy's double evaluation rounded to float (the libm behind exp and tanh differs in the
  last bits of a double).
* the advantage statistics against np.mean / np.std(ddof=1): the bounds of tests/test_ppo_host.py.
* float32 against float64, u = 2^-24, in the manner of tests/test_ppo_host.py: a value at the end of a chain of n float32 operations, none
  of which amplifies an error, on quantities no larger than A is off by at most n A u.  Nothing amplifies here: the gates' slopes are at most
  1/4 (sigmoid) and 1 (tanh); f, i, o and |tc| are at most 1; the cases keep |W_hh|_inf at 1/4.
  One step (step_bounds): a unit's forward pass is FWD_OPS = 13 roundings (4 sums a_k, 4 casts of the gates, 2 products and a sum for c,
  the cast of tc, the product h), so |delta h|, |delta c| <= Ef = 13 A u with A = max(1, max |a|, max |c|).  Its backward pass is
  BWD_OPS = 22 roundings on products of dct with at most four factors (activations or c0, each off by at most Ef, each at most
  Cmax = max(1, max |c|)): |delta d| <= Eb = (4 Ef + 22 u) Cmax Dmax with Dmax = max |dh| + max |dc|.
  A sequence of L steps behind products of K = D + H terms (sequence_bounds): the chain to the last h has n_fwd = L (K + 13)
  operations, Ef = n_fwd A u.  A weight gradient is a sum over the R = L S rows of da x; a da is dct times factors off by at most Ef as
  above, behind at most L (22 + H) roundings of the backward chain (H for d_gh W_hh), and the sum adds R:
  |delta dW| <= Eg = R Xmax DAmax u (4 n_fwd A + L (22 + H) + R), DAmax = Dmax max(1, Cmax / 4) (da_f = dct c0 f (1 - f); the other three
  are at most dct).  The magnitudes A, Cmax, Xmax and Dmax (the largest |dL/dc| of any step) are read from the float64 reference run and
  the inputs, never from the code under test."""
import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from test_plan_cem_host import within_one_f32_ulp
from test_ppo_host import (BATCH_PAIRS, NU, SENTINEL, BatchCase, guarded, host_batch, np_adv_stats, np_perm, np_reduce, same_f64,
                           same_u32, set_path, sum_bound)
from test_ppo_host import build_host as build_ppohost

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SRC = ROOT / "tests" / "lstmhost" / "lstmhost.cpp"
f = np.float32
U = 2.0 ** -24
N_ACT = 5
FWD_OPS, BWD_OPS = 13, 22
CELL_MS = [1, 63, 64, 65, 255, 256, 257]
CELL_HS = [1, 3, 64, 65]
START_KINDS = ["null", "zeros", "ones", "mixed"]


def build_host(path):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.lstmhost_sizeof.argtypes, lib.lstmhost_sizeof.restype = [C.c_int], C.c_int
    lib.lstmhost_n_blocks.argtypes, lib.lstmhost_n_blocks.restype = [C.c_longlong], C.c_int
    lib.lstmhost_cell.argtypes, lib.lstmhost_cell.restype = [C.c_void_p, C.c_void_p], None
    lib.lstmhost_cell_grad.argtypes, lib.lstmhost_cell_grad.restype = [C.c_void_p], None
    lib.lstmhost_seq_batch.argtypes, lib.lstmhost_seq_batch.restype = [C.c_void_p], None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_lstm.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    return build_host(tmp_path_factory.mktemp("lstmhost") / "liblstmhost.so")


@pytest.fixture(scope="module")
def ppohost(tmp_path_factory):
    return build_ppohost(tmp_path_factory.mktemp("ppohost_rppo") / "libppohost.so")


# ---- the cell: cases, restatements, host calls -------------------------------------------------------------------------------------------
def start_of(kind, M, seed=0):
    if kind == "null":
        return None
    if kind in ("zeros", "ones"):
        return np.full(M, kind == "ones", dtype=np.uint8)
    s = (np.random.default_rng([seed, M, 3]).uniform(size=M) < 0.4).astype(np.uint8)
    s[0] = 1                                                       # M = 1 included: at least one reset row
    if M > 1:
        s[1] = 0
    return s * np.uint8(7) if M % 2 else s                         # any non-zero byte starts an episode


class CellCase:
    """Inputs of one glgym_lstm_cell / glgym_lstm_cell_grad call in NumPy."""

    def __init__(self, M, H, start="mixed", seed=0, poison=False):
        rng = np.random.default_rng([seed, M, H, 11])
        self.M, self.H = M, H
        self.gx = rng.normal(size=(M, 4 * H)).astype(f) * f(1.5)
        self.gh = rng.normal(size=(M, 4 * H)).astype(f)
        self.c_prev = rng.normal(size=(M, H)).astype(f) * f(0.8)
        self.start = start_of(start, M, seed)
        self.dh = rng.normal(size=(M, H)).astype(f)
        self.dc = rng.normal(size=(M, H)).astype(f) * f(0.5)
        if poison:                                                 # what a diverged episode leaves behind, in rows that start a new one
            rows = np.flatnonzero(self.start)
            self.c_prev[rows[0::2], 0] = np.nan
            self.c_prev[rows[1::2], -1] = np.inf
            self.gh[rows[0::2], H] = -np.inf
            self.gh[rows[1::2], 4 * H - 1] = np.nan

    def keep(self):
        return np.ones(self.M, dtype=bool) if self.start is None else self.start == 0


def np_preact(c):
    """-> a [M, 4, H] and c0 [M, H], float32: the select of the header."""
    k = c.keep()[:, None, None]
    gx, gh = c.gx.reshape(c.M, 4, c.H), c.gh.reshape(c.M, 4, c.H)
    with np.errstate(all="ignore"):
        a = np.where(k, gx + gh, gx).astype(f)
    return a, np.where(k[:, 0], c.c_prev, f(0)).astype(f)


def np_gates64(a):
    """The four gate activations in double from a [M, 4, H] float32."""
    a = a.astype(np.float64)
    with np.errstate(all="ignore"):
        sig = lambda x: 1.0 / (1.0 + np.exp(-x))  # noqa: E731
        return np.stack([sig(a[:, 0]), sig(a[:, 1]), np.tanh(a[:, 2]), sig(a[:, 3])], axis=1)


def np_cell_given(c, act):
    """h, c of the call given its activations act [M, 5, H]: c = f * c0 + i * g (two products, one sum), h = o * tc."""
    _, c0 = np_preact(c)
    i, fg, g, o, tc = (act[:, k] for k in range(N_ACT))
    with np.errstate(all="ignore"):
        cell = (fg * c0).astype(f) + (i * g).astype(f)
        return (o * tc).astype(f), cell.astype(f)


def np_cell_grad(c, act, want_dc=True):
    """d_gx, d_gh [M, 4H] and d_c_prev [M, H] from the header's text, float32, every operation on its own."""
    _, c0 = np_preact(c)
    keep = c.keep()[:, None]
    i, fg, g, o, tc = (act[:, k] for k in range(N_ACT))
    one = f(1)
    with np.errstate(all="ignore"):
        dh = c.dh
        dc = c.dc if want_dc else np.zeros_like(c.dh)
        d_o = dh * tc
        dct = dc + (dh * o) * (one - tc * tc)
        da = np.stack([(dct * g) * (i * (one - i)), (dct * c0) * (fg * (one - fg)), (dct * i) * (one - g * g), d_o * (o * (one - o))], axis=1).astype(f)
        d_gh = np.where(keep[:, :, None], da, f(0)).astype(f)
        d_cp = np.where(keep, dct * fg, f(0)).astype(f)
    return da.reshape(c.M, 4 * c.H), d_gh.reshape(c.M, 4 * c.H), d_cp


def ptr_of(x):
    return None if x is None else x.ctypes.data


def cell_args(M, H, gx, gh, c_prev, start, h, c, act):
    from gl_gym_amd import _lib as L
    return L.make_plan_args(L.LstmCellArgs, M, H, gx, gh, c_prev, start, h, c, act)


def grad_args(M, H, dh, dc, act, c_prev, start, d_gx, d_gh, d_c_prev):
    from gl_gym_amd import _lib as L
    return L.make_plan_args(L.LstmCellGradArgs, M, H, dh, dc, act, c_prev, start, d_gx, d_gh, d_c_prev)


def cell_output_shapes(M, H):
    return dict(h=((M, H), np.float32), c=((M, H), np.float32), act=((M, N_ACT * H), np.float32))


def grad_output_shapes(M, H):
    return dict(d_gx=((M, 4 * H), np.float32), d_gh=((M, 4 * H), np.float32), d_c_prev=((M, H), np.float32))


def host_cell(host, c, act_in=None, want_act=True):
    """lstmhost_cell on the case -> {name: array with its GUARD rows}."""
    outs = {k: guarded(s, dt) for k, (s, dt) in cell_output_shapes(c.M, c.H).items()}
    a = cell_args(c.M, c.H, ptr_of(c.gx), ptr_of(c.gh), ptr_of(c.c_prev), ptr_of(c.start), ptr_of(outs["h"]), ptr_of(outs["c"]),
                  ptr_of(outs["act"]) if want_act else None)
    ai = None if act_in is None else np.ascontiguousarray(act_in, dtype=f)
    host.lstmhost_cell(C.addressof(a), ptr_of(ai))
    return outs


def host_cell_grad(host, c, act, want_dc=True):
    outs = {k: guarded(s, dt) for k, (s, dt) in grad_output_shapes(c.M, c.H).items()}
    act = np.ascontiguousarray(act, dtype=f)
    a = grad_args(c.M, c.H, ptr_of(c.dh), ptr_of(c.dc) if want_dc else None, ptr_of(act), ptr_of(c.c_prev), ptr_of(c.start), ptr_of(outs["d_gx"]),
                  ptr_of(outs["d_gh"]), ptr_of(outs["d_c_prev"]))
    host.lstmhost_cell_grad(C.addressof(a))
    return outs


def check_rows(got, want, M, names=None):
    """got: guarded outputs; rows < M of every name in want equal it bit for bit with the guard rows intact; every other output is untouched."""
    for k, v in got.items():
        if k in want and (names is None or k in names):
            assert same_u32(v[:M], want[k]), (k, v[:M], want[k])
            assert (v[M:] == SENTINEL).all(), k
        elif k not in want:
            assert (v == SENTINEL).all(), k


def activations_ok(c, act, cell):
    """act [M, 5H] within one float32 ulp of the double evaluation: the gates of the pre-activations, tc of the call's own c."""
    a, _ = np_preact(c)
    act = act.reshape(c.M, N_ACT, c.H)
    with np.errstate(all="ignore"):
        return within_one_f32_ulp(act[:, :4], np_gates64(a)) and within_one_f32_ulp(act[:, 4], np.tanh(cell.astype(np.float64)))


# ---- sequences: cases, restatement, host call -------------------------------------------------------------------------------------------
STATE_DIMS = (5, 64, 1, 3)
SEQ_PAIRS = dict(BATCH_PAIRS, mb_start="episode_starts")


class SeqCase(BatchCase):
    """A collector's [T][B] buffer, flat, plus episode starts and n_state state tensors [T / L][B][dim]."""

    def __init__(self, T, B, L, in_dim, n_state=0, seed=0):
        super().__init__(T * B, in_dim, seed=seed)
        rng = np.random.default_rng([seed, T, B, L, 9])
        self.T, self.B, self.L, self.n_state = T, B, L, n_state
        self.n_seq = (T // L) * B
        self.episode_starts = (rng.uniform(size=T * B) < 0.3).astype(np.uint8)
        self.state_dim = STATE_DIMS[:n_state]
        self.state_src = [rng.normal(size=(self.n_seq, d)).astype(f) for d in self.state_dim]

    def arrays(self):
        return dict(super().arrays(), episode_starts=self.episode_starts, **{f"state_src{k}": s for k, s in enumerate(self.state_src)})


def seq_output_shapes(c, S):
    M = c.L * S
    out = dict(mb_obs=((M, c.in_dim), np.float32), mb_action=((M, NU), np.float32), mb_logp=((M,), np.float32), mb_adv=((M,), np.float32),
               mb_ret=((M,), np.float32), mb_value=((M,), np.float32), mb_start=((M,), np.uint8), mb_index=((S,), np.int32),
               adv_stats=((2,), np.float64))
    out.update({f"state_out{k}": ((S, d), np.float32) for k, d in enumerate(c.state_dim)})
    return out


def seq_rows(c, S):
    return {k: (2 if k == "adv_stats" else S if k == "mb_index" or k.startswith("state_out") else c.L * S) for k in seq_output_shapes(c, S)}


def seq_args(c, S, offset, ptr, out, workspace, seed=1, draw_index=0, draw_base=None, want_index=True, want_stats=True, workspace_bytes=None):
    from gl_gym_amd import _lib as L
    pad = [None] * (4 - c.n_state)
    return L.make_plan_args(L.SeqBatchArgs, c.T, c.B, c.L, S, offset, c.in_dim, c.n_state, (C.c_int32 * 4)(*(list(c.state_dim) + [0] * (4 - c.n_state))),
                            seed, draw_index, draw_base, ptr("obs"), ptr("action"), ptr("logp"), ptr("advantage"), ptr("returns"), ptr("value"),
                            ptr("episode_starts"), (C.c_void_p * 4)(*([ptr(f"state_src{k}") for k in range(c.n_state)] + pad)),
                            out["mb_obs"], out["mb_action"], out["mb_logp"], out["mb_adv"], out["mb_ret"], out["mb_value"], out["mb_start"],
                            (C.c_void_p * 4)(*([out[f"state_out{k}"] for k in range(c.n_state)] + pad)),
                            out["mb_index"] if want_index else None, out["adv_stats"] if want_stats else None,
                            workspace if want_stats else None, L.SEQ_BATCH_WS_BYTES if workspace_bytes is None else workspace_bytes)


def host_seq(host, c, S, offset, draw_base=None, **kw):
    from gl_gym_amd import _lib as L
    arrays = c.arrays()
    outs = {k: guarded(s, dt) for k, (s, dt) in seq_output_shapes(c, S).items()}
    ws = np.zeros(L.SEQ_BATCH_WS_BYTES // 8)
    base = None if draw_base is None else np.array([draw_base], dtype=np.uint64)
    a = seq_args(c, S, offset, lambda k: arrays[k].ctypes.data, {k: v.ctypes.data for k, v in outs.items()}, ws.ctypes.data,
                 draw_base=None if base is None else base.ctypes.data, **kw)
    host.lstmhost_seq_batch(C.addressof(a))
    return outs


def np_seq(c, S, offset, D, seed, want_stats=True):
    """Every output of the call from the header's text: sequence q is chunk q // B of environment q % B; row (l, s) is l S + s."""
    q = np_perm(c.n_seq, D, seed)[offset:offset + S]
    rows = ((q // c.B) * c.L)[None, :] * c.B + np.arange(c.L)[:, None] * c.B + (q % c.B)[None, :]              # [L, S]
    flat = rows.reshape(-1)
    out = {k: getattr(c, src)[flat] for k, src in SEQ_PAIRS.items()}
    out["mb_index"] = q.astype(np.int32)
    for k, s in enumerate(c.state_src):
        out[f"state_out{k}"] = s[q]
    if want_stats:
        out["adv_stats"] = np_adv_stats(out["mb_adv"])
    return out


def check_seq(got, want, rows):
    for k, v in got.items():
        n = rows[k]
        if k in want:
            if v.dtype == np.float64:
                assert same_f64(v[:n], want[k]), (k, v[:n], want[k])
            elif v.dtype == np.float32:
                assert same_u32(v[:n], want[k]), (k, v[:n], want[k])
            else:
                assert np.array_equal(v[:n], want[k]), k
            assert (v[n:] == v.dtype.type(SENTINEL)).all(), k
        else:
            assert (v == v.dtype.type(SENTINEL)).all(), k


# ---- the float64 LSTM and the float32 chain ------------------------------------------------------------------------------------------------
class SequenceCase:
    """A time-major minibatch obs [L, S, D], starts inside the sequences, and the weights of a single-layer LSTM with |W_hh|_inf = 1/4."""

    def __init__(self, Ln=5, S=5, D=5, H=6, seed=0):
        rng = np.random.default_rng([seed, Ln, S, D, H])
        self.Ln, self.S, self.D, self.H = Ln, S, D, H
        self.obs = rng.normal(size=(Ln, S, D)).astype(f)
        self.W_ih = (rng.uniform(-1, 1, (4 * H, D)) * 0.6).astype(f)
        self.W_hh = (rng.uniform(-1, 1, (4 * H, H)) * (0.25 / H)).astype(f)
        self.b_ih, self.b_hh = (rng.uniform(-0.3, 0.3, 4 * H).astype(f) for _ in range(2))
        self.h0, self.c0 = rng.uniform(-0.9, 0.9, (S, H)).astype(f), rng.normal(size=(S, H)).astype(f)
        self.starts = (rng.uniform(size=(Ln, S)) < 0.5).astype(np.uint8)
        self.starts[0, 0], self.starts[min(2, Ln - 1), 1], self.starts[Ln - 1, 2] = 1, 1, 1
        self.starts[:, S - 1] = 0                                  # one sequence without a start
        self.w_h = rng.normal(size=(Ln, S, H)).astype(f)           # the loss: sum of w_h * h over all steps, plus w_c * c of the last
        self.w_c = rng.normal(size=(S, H)).astype(f) * f(0.5)


def lstm64(sc, masked=True):
    """torch.nn.LSTM in float64 on the CPU, stepped as sb3-contrib's _process_sequence steps it: the state times 1 - episode_start in
    front of every step (masked=False: the starts ignored).  -> dict of h [L, S, H], the last c, the gradients of the loss with respect
    to W_ih, W_hh, b_ih, b_hh, and the magnitudes the bounds are made of."""
    import torch
    T64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    lstm = torch.nn.LSTM(sc.D, sc.H).double()
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(T64(sc.W_ih))
        lstm.weight_hh_l0.copy_(T64(sc.W_hh))
        lstm.bias_ih_l0.copy_(T64(sc.b_ih))
        lstm.bias_hh_l0.copy_(T64(sc.b_hh))
    h, c = T64(sc.h0)[None], T64(sc.c0)[None]
    hs, cs, cmax = [], [], float(np.abs(sc.c0).max())
    for l in range(sc.Ln):
        if masked:
            keep = 1.0 - T64(sc.starts[l])[None, :, None]
            h, c = keep * h, keep * c
        out, (h, c) = lstm(T64(sc.obs[l])[None], (h, c))
        c.retain_grad()
        cs.append(c)
        hs.append(out[0])
        cmax = max(cmax, float(c.detach().abs().max()))
    hs = torch.stack(hs)
    loss = (hs * T64(sc.w_h)).sum() + (c[0] * T64(sc.w_c)).sum()
    loss.backward()
    g = {k: getattr(lstm, k + "_l0").grad.numpy().copy() for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
    with torch.no_grad():
        amax = float((T64(sc.obs).reshape(-1, sc.D) @ lstm.weight_ih_l0.T + lstm.bias_ih_l0 + lstm.bias_hh_l0).abs().max()) + 0.25
    dmax = max(float(x.grad.abs().max()) for x in cs)
    return dict(h=hs.detach().numpy(), c_last=c[0].detach().numpy(), grads=g, cmax=cmax, amax=amax, dmax=dmax)


def chain32(sc, cell, cell_grad, use_starts=True):
    """The float32 chain the package runs, with NumPy float32 products in place of torch's: gx of all rows at once, then per step
    gh = h W_hh^T and `cell`; backward through time with `cell_grad` and the products' own gradients.
    cell(CellCase-like fields) -> (h, c, act); cell_grad(...) -> (d_gx, d_gh, d_c_prev)."""
    Ln, S, D, H = sc.Ln, sc.S, sc.D, sc.H
    bias = sc.b_ih + sc.b_hh
    gx = (sc.obs.reshape(Ln * S, D) @ sc.W_ih.T + bias).astype(f).reshape(Ln, S, 4 * H)
    h, c, steps = sc.h0, sc.c0, []
    for l in range(Ln):
        gh = (h @ sc.W_hh.T).astype(f)
        start = sc.starts[l] if use_starts else None
        h2, c2, act = cell(gx[l], gh, c, start)
        steps.append((h, c, start, act))
        h, c = h2, c2
    hs = np.stack([cell_h for cell_h in _collect_h(steps, h)])
    dW_ih, dW_hh, db = np.zeros_like(sc.W_ih), np.zeros_like(sc.W_hh), np.zeros(4 * H, dtype=f)
    dh_next, dc_next = np.zeros((S, H), dtype=f), sc.w_c.copy()
    for l in reversed(range(Ln)):
        h_prev, c_prev, start, act = steps[l]
        d_gx, d_gh, d_cp = cell_grad((sc.w_h[l] + dh_next).astype(f), dc_next, act, c_prev, start)
        dW_ih += d_gx.T @ sc.obs[l]
        db += d_gx.sum(axis=0)
        dW_hh += d_gh.T @ h_prev
        dh_next, dc_next = (d_gh @ sc.W_hh).astype(f), d_cp
    return dict(h=hs, c_last=c, grads=dict(weight_ih=dW_ih, weight_hh=dW_hh, bias_ih=db, bias_hh=db))


def _collect_h(steps, last_h):
    """h_1 .. h_L from the h_prev each step stored and the last output."""
    return [s[0] for s in steps[1:]] + [last_h]


def host_cell_fns(host):
    """(cell, cell_grad) for chain32 through the host build."""
    class _C:
        pass

    def cell(gx, gh, c_prev, start):
        c = _C()
        c.M, c.H = c_prev.shape
        c.gx, c.gh, c.c_prev, c.start = (None if x is None else np.ascontiguousarray(x) for x in (gx, gh, c_prev, start))
        o = host_cell(host, c)
        return o["h"][:c.M].copy(), o["c"][:c.M].copy(), o["act"][:c.M].copy()

    def cell_grad(dh, dc, act, c_prev, start):
        c = _C()
        c.M, c.H = c_prev.shape
        c.dh, c.dc, c.c_prev, c.start = (None if x is None else np.ascontiguousarray(x) for x in (dh, dc, c_prev, start))
        o = host_cell_grad(host, c, act)
        return tuple(o[k][:c.M].copy() for k in ("d_gx", "d_gh", "d_c_prev"))

    return cell, cell_grad


def sequence_bounds(sc, ref):
    """-> (forward bound on |h| and |c|, {gradient name: bound}) of the module docstring, from the float64 run's magnitudes."""
    A, Cmax = max(1.0, ref["amax"], ref["cmax"]), max(1.0, ref["cmax"])
    n_fwd = sc.Ln * (sc.D + sc.H + FWD_OPS)
    Ef = n_fwd * A * U
    R = sc.Ln * sc.S
    n_bwd = 4 * n_fwd * A + sc.Ln * (BWD_OPS + sc.H) + R
    da_max = ref["dmax"] * max(1.0, Cmax / 4.0)
    x = dict(weight_ih=max(1.0, float(np.abs(sc.obs).max())), weight_hh=1.0, bias_ih=1.0, bias_hh=1.0)
    return Ef, {k: R * x[k] * da_max * U * n_bwd for k in x}


def compare_sequence(got, ref, Ef, Eg):
    """-> {name: largest |difference| / its bound}."""
    out = dict(h=float(np.abs(got["h"] - ref["h"]).max()) / Ef, c_last=float(np.abs(got["c_last"] - ref["c_last"]).max()) / Ef)
    for k, b in Eg.items():
        out[k] = float(np.abs(got["grads"][k] - ref["grads"][k]).max()) / b
    return out


# ---- 0. the feature is there -----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_bound_and_declared(host):
    from gl_gym_amd import _lib as L
    header = (ROOT / "include" / "glgym.h").read_text()
    for name in ("glgym_lstm_cell", "glgym_lstm_cell_grad", "glgym_seq_batch"):
        assert name in L.PROTOTYPES and f"int {name}(glgym_handle h" in header
    assert "#define GLGYM_ABI_VERSION 7" in header and L.ABI_VERSION == 7
    assert [host.lstmhost_sizeof(i) for i in range(3)] == [C.sizeof(L.LstmCellArgs), C.sizeof(L.LstmCellGradArgs), C.sizeof(L.SeqBatchArgs)]
    assert L.SEQ_BATCH_WS_BYTES == 16384 and "is a SELECT" in header
    for n in (1, 255, 256, 257, 256 * L.LSTM_MAX_BLOCKS, 256 * L.LSTM_MAX_BLOCKS + 1, 2 ** 29):
        assert host.lstmhost_n_blocks(n) == min(-(-n // 256), L.LSTM_MAX_BLOCKS)
    import gl_gym_amd
    assert {"RecurrentPPO", "RecurrentCollector", "RecurrentHeads", "lstm_cell"} <= set(gl_gym_amd.__all__)
    makefile = (CSRC / "Makefile").read_text()
    assert "glgym_rppo" in makefile.split("TUS =")[1].splitlines()[0]


# ---- 1. the cell -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", CELL_HS)
@pytest.mark.parametrize("kind", START_KINDS)
def test_cell_forward_and_backward_match_numpy(host, H, kind):
    for M in CELL_MS:
        c = CellCase(M, H, kind, seed=M)
        got = host_cell(host, c)
        act = got["act"][:M].reshape(M, N_ACT, H)
        assert activations_ok(c, got["act"][:M], got["c"][:M]), (M, H, kind)
        h, cell = np_cell_given(c, act)
        check_rows(got, dict(h=h, c=cell, act=got["act"][:M]), M)
        # the activations handed in give the same call; act left out leaves it untouched and changes nothing else
        check_rows(host_cell(host, c, act_in=act), dict(h=h, c=cell, act=got["act"][:M]), M)
        check_rows(host_cell(host, c, want_act=False), dict(h=h, c=cell), M)
        for want_dc in (True, False):
            d_gx, d_gh, d_cp = np_cell_grad(c, act, want_dc)
            check_rows(host_cell_grad(host, c, act, want_dc), dict(d_gx=d_gx, d_gh=d_gh, d_c_prev=d_cp), M)


def test_a_reset_row_reads_neither_gh_nor_c_prev(host):
    """A NaN and an infinity in the state of an episode that has ended do not enter the next one -- by the select; the product with
    1 - start that sb3-contrib uses would hand them on (0 * NaN)."""
    M, H = 65, 3
    c = CellCase(M, H, "mixed", seed=5, poison=True)
    rows = np.flatnonzero(c.start)
    assert len(rows) >= 4 and not np.isfinite(c.c_prev[rows]).all() and not np.isfinite(c.gh[rows]).all()
    got = host_cell(host, c)
    assert np.isfinite(got["h"][:M]).all() and np.isfinite(got["c"][:M]).all() and np.isfinite(got["act"][:M]).all()
    clean = CellCase(M, H, "mixed", seed=5)
    ref = host_cell(host, clean)
    for k in ("h", "c", "act"):
        assert same_u32(got[k][:M], ref[k][:M]), k
    g = host_cell_grad(host, c, got["act"][:M])
    assert all(np.isfinite(g[k][:M]).all() for k in g)
    assert not g["d_gh"][:M][rows].any() and not g["d_c_prev"][:M][rows].any() and g["d_gx"][:M][rows].any()
    with np.errstate(all="ignore"):                               # the product form on the same rows is not finite
        assert not np.isfinite((f(1) - (c.start[:, None] != 0).astype(f)) * c.c_prev).all()


# ---- 2. sequences ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_dim", [1, 23, 24])
def test_seq_batch_rows_are_the_sequences_rows(host, in_dim):
    seed, draw_index, base = 0xABCDEF0123, 5, 9
    for B in (1, 3, 8):
        for Ln in (1, 2, 5):
            for n_chunk in (1, 3):
                for n_state in (0, 2, 4):
                    c = SeqCase(n_chunk * Ln, B, Ln, in_dim, n_state, seed=B + Ln)
                    N = c.n_seq
                    for S, offset in {(N, 0), (1, N - 1), (max(1, N // 2), N - max(1, N // 2))}:
                        stats = Ln * S > 1
                        got = host_seq(host, c, S, offset, seed=seed, draw_index=draw_index, draw_base=base, want_stats=stats)
                        check_seq(got, np_seq(c, S, offset, draw_index + base, seed, want_stats=stats), seq_rows(c, S))
    c = SeqCase(10, 8, 5, in_dim, 2)                               # optional outputs not asked for are not written
    lean = host_seq(host, c, 7, 3, seed=seed, want_index=False, want_stats=False)
    want = np_seq(c, 7, 3, 0, seed, want_stats=False)
    del want["mb_index"]
    check_seq(lean, want, seq_rows(c, 7))


@pytest.mark.parametrize("S", [1, 63, 64, 65, 257])
def test_seq_batch_minibatch_sizes_and_a_ragged_epoch(host, S):
    c = SeqCase(6, 100, 2, 23, 4, seed=S)                          # 300 sequences
    got = host_seq(host, c, S, 300 - S, seed=3, draw_index=1)
    check_seq(got, np_seq(c, S, 300 - S, 1, 3), seq_rows(c, S))
    if S == 64:                                                     # 64 + 64 + 64 + 64 + 44: every sequence once
        idx = []
        for o in range(0, c.n_seq, S):
            s = min(S, c.n_seq - o)
            g = host_seq(host, c, s, o, seed=3, draw_index=1)
            check_seq(g, np_seq(c, s, o, 1, 3), seq_rows(c, s))
            idx.append(g["mb_index"][:s])
        assert [len(i) for i in idx] == [64, 64, 64, 64, 44] and np.array_equal(np.sort(np.concatenate(idx)), np.arange(c.n_seq))


@pytest.mark.parametrize("in_dim", [1, 23])
def test_seq_batch_with_one_step_is_ppo_batch(host, ppohost, in_dim):
    c = SeqCase(40, 25, 1, in_dim, 0, seed=4)
    for M, offset in ((257, 300), (1000, 0), (2, 998)):
        seq = host_seq(host, c, M, offset, seed=8, draw_index=2, draw_base=1)
        flat = host_batch(ppohost, c, M, offset, seed=8, draw_index=2, draw_base=1)
        for k in list(BATCH_PAIRS) + ["mb_index"]:
            assert np.array_equal(seq[k].view(np.uint8), flat[k].view(np.uint8)), k
        assert same_f64(seq["adv_stats"][:2], flat["adv_stats"][:2])


@pytest.mark.parametrize("LS", [(1, 2), (5, 13), (2, 128), (4, 250)])
def test_seq_adv_stats_against_float64_numpy(host, LS):
    Ln, S = LS
    M = Ln * S
    c = SeqCase(2 * Ln, 150, Ln, 1, 0, seed=M)
    got = host_seq(host, c, S, 0, seed=8)
    adv = got["mb_adv"][:M].astype(np.float64)
    mean, sd = got["adv_stats"][:2]
    assert same_f64(got["adv_stats"][:2], np_adv_stats(got["mb_adv"][:M]))
    u = 2.0 ** -52
    S1, S2 = math.fsum(adv), math.fsum(adv * adv)
    e1, e2 = sum_bound(adv), sum_bound(adv * adv)
    assert abs(np_reduce(adv) - S1) <= e1 and abs(np_reduce(adv * adv) - S2) <= e2
    assert abs(mean - np.mean(adv)) <= e1 / M + 2 * u * abs(mean)
    var = np.var(adv, ddof=1)
    dv = (e2 + 2 * abs(S1) * e1 / M + 4 * u * S1 * S1 / M + 2 * u * S2) / (M - 1) + 4 * u * var
    true_sd = np.std(adv, ddof=1)
    assert abs(sd - true_sd) <= dv / (2 * true_sd) + 2 * u * true_sd


# ---- 3. against torch's LSTM in float64 --------------------------------------------------------------------------------------------------
def step_bounds(c, K=0):
    """One step on given gx, gh, c_prev (K = 0: no dot product in front) -> (bound on |h|, |c|; bound on the three gradients)."""
    A = max(1.0, float(np.abs(c.gx).max() + np.abs(c.gh).max()), float(np.abs(c.c_prev).max()) + 1.0)
    Cmax = max(1.0, float(np.abs(c.c_prev).max()))
    Ef = (K + FWD_OPS) * A * U
    Dmax = float(np.abs(c.dh).max() + np.abs(c.dc).max())
    return Ef, (4.0 * Ef + BWD_OPS * U) * Cmax * Dmax


def cell64(c, masked=True):
    """The LSTM step in float64 with autograd, the state times 1 - start as sb3-contrib has it -> h, c and the gradients of
    sum(h dh) + sum(c dc) with respect to gx, gh, c_prev."""
    import torch
    T64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    gx, gh, cp = T64(c.gx).requires_grad_(), T64(c.gh).requires_grad_(), T64(c.c_prev).requires_grad_()
    keep = T64(c.keep().astype(np.float64))[:, None] if masked else torch.ones(c.M, 1, dtype=torch.float64)
    i, fg, g, o = (gx + keep * gh).chunk(4, dim=1)
    cell = torch.sigmoid(fg) * (keep * cp) + torch.sigmoid(i) * torch.tanh(g)
    h = torch.sigmoid(o) * torch.tanh(cell)
    ((h * T64(c.dh)).sum() + (cell * T64(c.dc)).sum()).backward()
    return dict(h=h.detach().numpy(), c=cell.detach().numpy(), d_gx=gx.grad.numpy(), d_gh=gh.grad.numpy(), d_c_prev=cp.grad.numpy())


def test_the_float64_step_is_torchs_lstm():
    """A check of the ORACLE only (it runs nothing of the feature beyond this module's imports): cell64 above, the float64 step the
    host build is compared with, on gx = x W_ih^T + b_ih + b_hh, gh = h W_hh^T is torch.nn.LSTM's own step (to 1e-13) -- gate order and
    formulas.  test_one_step_against_float64_autograd then holds the host build against cell64."""
    import torch
    sc = SequenceCase(Ln=1, S=9)
    lstm = torch.nn.LSTM(sc.D, sc.H).double()
    T64 = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    with torch.no_grad():
        for k, v in (("weight_ih", sc.W_ih), ("weight_hh", sc.W_hh), ("bias_ih", sc.b_ih), ("bias_hh", sc.b_hh)):
            getattr(lstm, k + "_l0").copy_(T64(v))
        out, (h, c) = lstm(T64(sc.obs[0])[None], (T64(sc.h0)[None], T64(sc.c0)[None]))

    class _C:
        pass
    cc = _C()
    cc.M, cc.H = sc.S, sc.H
    cc.gx = sc.obs[0].astype(np.float64) @ sc.W_ih.T.astype(np.float64) + sc.b_ih.astype(np.float64) + sc.b_hh
    cc.gh = sc.h0.astype(np.float64) @ sc.W_hh.T.astype(np.float64)
    cc.c_prev, cc.dh, cc.dc = sc.c0, np.ones((sc.S, sc.H)), np.ones((sc.S, sc.H))
    cc.keep = lambda: np.ones(sc.S, dtype=bool)
    mine = cell64(cc)
    assert np.abs(mine["h"] - h[0].numpy()).max() < 1e-13 and np.abs(mine["c"] - c[0].numpy()).max() < 1e-13


def test_one_step_against_float64_autograd(host):
    """Values and the gradients with respect to gx, gh and c_prev of one step with starts, within step_bounds; the same comparison with the
    starts ignored on the float64 side misses every one of the five bounds (d_gx included: the activations of a reset row differ) by more
    than 100 times."""
    c = CellCase(257, 64, "mixed", seed=2)
    got = host_cell(host, c)
    grads = host_cell_grad(host, c, got["act"][:c.M])
    mine = dict(h=got["h"][:c.M], c=got["c"][:c.M], **{k: v[:c.M] for k, v in grads.items()})
    Ef, Eb = step_bounds(c)
    bound = dict(h=Ef, c=Ef, d_gx=Eb, d_gh=Eb, d_c_prev=Eb)
    for masked, verdict in ((True, "within"), (False, "misses")):
        ref = cell64(c, masked)
        ratio = {k: float(np.abs(mine[k].astype(np.float64) - ref[k]).max()) / bound[k] for k in bound}
        print(f"starts {'honoured' if masked else 'ignored'}: largest |float32 - float64| / bound = {ratio}")
        if masked:
            assert max(ratio.values()) <= 1.0, ratio
        else:
            assert min(ratio.values()) >= 100.0, ratio


def test_a_sequence_against_torchs_lstm_in_float64(host):
    """L = 5 steps with starts inside the sequences: every h, the last c and the gradients with respect to W_ih, W_hh and the two biases
    against torch.nn.LSTM in float64 stepped with sb3-contrib's masked state, within sequence_bounds; the same comparison against the
    float64 run that ignores the starts misses the bound of every quantity by more than 100 times."""
    sc = SequenceCase()
    assert sc.starts[1:].any() and abs(float(np.abs(sc.W_hh).sum(axis=1).max()) - 0.25) < 0.1
    cell, cell_grad = host_cell_fns(host)
    got = chain32(sc, cell, cell_grad)
    ref = lstm64(sc)
    Ef, Eg = sequence_bounds(sc, ref)
    ratio = compare_sequence(got, ref, Ef, Eg)
    print(f"forward bound {Ef:.2e}, gradient bounds { {k: f'{v:.2e}' for k, v in Eg.items()} }")
    print(f"largest |float32 - float64| / bound: {ratio}")
    assert max(ratio.values()) <= 1.0, ratio
    blind = compare_sequence(got, lstm64(sc, masked=False), Ef, Eg)
    print(f"the same with the starts ignored: {blind}")
    assert min(blind.values()) >= 100.0, blind
    # and the chain itself sees the starts: without them it is the unmasked LSTM, within the same bounds
    assert max(compare_sequence(chain32(sc, cell, cell_grad, use_starts=False), lstm64(sc, masked=False), Ef, Eg).values()) <= 1.0


# An entry that moves an output onto another output puts it INSIDE that output's span: on a device, where the buffers are real allocations,
# nothing of it can then lie on an input as well (inputs are looked at first).
# ---- 4. refusals without a device ------------------------------------------------------------------------------------------------------
P_ = 0x10000                                                  # a non-null pointer: never followed, nothing is launched
MB_ = 0x100000                                                # the distance between two of them
CELL_M, CELL_H = 130, 64
ROW = CELL_M * CELL_H * 4                                     # bytes of an [M][H] tensor


def good_cell_args():
    p = [P_ + k * MB_ for k in range(7)]
    return cell_args(CELL_M, CELL_H, *p)


def good_grad_args():
    p = [P_ + k * MB_ for k in range(8)]
    return grad_args(CELL_M, CELL_H, *p)


SEQ_GOOD = dict(T=20, B=26, L=4, S=40, offset=60, in_dim=23, n_state=2, state_dim=(64, 3))


def good_seq_args():
    from gl_gym_amd import _lib as L
    p = [P_ + k * MB_ for k in range(24)]
    g = SEQ_GOOD
    return L.make_plan_args(L.SeqBatchArgs, g["T"], g["B"], g["L"], g["S"], g["offset"], g["in_dim"], g["n_state"], (C.c_int32 * 4)(*g["state_dim"], 0, 0),
                            1, 0, None, p[0], p[1], p[2], p[3], p[4], p[5], p[6], (C.c_void_p * 4)(p[7], p[8], None, None), p[9], p[10], p[11],
                            p[12], p[13], p[14], p[15], (C.c_void_p * 4)(p[16], p[17], None, None), p[18], p[19], p[20], L.SEQ_BATCH_WS_BYTES)


CELL_REFUSALS = [("struct_size", 8, b"struct_size"), ("M", 0, b"M < 1"), ("M", -1, b"M < 1"), ("H", 0, b"H outside"), ("H", 1025, b"H outside"),
                 ("M", 2 ** 23, b"M * 4 H above"), ("gx", None, b"null gx"), ("gh", None, b"null gx"), ("c_prev", None, b"null gx"),
                 ("h", None, b"null h or c"), ("c", None, b"null h or c"), ("h", P_, b"overlaps an input"),
                 ("h", P_ + 4 * ROW - 4, b"overlaps an input"), ("c", P_ + MB_ + 4 * ROW - 4, b"overlaps an input"),
                 ("c", P_ + 2 * MB_ + ROW - 4, b"overlaps an input"), ("act", P_ + 3 * MB_ + CELL_M - 1, b"overlaps an input"),
                 ("c", P_ + 4 * MB_, b"overlaps another output"), ("h", P_ + 6 * MB_ + 8, b"overlaps another output"),
                 ("c", P_ + 6 * MB_ + 4 * ROW, b"overlaps another output")]
GRAD_REFUSALS = [("struct_size", 8, b"struct_size"), ("M", 0, b"M < 1"), ("H", 0, b"H outside"), ("H", 1025, b"H outside"),
                 ("M", 2 ** 23, b"M * 4 H above"), ("dh", None, b"null dh"), ("act", None, b"null dh"), ("c_prev", None, b"null dh"),
                 ("d_gx", None, b"null d_gx"), ("d_gh", None, b"null d_gx"), ("d_c_prev", None, b"null d_gx"),
                 ("d_gx", P_ + ROW - 4, b"overlaps an input"), ("d_gh", P_ + MB_, b"overlaps an input"),
                 ("d_c_prev", P_ + 2 * MB_ + 5 * ROW - 4, b"overlaps an input"), ("d_gx", P_ + 3 * MB_, b"overlaps an input"),
                 ("d_gh", P_ + 4 * MB_ + CELL_M - 1, b"overlaps an input"), ("d_gh", P_ + 5 * MB_, b"overlaps another output"),
                 ("d_c_prev", P_ + 6 * MB_ + ROW, b"overlaps another output"), ("d_c_prev", P_ + 5 * MB_ + 3 * ROW, b"overlaps another output")]
_R = 520                                                      # T * B of SEQ_GOOD, 130 sequences, 160 minibatch rows
SEQ_REFUSALS = [("struct_size", 8, b"struct_size"), ("T", 0, b"T or B < 1"), ("B", 0, b"T or B < 1"), ("L", 0, b"L < 1"), ("L", -2, b"L < 1"),
                ("L", 3, b"no multiple of L"), ("T", 21, b"no multiple of L"), ("T", 2 ** 31 - 4, b"2^31 - 256 transitions"), ("S", 0, b"S < 1"),
                ("offset", -1, b"offset < 0"), ("offset", 91, b"offset + S >"), ("S", 71, b"offset + S >"), ("in_dim", 0, b"in_dim outside"),
                ("in_dim", 1025, b"in_dim outside"), ("n_state", -1, b"n_state outside"), ("n_state", 5, b"n_state outside"),
                (("state_dim", 1), 0, b"state dimension outside"), (("state_dim", 0), 1025, b"state dimension outside"),
                (("state_src", 1), None, b"null state_src"), (("state_out", 0), None, b"null state_src"),
                ("obs", None, b"null obs"), ("action", None, b"null obs"), ("logp", None, b"null obs"), ("advantage", None, b"null obs"),
                ("returns", None, b"null obs"), ("value", None, b"null obs"), ("episode_starts", None, b"null obs"), ("mb_obs", None, b"null mb_obs"),
                ("mb_action", None, b"null mb_obs"), ("mb_logp", None, b"null mb_obs"), ("mb_adv", None, b"null mb_obs"),
                ("mb_ret", None, b"null mb_obs"), ("mb_value", None, b"null mb_obs"), ("mb_start", None, b"null mb_obs"),
                ("workspace", None, b"without a workspace"), ("workspace_bytes", 16383, b"workspace smaller"),
                ("mb_obs", P_ + _R * 23 * 4 - 4, b"overlaps a source"), ("mb_start", P_ + 6 * MB_ + _R - 1, b"overlaps a source"),
                (("state_out", 1), P_ + 8 * MB_ + 130 * 3 * 4 - 4, b"overlaps a source"), ("mb_index", P_ + 7 * MB_, b"overlaps a source"),
                ("adv_stats", P_ + 5 * MB_ + _R * 4 - 8, b"overlaps a source"), ("workspace", P_ + 4 * MB_, b"overlaps a source"),
                ("mb_action", P_ + 9 * MB_ + 4, b"overlaps another output"), ("mb_index", P_ + 9 * MB_ + 64, b"overlaps another output"),
                (("state_out", 1), P_ + 16 * MB_ + 16, b"overlaps another output"), ("mb_start", P_ + 14 * MB_ + 160 * 4 - 160, b"overlaps another output"),
                ("adv_stats", P_ + 20 * MB_ + 16384 - 8, b"overlaps another output")]


def refused(lib, fn, h, a, word):
    from gl_gym_amd import _lib as L
    assert fn(h, C.byref(a), None) == L.EINVAL
    msg = lib.glgym_last_error()
    assert msg and word in msg, (word, msg)


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every check happens before the handle is looked at: with good arguments and no handle the refusal names the handle, with a bad
    argument it names the argument."""
    import __graft_entry__ as g
    from gl_gym_amd import _lib as L
    if not L.LIB_PATH.exists():
        g.build()
    lib = L.load()
    for name, fn, good, table in (("glgym_lstm_cell", lib.glgym_lstm_cell, good_cell_args, CELL_REFUSALS),
                                  ("glgym_lstm_cell_grad", lib.glgym_lstm_cell_grad, good_grad_args, GRAD_REFUSALS),
                                  ("glgym_seq_batch", lib.glgym_seq_batch, good_seq_args, SEQ_REFUSALS)):
        refused(lib, fn, None, good(), name.encode() + b": null handle")
        for path, value, word in table:
            a = good()
            set_path(a, path, value)
            refused(lib, fn, None, a, word)
            assert name.encode() + b":" in lib.glgym_last_error(), (path, lib.glgym_last_error())
        assert fn(None, None, None) == L.EINVAL
    a = good_cell_args()                                          # the optional pointers left out
    a.start = a.act = None
    refused(lib, lib.glgym_lstm_cell, None, a, b"null handle")
    a = good_grad_args()
    a.dc = a.start = None
    refused(lib, lib.glgym_lstm_cell_grad, None, a, b"null handle")
    a = good_seq_args()
    a.L, a.S, a.offset = 1, 1, 0
    refused(lib, lib.glgym_seq_batch, None, a, b"adv_stats with L * S < 2")
    a.adv_stats = a.workspace = a.mb_index = None                 # without adv_stats neither the workspace nor two rows are asked for
    a.workspace_bytes = 0
    refused(lib, lib.glgym_seq_batch, None, a, b"null handle")
    a = good_seq_args()                                           # no states: their pointers and dimensions are not looked at
    a.n_state = 0
    a.state_dim[0], a.state_src[1], a.state_out[0] = 0, None, None
    a.S, a.offset = 130, 0
    refused(lib, lib.glgym_seq_batch, None, a, b"null handle")


def test_the_python_classes_refuse_what_is_out_of_scope():
    import torch
    import gl_gym_amd
    from gl_gym_amd import RecurrentCollector, RecurrentHeads, RecurrentPPO
    lin, log_std = torch.nn.Linear, torch.zeros(6)
    ok = torch.nn.LSTM(23, 8)
    for bad in (torch.nn.LSTM(23, 8, num_layers=2), torch.nn.LSTM(23, 8, bidirectional=True), torch.nn.LSTM(23, 8, proj_size=4)):
        with pytest.raises(NotImplementedError):
            RecurrentHeads(bad, lin(8, 6), lin(8, 1), log_std)
        with pytest.raises(NotImplementedError):
            RecurrentHeads(ok, lin(8, 6), lin(8, 1), log_std, lstm_vf=bad)
    with pytest.raises(TypeError):
        RecurrentHeads(torch.nn.GRU(23, 8), lin(8, 6), lin(8, 1), log_std)
    with pytest.raises(ValueError):
        RecurrentHeads(ok, lin(8, 6), lin(8, 1), log_std, lstm_vf=torch.nn.LSTM(23, 8), shared_lstm=True)
    with pytest.raises(ValueError):
        RecurrentHeads(ok, lin(8, 6), lin(8, 1), log_std, lstm_vf=torch.nn.LSTM(24, 8))
    assert [RecurrentHeads(ok, lin(8, 6), lin(8, 1), log_std, **kw).arrangement for kw in (dict(lstm_vf=torch.nn.LSTM(23, 4)), dict(shared_lstm=True), {})] \
        == ["separate", "shared", "actor_only"]
    heads = RecurrentHeads(ok, lin(8, 6), lin(23, 1), log_std)
    sd = {k: v.clone() for k, v in torch.nn.LSTM(23, 8).state_dict().items()}     # sb3-contrib's names load as they are
    assert set(sd) == {"weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"}
    heads.lstms["pi"].load_state_dict(sd)
    for kw in (dict(seq_len=0), dict(seq_len=3)):                 # the constructor's checks come before the environment is looked at
        with pytest.raises(ValueError):
            RecurrentCollector(None, 8, heads, **kw)
    with pytest.raises(TypeError):
        RecurrentCollector(None, 8, gl_gym_amd.TorchHeads(lin(23, 6), lin(23, 1), log_std), seq_len=4)

    class Col:
        T, B, D, device = 4, 130, 23, "cpu"
    for kw, exc in ((dict(target_kl=0.01), NotImplementedError), (dict(clip_range=lambda p: 0.2), NotImplementedError),
                    (dict(clip_range_vf=lambda p: 0.2), NotImplementedError), (dict(clip_range=0.0), ValueError),
                    (dict(clip_range_vf=-1.0), ValueError), ({}, TypeError)):
        with pytest.raises(exc):
            RecurrentPPO(Col(), None, **kw)
    with pytest.raises(NotImplementedError):                     # a recurrent SAC stays out of scope
        gl_gym_amd.SAC(None, None, None, None, None, recurrent=True)


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """tests/lstmhost/lstmhost.cpp with its own main, AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (nothing is
    loaded into Python): exactly sized heap buffers, so an index past a gate plane, a sequence's last step or a state row is reported."""
    exe = tmp_path / "lstmhost_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DLSTMHOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lstmhost ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
