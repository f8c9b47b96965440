"""CPU tests of closed-loop neural-policy rollouts: csrc/gl_mlp.hpp (host instantiation, tests/mlphost/mlphost.cpp -- a lane is a call)
against a NumPy float32 restatement written from the text of include/glgym.h; the refusals of glgym_policy_rows /
glgym_plan_rollout_policy through libglgym.so (no device: every check precedes the handle); the host side of
gl_gym_amd.planner.MLPSpec / PolicySearch.

Bounds.
* relu nets with squash "clip": EXACT (uint32 view).  Parameter indexing, scale, normalisation, the layers' sums and the clips are
  single correctly rounded float32 operations in a fixed order, which NumPy performs in the same order (np_forward below: one
  float32 product and one float32 sum per input, i ascending); fmax / fmin return the other operand for a NaN on both sides.
* tanh, silu and squash "tanh": the library's tanhf / expf are not NumPy's.  Truth is the float64 NumPy evaluation of the same
  float32 inputs; bound = max(4 x max|np32 - truth|, 2^-22), with np32 NumPy's own float32 evaluation -- never the code under test.
  Weights have the scale 1 / sqrt(fan_in), so that pre-activations stay moderate."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SRC = ROOT / "tests" / "mlphost" / "mlphost.cpp"
NU = 6
ACT = {"relu": 0, "tanh": 1, "silu": 2}
SQUASH = {"clip": 0, "tanh": 1}
CHILD, CANDIDATE = 0, 1
HIDDEN = [(), (1,), (5,), (8, 7, 64)]
IN_DIMS = [1, 23, 33]


def build_host(path):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.mlphost_sizeof.argtypes, lib.mlphost_sizeof.restype = [C.c_int], C.c_int
    lib.mlphost_net_error.argtypes, lib.mlphost_net_error.restype = [C.c_void_p, C.c_char_p, C.c_int], C.c_int
    lib.mlphost_n_params.argtypes, lib.mlphost_n_params.restype = [C.c_void_p], C.c_longlong
    lib.mlphost_buffer_rows.argtypes, lib.mlphost_buffer_rows.restype = [C.c_void_p], C.c_int
    lib.mlphost_policy_row.argtypes, lib.mlphost_policy_row.restype = [C.c_int] * 4, C.c_int
    lib.mlphost_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.mlphost_rows.restype = None
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_mlp.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    return build_host(tmp_path_factory.mktemp("mlphost") / "libmlphost.so")


# ---- the net of a test case, and its NumPy restatement ------------------------------------------------------------------------------
class Net:
    """in_dim, hidden, activation, squash, per-group scale [2 (n_hidden + 1)] f32, optional (mean, inv_std) f32 [in_dim] and clip_obs."""

    def __init__(self, in_dim, hidden, activation="relu", squash="clip", scale=None, norm=None, clip_obs=10.0):
        self.in_dim, self.hidden, self.activation, self.squash = in_dim, tuple(hidden), activation, squash
        sizes = (in_dim,) + self.hidden + (NU,)
        self.shapes = [(sizes[l + 1], sizes[l]) for l in range(len(sizes) - 1)]
        self.D = sum(o * (i + 1) for o, i in self.shapes)
        self.Ht = (self.D + NU - 1) // NU
        g = 2 * len(self.shapes)
        self.scale = np.ones(g, dtype=np.float32) if scale is None else np.asarray(scale, dtype=np.float32)
        assert self.scale.shape == (g,)
        self.mean, self.inv_std = (None, None) if norm is None else (np.ascontiguousarray(norm[0], dtype=np.float32),
                                                                     np.ascontiguousarray(norm[1], dtype=np.float32))
        self.clip_obs = np.float32(clip_obs)

    def struct(self, mean_ptr=None, inv_std_ptr=None):
        """The glgym_mlp_net; without pointers given, mean / inv_std point at this object's host arrays (the host instantiation)."""
        from gl_gym_amd import _lib as L
        n = L.MlpNet()
        n.in_dim, n.n_hidden, n.activation, n.squash = self.in_dim, len(self.hidden), ACT[self.activation], SQUASH[self.squash]
        for l, w in enumerate(self.hidden):
            n.width[l] = w
        for g in range(8):
            n.scale[g] = float(self.scale[g]) if g < len(self.scale) else 1.0
        n.clip_obs = float(self.clip_obs)
        if self.mean is not None:
            n.mean = self.mean.ctypes.data if mean_ptr is None else mean_ptr
            n.inv_std = self.inv_std.ctypes.data if inv_std_ptr is None else inv_std_ptr
        return n


def policy_rows(B, S, J, mode):
    """The row of theta child c reads: c / max(S, 1) in CHILD mode, (c / max(S, 1)) % J in CANDIDATE mode."""
    cand = np.arange(B) // max(S, 1)
    return cand % J if mode == CANDIDATE else cand


def flat_of(theta, D):
    """theta [Ht, J, 6] -> [J, D]: component i of row j is theta[i / 6][j][i % 6]."""
    Ht, J, _ = theta.shape
    out = np.empty((J, D), dtype=theta.dtype)
    for i in range(D):
        out[:, i] = theta[i // NU, :, i % NU]
    return out


def np_forward(net, obs, theta, J, S, mode, dtype=np.float32):
    """The actions [B, 6] from the header's text, in `dtype` (float32: the restatement; float64: the truth of the bounds)."""
    T = dtype
    B = len(obs)
    flat = flat_of(theta, net.D)[policy_rows(B, S, J, mode)].astype(T)             # [B, D]
    a = obs.astype(T)
    with np.errstate(all="ignore"):
        if net.mean is not None:
            c = T(net.clip_obs)
            a = np.fmin(np.fmax((a - net.mean.astype(T)) * net.inv_std.astype(T), -c), c)
        at = 0
        for l, (o, i) in enumerate(net.shapes):
            W = (T(net.scale[2 * l]) * flat[:, at:at + o * i]).reshape(B, o, i)
            at += o * i
            z = T(net.scale[2 * l + 1]) * flat[:, at:at + o]                         # z_o = bias_o
            at += o
            for k in range(i):                                                       # then for i ascending z_o = z_o + w_oi * a_i
                z = z + W[:, :, k] * a[:, k:k + 1]
            if l < len(net.shapes) - 1:
                if net.activation == "relu":
                    z = np.fmax(z, T(0))
                elif net.activation == "tanh":
                    z = np.tanh(z)
                else:
                    z = z / (T(1) + np.exp(-z))
            a = z
        assert at == net.D
        if net.squash == "tanh":
            a = np.tanh(a)
        return np.fmin(np.fmax(a, T(-1)), T(1)).astype(T)


def host_forward(host, net, obs, theta, J, S, mode):
    B = len(obs)
    obs, theta = np.ascontiguousarray(obs, dtype=np.float32), np.ascontiguousarray(theta, dtype=np.float32)
    assert theta.shape == (net.Ht, J, NU) and obs.shape == (B, net.in_dim)
    out = np.full((B, NU), np.nan, dtype=np.float32)
    n = net.struct()
    host.mlphost_rows(C.addressof(n), obs.ctypes.data, theta.ctypes.data, J, S, mode, B, out.ctypes.data)
    return out


def bound_of(net, obs, theta, J, S, mode):
    """(truth [B, 6] float64, the bound of the tanh / silu comparisons): max(4 x max|np32 - truth|, 2^-22)."""
    truth = np_forward(net, obs, theta, J, S, mode, np.float64)
    np32 = np_forward(net, obs, theta, J, S, mode, np.float32).astype(np.float64)
    return truth, max(4.0 * float(np.abs(np32 - truth).max()), 2.0 ** -22)


def make_case(in_dim, hidden, activation="relu", squash="clip", norm=False, J=5, B=None, seed=0, scales=True, nan=False):
    """A net with weights of scale 1 / sqrt(fan_in) (theta in [-1, 1] times that scale, or folded into theta with scales=False),
    J rows of theta with NaN in the padding, B rows of observations -> (net, obs, theta)."""
    rng = np.random.default_rng([seed, in_dim, len(hidden), J])
    sizes = (in_dim,) + tuple(hidden) + (NU,)
    fan = np.repeat([1.0 / np.sqrt(sizes[l]) for l in range(len(sizes) - 1)], 2)
    fan[1::2] = 0.5                                              # the biases' bound
    stats = (rng.uniform(-1, 1, in_dim), rng.uniform(0.5, 2.0, in_dim)) if norm else None
    net = Net(in_dim, hidden, activation, squash, scale=fan if scales else None, norm=stats, clip_obs=1.5)
    flat = rng.uniform(-1.0, 1.0, (J, net.Ht * NU)).astype(np.float32)
    if not scales:
        at = 0
        for l, (o, i) in enumerate(net.shapes):
            flat[:, at:at + o * i] *= np.float32(fan[2 * l])
            flat[:, at + o * i:at + o * (i + 1)] *= np.float32(0.5)
            at += o * (i + 1)
    flat[:, net.D:] = np.nan                                     # padding: never used
    B = J if B is None else B
    obs = rng.uniform(-2.0, 2.0, (B, in_dim)).astype(np.float32)
    if nan:                                                      # a NaN in a used entry of every other row, and in one observation
        flat[::2, rng.integers(0, net.D)] = np.nan
        flat[1, 0] = np.nan
        obs[B // 2, in_dim // 2] = np.nan
    theta = np.ascontiguousarray(flat.reshape(J, net.Ht, NU).transpose(1, 0, 2))
    return net, obs, theta


def same_u32(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


# ---- 0. the feature is there ----------------------------------------------------------------------------------------------------------
def test_the_symbols_are_bound_and_declared():
    from gl_gym_amd import _lib as L
    header = (ROOT / "include" / "glgym.h").read_text()
    for name in ("glgym_policy_rows", "glgym_plan_rollout_policy"):
        assert name in L.PROTOTYPES and f"int {name}(glgym_handle h" in header
    assert "GLGYM_POLICY_ROW_CHILD" in header and "GLGYM_POLICY_ROW_CANDIDATE" in header and "#define GLGYM_ABI_VERSION 7" in header
    assert (L.POLICY_ROW_CHILD, L.POLICY_ROW_CANDIDATE, L.ABI_VERSION) == (CHILD, CANDIDATE, 7)
    assert L.MLP_ACTIVATIONS == ACT and L.MLP_SQUASHES == SQUASH


def test_struct_sizes_and_parameter_counts(host):
    from gl_gym_amd import _lib as L
    from gl_gym_amd.planner import MLPSpec
    assert [host.mlphost_sizeof(i) for i in range(3)] == [C.sizeof(L.MlpNet), C.sizeof(L.PolicyRowsArgs), C.sizeof(L.PlanRolloutPolicyArgs)]
    for hidden in HIDDEN + [(64, 64, 64)]:
        for in_dim in IN_DIMS + [130, 1024]:
            net = Net(in_dim, hidden)
            n = net.struct()
            spec = MLPSpec(in_dim, hidden)
            assert host.mlphost_n_params(C.addressof(n)) == net.D == spec.D and spec.Ht == net.Ht
            assert host.mlphost_buffer_rows(C.addressof(n)) == max([min(in_dim, 64), 6] + list(hidden))
    import torch
    seq = torch.nn.Sequential(torch.nn.Linear(23, 8), torch.nn.Tanh(), torch.nn.Linear(8, 7), torch.nn.Tanh(), torch.nn.Linear(7, 6))
    assert torch.nn.utils.parameters_to_vector(seq.parameters()).numel() == Net(23, (8, 7)).D


# ---- 1. exact: relu nets, squash clip ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("in_dim", IN_DIMS + [130])
@pytest.mark.parametrize("hidden", HIDDEN, ids=str)
def test_relu_nets_are_exact(host, hidden, in_dim, norm):
    net, obs, theta = make_case(in_dim, hidden, norm=norm, J=7, nan=True)
    got = host_forward(host, net, obs, theta, 7, 0, CHILD)
    exp = np_forward(net, obs, theta, 7, 0, CHILD)
    assert same_u32(got, exp), np.abs(got - exp).max()
    assert not np.isnan(got).any() and (np.abs(got) <= 1).all()                     # no NaN reaches an action
    # without the NaNs: exact too, and the scale is a product of its own (folded into theta the bits differ somewhere, the values not)
    net, obs, theta = make_case(in_dim, hidden, norm=norm, J=7)
    got = host_forward(host, net, obs, theta, 7, 0, CHILD)
    assert same_u32(got, np_forward(net, obs, theta, 7, 0, CHILD))
    assert np.abs(got).min() < 1 and len(np.unique(got, axis=0)) == 7                # not all saturated, every row its own actions


def test_padding_is_ignored_and_components_are_where_the_header_says(host):
    net, obs, theta = make_case(33, (5,), J=4)                   # D = 206: Ht = 35, four padding entries
    assert (net.D, net.Ht) == (206, 35) and np.isnan(theta[-1, :, 2:]).all() and not np.isnan(theta[-1, :, :2]).any()
    ref = host_forward(host, net, obs, theta, 4, 0, CHILD)
    other = theta.copy()
    other[-1, :, 2:] = 1e30
    assert same_u32(host_forward(host, net, obs, other, 4, 0, CHILD), ref)
    # component i of row j is theta[i / 6][j][i % 6]: moving one used component of one row moves that row's actions and no other's
    for i in (0, 5, 6, 170, 171, 200, 205):                      # first / last weights of layer 0, its biases, the output layer's bias
        moved = theta.copy()
        moved[i // NU, 2, i % NU] += 0.75
        got = host_forward(host, net, obs, moved, 4, 0, CHILD)
        assert same_u32(got, np_forward(net, obs, moved, 4, 0, CHILD)), i
        assert same_u32(got[[0, 1, 3]], ref[[0, 1, 3]]), i
    out_bias = theta.copy()
    out_bias[205 // NU, 2, 205 % NU] += 0.25                     # the last component: the bias of action 5, scale 0.5
    got = host_forward(host, net, obs, out_bias, 4, 0, CHILD)
    assert same_u32(got[2, :5], ref[2, :5]) and got[2, 5] != ref[2, 5]


def test_scale_is_one_float32_product(host):
    net, obs, theta = make_case(23, (5,), J=3)
    net.scale[:] = [0.3, 0.7, 1.1, 0.9]                          # products that round
    got = host_forward(host, net, obs, theta, 3, 0, CHILD)
    assert same_u32(got, np_forward(net, obs, theta, 3, 0, CHILD))
    ones = Net(23, (5,))
    assert not same_u32(got, host_forward(host, ones, obs, theta, 3, 0, CHILD))


def test_normalisation_clips(host):
    net, obs, theta = make_case(23, (), norm=True, J=6)
    z = (obs - net.mean) * net.inv_std
    assert (np.abs(z) > net.clip_obs).any() and (np.abs(z) < net.clip_obs).any()       # both sides of clip_obs = 1.5 occur
    got = host_forward(host, net, obs, theta, 6, 0, CHILD)
    assert same_u32(got, np_forward(net, obs, theta, 6, 0, CHILD))
    raw = Net(23, (), scale=net.scale)
    assert not same_u32(got, host_forward(host, raw, obs, theta, 6, 0, CHILD))


# ---- 2. tanh / silu / squash tanh within the bound -----------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "norm"])
@pytest.mark.parametrize("activation,squash", [("tanh", "clip"), ("silu", "clip"), ("relu", "tanh"), ("tanh", "tanh"), ("silu", "tanh")])
@pytest.mark.parametrize("hidden,in_dim", [((), 23), ((1,), 1), ((5,), 33), ((8, 7, 64), 23), ((16,), 130)], ids=str)
def test_smooth_activations_within_the_bound(host, hidden, in_dim, activation, squash, norm):
    net, obs, theta = make_case(in_dim, hidden, activation, squash, norm=norm, J=9, seed=1)
    got = host_forward(host, net, obs, theta, 9, 0, CHILD).astype(np.float64)
    truth, bound = bound_of(net, obs, theta, 9, 0, CHILD)
    err = np.abs(got - truth).max()
    print(f"{hidden} in={in_dim} {activation}/{squash} norm={norm}: err {err:.3g} bound {bound:.3g}")
    assert err <= bound and bound < 1e-4
    assert np.abs(truth).max() > 0.05 and np.abs(truth).min() < 1                   # moderate pre-activations: the outputs are alive
    net, obs, theta = make_case(in_dim, hidden, activation, squash, norm=norm, J=9, seed=1, nan=True)
    got = host_forward(host, net, obs, theta, 9, 0, CHILD)
    assert not np.isnan(got).any() and (np.abs(got) <= 1).all()


# ---- 3. row modes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [0, 1, 3])
@pytest.mark.parametrize("mode", [CHILD, CANDIDATE], ids=["child", "candidate"])
def test_row_modes(host, mode, S):
    J, m = 4, max(S, 1)
    B = J * m - (1 if S == 3 else 0) if mode == CHILD else 3 * J * m + 2           # CANDIDATE: greenhouses share the J policies
    net, obs, theta = make_case(23, (5,), J=J, B=B, seed=2)
    rows = policy_rows(B, S, J, mode)
    assert [host.mlphost_policy_row(c, S, J, mode) for c in range(B)] == list(rows) and rows.max() == J - 1
    got = host_forward(host, net, obs, theta, J, S, mode)
    assert same_u32(got, np_forward(net, obs, theta, J, S, mode))
    same_obs = np.tile(obs[:1], (B, 1))                          # one observation everywhere: the action tells the row
    got = host_forward(host, net, same_obs, theta, J, S, mode)
    per_row = host_forward(host, net, same_obs[:J], theta, J, 0, CHILD)
    assert same_u32(got, per_row[rows]) and len(np.unique(per_row, axis=0)) == J
    one = host_forward(host, net, obs, theta[:, 2:3].copy(), 1, S, CANDIDATE)      # J = 1: one policy everywhere
    assert same_u32(one, np_forward(net, obs, np.repeat(theta[:, 2:3], J, axis=1), J, 0, CANDIDATE))


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def good_net(P_=None):
    net = Net(23, (16, 8), "tanh", "clip", scale=[0.5] * 6)
    n = net.struct()
    if P_:
        n.mean = n.inv_std = P_
        n.clip_obs = 10.0
    return n


NET_REFUSALS = [("in_dim", 0, b"in_dim"), ("in_dim", 1025, b"in_dim"), ("n_hidden", -1, b"n_hidden"), ("n_hidden", 4, b"n_hidden"),
                (("width", 0), 0, b"width"), (("width", 1), 65, b"width"), ("activation", 3, b"activation"), ("activation", -1, b"activation"),
                ("squash", 2, b"squash"), (("scale", 0), 0.0, b"scale"), (("scale", 5), -1.0, b"scale"), (("scale", 3), float("nan"), b"scale"),
                (("scale", 2), float("inf"), b"scale"), ("mean", None, b"exactly one"), ("inv_std", None, b"exactly one"),
                ("clip_obs", 0.0, b"clip_obs"), ("clip_obs", -1.0, b"clip_obs"), ("clip_obs", float("nan"), b"clip_obs"),
                ("clip_obs", float("inf"), b"clip_obs")]


def set_path(obj, path, value):
    path = path if isinstance(path, tuple) else (path,)
    for name in path[:-1]:
        obj = getattr(obj, name)
    if isinstance(path[-1], int):
        obj[path[-1]] = value
    else:
        setattr(obj, path[-1], value)


def test_net_refusals(host):
    n = good_net(0x1000)
    assert host.mlphost_net_error(C.addressof(n), None, 0) == 0
    for path, value, word in NET_REFUSALS:
        n = good_net(0x1000)
        set_path(n, path, value)
        msg = C.create_string_buffer(128)
        assert host.mlphost_net_error(C.addressof(n), msg, 128) == 1 and word in msg.value, (path, msg.value)
    n = good_net()                                               # without statistics clip_obs is not looked at; unused entries neither
    n.clip_obs, n.width[2], n.scale[6], n.scale[7] = 0.0, 999, 0.0, float("nan")
    assert host.mlphost_net_error(C.addressof(n), None, 0) == 0
    big = Net(1024, (64, 64, 64)).struct()                       # the largest net: 64 x 1025 + 2 x 64 x 65 + 6 x 65 = 74 310 parameters
    assert host.mlphost_net_error(C.addressof(big), None, 0) == 0 and host.mlphost_n_params(C.addressof(big)) == 74310


def test_entry_points_refuse_bad_arguments_without_a_device():
    """Every check happens before the handle is looked at: with good arguments and no handle the refusal names the handle, with a bad
    argument it names the argument."""
    import __graft_entry__ as g
    from gl_gym_amd import _lib as L
    if not L.LIB_PATH.exists():
        g.build()
    lib = L.load()
    P_ = 0x1000                                                  # a non-null pointer: never followed, nothing is launched

    def refused(fn, a, word):
        assert fn(None, C.byref(a), None) == L.EINVAL
        msg = lib.glgym_last_error()
        assert msg and word in msg, (word, msg)

    def rows(mode=CHILD):
        return L.make_plan_args(L.PolicyRowsArgs, 130, 44, 3, mode, good_net(P_), P_, P_, P_)

    for mode in (CHILD, CANDIDATE):
        refused(lib.glgym_policy_rows, rows(mode), b"null handle")
        for path, value, word in NET_REFUSALS:
            a = rows(mode)
            set_path(a.net, path, value)
            refused(lib.glgym_policy_rows, a, word)
            assert b"glgym_policy_rows: bad net" in lib.glgym_last_error()
        for path, value, word in (("struct_size", 8, b"struct_size"), ("theta", None, b"null obs, theta"), ("obs", None, b"null obs"),
                                  ("action", None, b"action"), ("B", 0, b"B < 1"), ("S", -1, b"S outside"), ("S", 257, b"S outside"),
                                  ("row_mode", 2, b"row_mode"), ("row_mode", -1, b"row_mode"), ("J", 0, b"J < 1")):
            a = rows(mode)
            set_path(a, path, value)
            refused(lib.glgym_policy_rows, a, word)
            assert b"glgym_policy_rows" in lib.glgym_last_error()
    for path, value in (("J", 43), ("S", 2), ("B", 133)):        # CHILD: B <= J * max(S, 1) ...
        a = rows(CHILD)
        set_path(a, path, value)
        refused(lib.glgym_policy_rows, a, b"B > J")
        a = rows(CANDIDATE)                                      # ... CANDIDATE: any B
        set_path(a, path, value)
        refused(lib.glgym_policy_rows, a, b"null handle")
    a = rows(CHILD)                                              # S = 0: one row of theta per row
    a.S, a.J = 0, 130
    refused(lib.glgym_policy_rows, a, b"null handle")
    a.J = 129
    refused(lib.glgym_policy_rows, a, b"B > J")
    a = rows(CANDIDATE)
    a.J = 1
    refused(lib.glgym_policy_rows, a, b"null handle")
    a.B = 2 ** 31 - 64
    refused(lib.glgym_policy_rows, a, b"null handle")
    a.B = 2 ** 31 - 63                                           # the last block's lane indices would wrap
    refused(lib.glgym_policy_rows, a, b"2^31 - 64 rows")
    assert lib.glgym_policy_rows(None, None, None) == L.EINVAL

    def roll(S=3, mode=CHILD):
        B = 30 if S else 6
        step = L.make_step_args(B, 64, P_, P_, None, None, P_, 100, P_, P_, P_ if S else None, 97, P_, P_, P_, None, P_)
        r = L.make_plan_args(L.PlanRolloutArgs, 3, 0.99, step, None, None, P_, P_, P_, P_, P_)
        J = (10 if S else 6) if mode == CHILD else (5 if S else 3)
        return L.make_plan_args(L.PlanRolloutPolicyArgs, 0, r, good_net(P_), P_, P_, P_, P_, 0, mode, J, 2, 5, S, 0, 0.2, 1, 0, None)

    for S in (3, 0):
        for mode in (CHILD, CANDIDATE):
            refused(lib.glgym_plan_rollout_policy, roll(S, mode), b"null handle")
            for path, value, word in NET_REFUSALS:
                a = roll(S, mode)
                set_path(a.net, path, value)
                refused(lib.glgym_plan_rollout_policy, a, word)
            for path, value, word in (("struct_size", 8, b"struct_size"), (("rollout", "struct_size"), 4, b"struct_size"),
                                      ("theta", None, b"null theta"), ("obs", None, b"obs"), ("actions", None, b"actions"),
                                      (("rollout", "actions"), P_, b"must be NULL"), (("rollout", "controls"), P_, b"must be NULL"),
                                      ("record", 2, b"record"), ("record", -1, b"record"), (("rollout", "H"), 0, b"H < 1"),
                                      (("rollout", "gamma"), -1.0, b"gamma"), (("rollout", "gamma"), float("nan"), b"gamma"),
                                      (("rollout", "gamma"), float("inf"), b"gamma"), ("Np", -1, b"Np outside"), ("Np", 129, b"Np outside"),
                                      ("S", 257, b"S outside"), ("S", -1, b"S outside"), ("row_mode", 2, b"row_mode"), ("J", 0, b"J < 1"),
                                      (("rollout", "step", "ld"), 5, b"step.ld"), (("rollout", "step", "B"), 0, b"step.B < 1"),
                                      ("start_day", None, b"start_day"), (("rollout", "ret"), None, b"accumulators"),
                                      (("rollout", "failed"), None, b"accumulators"), (("rollout", "step", "reward"), None, b"reward"),
                                      (("rollout", "step", "done"), None, b"done")):
                a = roll(S, mode)
                set_path(a, path, value)
                refused(lib.glgym_plan_rollout_policy, a, word)
                assert b"glgym_plan_rollout_policy" in lib.glgym_last_error()
    for mode in (CHILD, CANDIDATE):
        for path, value in ((("rollout", "step", "B"), 29), ("J", 30), ("J", 11 if mode == CHILD else 10), (("rollout", "step", "crop_p"), None),
                            ("hold", 2), ("scale", -0.5), ("scale", float("nan")), ("P", 0), (("rollout", "H"), 65537)):
            a = roll(3, mode)
            set_path(a, path, value)
            refused(lib.glgym_plan_rollout_policy, a, b"with scenarios")
    a = roll(3, CHILD)
    a.J = 9                                                      # fewer rows than candidates: the row check comes first
    refused(lib.glgym_plan_rollout_policy, a, b"B > J")
    a = roll(0, CHILD)                                           # without scenarios: step.B <= J, fewer children than rows are fine
    a.J = 5
    refused(lib.glgym_plan_rollout_policy, a, b"B > J")
    a.J = 60
    refused(lib.glgym_plan_rollout_policy, a, b"null handle")
    a = roll(0, CANDIDATE)                                       # ... P, K, hold, scale are not looked at, and a long horizon is fine
    a.P, a.hold, a.scale, a.rollout.H, a.J = 0, 7, -1.0, 70000, 1
    refused(lib.glgym_plan_rollout_policy, a, b"null handle")
    assert lib.glgym_plan_rollout_policy(None, None, None) == L.EINVAL


# ---- 5. the Python side without a device -----------------------------------------------------------------------------------------
def torch_net(in_dim, hidden, seed=0):
    import torch
    torch.manual_seed(seed)
    layers, last = [], in_dim
    for w in hidden:
        layers += [torch.nn.Linear(last, w), torch.nn.Tanh()]
        last = w
    layers.append(torch.nn.Linear(last, NU))
    return torch.nn.Sequential(*layers)


@pytest.mark.parametrize("hidden", [(), (16,), (8, 7, 64)], ids=str)
def test_encode_round_trips_a_torch_net_and_a_state_dict(host, hidden):
    import torch
    from gl_gym_amd.planner import MLPSpec
    seq = torch_net(23, hidden)
    spec = MLPSpec(23, hidden, activation="tanh")
    theta = spec.encode(seq)
    assert theta.shape == (spec.Ht, 1, NU) and theta.dtype == np.float32 and (theta.reshape(-1)[spec.D:] == 0).all()
    vec = torch.nn.utils.parameters_to_vector(seq.parameters()).detach().numpy()
    assert same_u32(spec.flat(theta)[0], vec)                    # exactly torch's own flat order at scale 1
    linears = [m for m in seq if isinstance(m, torch.nn.Linear)]
    for (W, b), m in zip(spec.decode(theta), linears):
        assert same_u32(W[0], m.weight.detach().numpy()) and same_u32(b[0], m.bias.detach().numpy())
    sd = {}
    for l, m in enumerate(linears[:-1]):
        sd[f"mlp_extractor.policy_net.{2 * l}.weight"], sd[f"mlp_extractor.policy_net.{2 * l}.bias"] = m.weight.detach(), m.bias.detach()
    sd["action_net.weight"], sd["action_net.bias"] = linears[-1].weight.detach(), linears[-1].bias.detach()
    sd["mlp_extractor.value_net.0.weight"] = torch.zeros(3, 3)   # other entries of an SB3 policy are not looked at
    assert same_u32(spec.encode(sd), theta)
    assert same_u32(spec.encode([(m.weight.detach().numpy(), m.bias.detach().numpy()) for m in linears]), theta)
    # the encoded net, run by the header, is the torch module (float32 sums in another order: 1e-5)
    obs = np.random.default_rng(0).uniform(-1, 1, (4, 23)).astype(np.float32)
    got = host_forward(host, Net(23, hidden, "tanh"), obs, np.repeat(theta, 4, axis=1), 4, 0, CHILD)
    with torch.no_grad():
        ref = seq(torch.from_numpy(obs)).clamp(-1, 1).numpy()
    assert np.abs(got - ref).max() < 1e-5
    # a scale divides on the way in and multiplies on the way out
    scaled = MLPSpec(23, hidden, scale=[0.5, 2.0] * (len(hidden) + 1))
    th = scaled.encode(seq)
    for (W, b), m in zip(scaled.decode(th), linears):            # powers of two: exact
        assert same_u32(W[0], m.weight.detach().numpy()) and same_u32(b[0], m.bias.detach().numpy())
    assert same_u32(scaled.flat(th)[0][:linears[0].weight.numel()], 2.0 * linears[0].weight.detach().numpy().reshape(-1))


def test_mlp_spec_argument_checks():
    import torch
    from gl_gym_amd.planner import MLPSpec, PolicySearch
    for kw in (dict(in_dim=0), dict(in_dim=1025), dict(hidden=(1, 2, 3, 4)), dict(hidden=(65,)), dict(hidden=(0,)), dict(activation="gelu"),
               dict(squash="sigmoid"), dict(scale=0.0), dict(scale=[1.0, 1.0]), dict(scale=float("inf")),
               dict(obs_norm=(np.zeros(22), np.ones(22), 1e-8, 10.0)), dict(obs_norm=(np.zeros(23), np.ones(23), 1e-8, 0.0)),
               dict(obs_norm=(np.zeros(23), -np.ones(23), 1e-8, 10.0))):
        with pytest.raises(ValueError):
            MLPSpec(**{"in_dim": 23, "hidden": (4,), **kw})
    spec = MLPSpec(23, (4,), obs_norm=(np.full(23, 0.1), np.full(23, 3.0), 1e-8, 10.0))
    assert spec.inv_std.dtype == np.float32 and spec.inv_std[0] == np.float32(1.0 / np.sqrt(3.0 + 1e-8)) and spec.mean[0] == np.float32(0.1)
    assert (spec.D, spec.Ht, spec.struct().n_hidden, spec.struct().clip_obs) == (4 * 24 + 6 * 5, 21, 1, 10.0)
    for wrong in (torch_net(22, (4,)), torch_net(23, (5,)), torch_net(23, ()), torch_net(23, (4, 4)),
                  [(np.zeros((4, 23)), np.zeros(4)), (np.zeros((6, 4)), np.zeros(5))],
                  {"action_net.weight": torch.zeros(6, 4), "action_net.bias": torch.zeros(6),
                   "mlp_extractor.policy_net.0.weight": torch.zeros(4, 22), "mlp_extractor.policy_net.0.bias": torch.zeros(4)}):
        with pytest.raises(ValueError):
            spec.encode(wrong)
    with pytest.raises(ValueError, match="no bias"):
        spec.encode(torch.nn.Sequential(torch.nn.Linear(23, 4, bias=False), torch.nn.Tanh(), torch.nn.Linear(4, 6)))
    # refused before the environment is touched
    with pytest.raises(ValueError, match="weather_sigma.*window"):
        PolicySearch(None, 4, 3, spec, n_scenarios=2, weather_sigma=[0.1] * 7)
    with pytest.raises(TypeError):
        PolicySearch(None, 4, 3, spec, crop="current")
    with pytest.raises(ValueError, match="share"):
        PolicySearch(None, 4, 3, spec, share="some")


def test_standalone_program_is_clean_under_the_sanitizers(tmp_path):
    """tests/mlphost/mlphost.cpp with its own main, AddressSanitizer + UndefinedBehaviorSanitizer, as a program of its own (nothing is
    loaded into Python): exactly sized heap buffers, so an index past a theta row, an observation row, a statistics vector or an
    activation buffer is reported."""
    exe = tmp_path / "mlphost_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DMLPHOST_MAIN", f"-I{CSRC}", f"-I{ROOT / 'include'}", "-o", str(exe), str(SRC)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mlphost ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
