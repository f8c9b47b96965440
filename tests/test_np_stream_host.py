"""CPU tests of rng="numpy": csrc/gl_pcg64.hpp (host instantiation, tests/pcg64host/pcg64host.cpp) and gl_gym_amd/np_stream.py against
NumPy itself.  Every comparison of random numbers and of generator states is EXACT.

Established with NumPy 2.2.6 (the pure-Python restatement below, test_pure_python_restatement_is_what_numpy_does):
  * PCG64 XSL-RR 128/64 + buffered 32-bit draws + Lemire's rejection method reproduce Generator.choice(list) and Generator.uniform;
  * choice of a one-element list draws nothing (the state does not move);
  * two choices in a row use ONE 64-bit draw (low half, then the buffered high half), and uniform leaves the buffer alone;
  * the fixture's un_p follows from seed 668 through float32(double(p) + noise * double(p)), p144 = p141 / p142 in float32.
"""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SEEDS = [0, 1, 666, 668, 2**31, 2**63 + 5]
M128, M64 = (1 << 128) - 1, (1 << 64) - 1


def np_gen(seed):               # gymnasium.utils.seeding.np_random
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))


def reference_flow(g, years, days, n_steps, scale, p32=None):
    """One episode of the reference's draws (tomato_env.py:236-241, then :118 per step) from generator g."""
    from oracle.gl_env_oracle import crop_noise
    y, d = g.choice(years), g.choice(days)
    blocks = []
    for _ in range(n_steps):
        if p32 is None:
            blocks.append(g.uniform(-scale / 2, scale / 2, size=34))
        else:
            blocks.append(crop_noise(p32, scale, g)[128:162])
    return y, d, blocks


class PyPcg64:
    """PCG64 as NumPy seeds and steps it, in Python integers."""
    MULT = 0x2360ED051FC65DA44385DF649FCCF645

    def __init__(self, seed):
        s = [int(v) for v in np.random.SeedSequence(seed).generate_state(4, np.uint64)]
        self.inc = (((s[2] << 64 | s[3]) << 1) | 1) & M128
        self.state = 0
        self.step()
        self.state = (self.state + (s[0] << 64 | s[1])) & M128
        self.step()
        self.has, self.u = 0, 0

    def step(self):
        self.state = (self.state * self.MULT + self.inc) & M128

    def u64(self):
        self.step()
        v, r = (self.state >> 64) ^ (self.state & M64), self.state >> 122
        return ((v >> r) | (v << ((-r) & 63))) & M64

    def u32(self):
        if self.has:
            self.has = 0
            return self.u
        n = self.u64()
        self.has, self.u = 1, n >> 32
        return n & 0xFFFFFFFF

    def dbl(self):
        return (self.u64() >> 11) * (1.0 / 9007199254740992.0)

    def bounded(self, n):
        if n == 1:
            return 0
        m = self.u32() * n
        if (m & 0xFFFFFFFF) < n:
            thr = (0xFFFFFFFF - (n - 1)) % n
            while (m & 0xFFFFFFFF) < thr:
                m = self.u32() * n
        return m >> 32

    def st(self):
        return {"bit_generator": "PCG64", "state": {"state": self.state, "inc": self.inc}, "has_uint32": self.has, "uinteger": self.u}


def test_pure_python_restatement_is_what_numpy_does():
    for seed in SEEDS:
        g, p = np_gen(seed), PyPcg64(seed)
        assert g.bit_generator.state == p.st()
        for n in (1, 2, 3, 20, 365):
            for _ in range(3):
                before = g.bit_generator.state
                y, d = g.choice(list(range(n))), g.choice(list(range(1000, 1000 + n)))
                if n == 1:
                    assert g.bit_generator.state == before
                assert (y, d - 1000) == (p.bounded(n), p.bounded(n)), (seed, n)
                for _ in range(5):
                    u = g.uniform(-0.1, 0.1, size=34)
                    assert np.array_equal(u, np.array([-0.1 + (0.1 - -0.1) * p.dbl() for _ in range(34)]))
            assert g.bit_generator.state == p.st()
        before = g.bit_generator.state["state"]["state"]
        g.choice([3, 4]), g.choice([5, 6, 7])
        assert g.bit_generator.state["state"]["state"] == (before * PyPcg64.MULT + p.inc) & M128      # one 64-bit draw for both


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_pcg64.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    from gl_gym_amd import np_stream as S
    so = tmp_path_factory.mktemp("pcg64host") / "libpcg64host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", "-o", str(so),
                           str(ROOT / "tests" / "pcg64host" / "pcg64host.cpp")])
    L = C.CDLL(str(so))
    u64p = C.POINTER(C.c_uint64)
    L.pcg64host_uint64.argtypes = [u64p, C.c_int, u64p]
    L.pcg64host_uint32.argtypes = [u64p, C.c_int, C.POINTER(C.c_uint32)]
    L.pcg64host_double.argtypes = [u64p, C.c_int, C.POINTER(C.c_double)]
    L.pcg64host_uniform.argtypes = [u64p, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_double)]
    L.pcg64host_bounded.argtypes, L.pcg64host_bounded.restype = [u64p, C.c_uint64], C.c_uint32
    L.pcg64host_advance.argtypes = [u64p, C.c_uint64]
    L.pcg64host_advance_step.argtypes = [u64p]
    L.pcg64host_crop_block.argtypes = [u64p, C.POINTER(C.c_float), C.c_double, C.POINTER(C.c_float)]

    class Stream:
        def __init__(self, seed):
            self.w = np.ascontiguousarray(S.seed_states([seed])[:, 0])
            self.p = self.w.ctypes.data_as(u64p)

        def state(self):
            return S.unpack_states(self.w.reshape(5, 1))[0]

        def uint64(self, n):
            out = np.empty(n, dtype=np.uint64)
            L.pcg64host_uint64(self.p, n, out.ctypes.data_as(u64p))
            return out

        def uint32(self, n):
            out = np.empty(n, dtype=np.uint32)
            L.pcg64host_uint32(self.p, n, out.ctypes.data_as(C.POINTER(C.c_uint32)))
            return out

        def double(self, n):
            out = np.empty(n)
            L.pcg64host_double(self.p, n, out.ctypes.data_as(C.POINTER(C.c_double)))
            return out

        def uniform(self, lo, hi, n):
            out = np.empty(n)
            L.pcg64host_uniform(self.p, lo, hi, n, out.ctypes.data_as(C.POINTER(C.c_double)))
            return out

        def bounded(self, n):
            return int(L.pcg64host_bounded(self.p, n))

        def advance(self, k):
            L.pcg64host_advance(self.p, k)

        def advance_step(self):
            L.pcg64host_advance_step(self.p)

        def crop_block(self, p0, scale):
            p0 = np.ascontiguousarray(p0, dtype=np.float32)
            out = np.empty(34, dtype=np.float32)
            L.pcg64host_crop_block(self.p, p0.ctypes.data_as(C.POINTER(C.c_float)), scale, out.ctypes.data_as(C.POINTER(C.c_float)))
            return out
    return Stream


def test_seeding_equals_numpys():
    """1. np_stream.seed_states (vectorised SeedSequence + PCG64 seeding) against PCG64(SeedSequence(s)).state."""
    from gl_gym_amd import np_stream as S
    seeds = SEEDS + [s + rank for s in (666, 2**63 + 5) for rank in range(64)] + [2**32 - 1, 2**32, 2**64 - 1, 2**64, 2**96 + 7,
                                                                                   2**128 - 1, 2**128, 2**200 + 11]
    want = [np.random.PCG64(np.random.SeedSequence(s)).state for s in seeds]
    assert S.unpack_states(S.seed_states(seeds)) == want
    assert S.unpack_states(S.seed_states(seeds[:7])) == want[:7]                 # the vectorised path alone (all below 2^128)
    ss = S.seed_sequence_state(seeds[:-2])
    for k, s in enumerate(seeds[:-2]):
        assert np.array_equal(ss[:, k], np.random.SeedSequence(s).generate_state(4, np.uint64)), s
    assert np.array_equal(S.pack_states(want), S.seed_states(seeds))
    with pytest.raises(ValueError):
        S.seed_states([-1])
    with pytest.raises(ValueError):
        S.pack_states([np.random.MT19937(1).state])


def test_state_after_seeding_round_trips_through_the_header(host):
    for seed in SEEDS + [668 + rank for rank in range(64)]:
        s = host(seed)
        assert s.state() == np_gen(seed).bit_generator.state
        s.uint64(0)
        assert s.state() == np_gen(seed).bit_generator.state


@pytest.mark.parametrize("seed", SEEDS)
def test_ten_thousand_draws_equal_numpys(host, seed):
    """2. next_uint64 / next_double / next_uint32, values and final state (buffer word included)."""
    g, s = np_gen(seed), host(seed)
    assert np.array_equal(s.uint64(10000), g.bit_generator.random_raw(10000))
    assert np.array_equal(s.double(10000), g.random(10000))
    assert s.state() == g.bit_generator.state
    u32 = s.uint32(10001)                 # odd count: the high half of the last draw stays buffered
    raw = g.bit_generator.random_raw(5001)
    want = np.stack([raw & np.uint64(0xFFFFFFFF), raw >> np.uint64(32)], axis=1).reshape(-1)[:10001]
    assert np.array_equal(u32, want.astype(np.uint32))
    st = s.state()
    assert st["has_uint32"] == 1 and st["uinteger"] == int(raw[-1] >> np.uint64(32)) and st["state"] == g.bit_generator.state["state"]
    # the same through NumPy's own buffered 32-bit path (integers of dtype uint32 over the full range)
    g2, s2 = np_gen(seed), host(seed)
    assert np.array_equal(s2.uint32(10001), g2.integers(0, 2**32, size=10001, dtype=np.uint32))


@pytest.mark.parametrize("n", [1, 2, 3, 20, 365])
@pytest.mark.parametrize("seed", SEEDS)
def test_interleaved_reference_flow(host, seed, n):
    """3. choice(years), choice(days), 5 x 34 uniforms, three episodes: every value and the final state."""
    g, s = np_gen(seed), host(seed)
    years, days = list(range(2000, 2000 + n)), list(range(100, 100 + n))
    for _ in range(3):
        y, d, blocks = reference_flow(g, years, days, 5, 0.2)
        assert (years[s.bounded(n)], days[s.bounded(n)]) == (y, d)
        for blk in blocks:
            assert np.array_equal(s.uniform(-0.1, 0.1, 34), blk)
    assert s.state() == g.bit_generator.state


def test_bounded_on_mixed_list_lengths_and_the_full_range(host):
    g, s = np_gen(12345), host(12345)
    for n in [7, 1, 2**31 + 3, 2, 365, 3, 2**32 - 1, 2**32, 20] * 50:
        assert s.bounded(n) == int(g.integers(0, n)), n
    assert s.state() == g.bit_generator.state


@pytest.mark.parametrize("seed", SEEDS)
def test_advance_equals_discarded_draws(host, seed):
    """4. advance(34) -- through the general constants and through the compile-time ones of the kernel -- equals 34 discarded draws,
    and leaves a buffered 32-bit word alone, as 34 uniforms do."""
    for k in (0, 1, 34, 1000):
        a, b = host(seed), host(seed)
        a.bounded(3)
        b.bounded(3)
        a.advance(k)
        b.double(k)
        assert a.state() == b.state(), k
    a, b, g = host(seed), host(seed), np_gen(seed)
    a.advance_step()
    b.uint64(34)
    g.uniform(-0.0, 0.0, size=34)
    assert a.state() == b.state() == g.bit_generator.state


def test_crop_block_equals_the_fixture_and_the_oracle(host, golden):
    """5. the crop block from seed 668 equals un_p[0..7] of tests/golden/refenv_1day.npz (the reference's own TomatoEnv) bit for
    bit, and oracle.gl_env_oracle.crop_noise on fresh seeds and scales."""
    from gl_gym_amd.parameters import init_default_params
    from oracle.gl_env_oracle import crop_noise
    g = golden("refenv_1day")
    un_p = g["un_p"]
    p32 = np.asarray(g["p"], dtype=np.float32) if "p" in g.files else np.asarray(init_default_params(208), dtype=np.float32)
    s = host(668)
    assert (s.bounded(1), s.bounded(1)) == (0, 0)            # one train year, one train day: nothing drawn
    assert un_p.shape[0] == 8
    for k in range(un_p.shape[0]):
        blk = s.crop_block(p32[128:162], 0.2)
        assert np.array_equal(blk.astype(np.float64), un_p[k][128:162]), k
    for seed in (3, 17, 2**40 + 1):
        for scale in (0.05, 0.2, 1.0, 0.0):
            gn, s = np_gen(seed), host(seed)
            for _ in range(20):
                assert np.array_equal(s.crop_block(p32[128:162], scale), crop_noise(p32, scale, gn)[128:162]), (seed, scale)
            assert s.state() == gn.bit_generator.state


def test_stream_abi_is_declared_bound_and_refuses_null_arguments():
    """6. header, _lib.PROTOTYPES and the library agree on the two new entry points; the ABI version did not move."""
    import __graft_entry__ as g
    from gl_gym_amd import _lib
    if not _lib.LIB_PATH.exists():
        g.build()
    hdr = (ROOT / "include" / "glgym.h").read_text()
    L = _lib.load()
    for name in ("glgym_rng_crop_noise", "glgym_rng_reset_draw"):
        assert re.search(rf"\bint {name}\s*\(", hdr), name
        assert getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
    assert _lib.ABI_VERSION == 7 == L.glgym_abi_version()
    assert L.glgym_rng_crop_noise(None, None, 1, 64, 0.2, None, None) == _lib.EINVAL
    assert L.glgym_rng_reset_draw(None, 1, 64, None, None, 1, 1, None, None, None, None, None) == _lib.EINVAL
    from gl_gym_amd import np_stream as S
    assert S.NWORD == int(re.search(r"uint64 \[(\d)\]\[ld\]", hdr).group(1)) == 5


def test_rng_argument_is_validated_before_the_device():
    from gl_gym_amd.tomato_env import _check_rng
    assert _check_rng("philox", None, 3) == ("philox", None)
    assert _check_rng("numpy", None, 7) == ("numpy", (1, 7))
    assert _check_rng("numpy", (3, 20), 60) == ("numpy", (3, 20))
    for bad in (("pcg", None, 1), ("numpy", (3, 20), 59), ("numpy", (0, 5), 0), ("philox", (1, 2, 3), 6)):
        with pytest.raises(ValueError):
            _check_rng(*bad)
