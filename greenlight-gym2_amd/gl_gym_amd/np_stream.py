"""Host side of rng="numpy": seeding and (un)packing of the per-environment PCG64 streams that csrc/glgym_rng.hip advances.

The reference's TomatoEnv draws everything random from ``gymnasium.utils.seeding.np_random(seed)`` =
``Generator(PCG64(SeedSequence(seed)))``, and environment ``rank`` of its ``make_vec_env`` is seeded with ``seed + rank``
(gl_gym/RL/utils.py:39).  ``seed_states(seeds)`` returns what ``np.random.PCG64(np.random.SeedSequence(s)).state`` holds for every
``s``, packed the way the device reads it: uint64 ``[5, n]`` = state low / high word, increment low / high word, buffer word
(``has_uint32 << 32 | uinteger``).

The plain loop over NumPy's own objects takes 21 us per seed -- 1.37 s for 65 536 environments, measured on one core of the build
machine's CPU, paid at construction and at every reseed -- so SeedSequence's entropy mixing and PCG64's seeding are restated here on
uint32 / uint64 arrays, one lane per seed (65 536 seeds: 0.21 s, most of it splitting the Python integers into words);
tests/test_np_stream_host.py holds them against NumPy's.  Seeds of more than 128 bits take the loop.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

NWORD = 5
_M32 = np.uint64(0xFFFFFFFF)
# numpy/random/bit_generator.pyx (SeedSequence) -- published constants of M. E. O'Neill's seed_seq_fe
_INIT_A, _MULT_A, _INIT_B, _MULT_B = 0x43B0D7E5, 0x931E8875, 0x8B51F9DD, 0x58F38DED
_MIX_L, _MIX_R, _XSHIFT, _POOL = 0xCA01F9DD, 0x4973F715, 16, 4
_PCG_MULT = (0x4385DF649FCCF645, 0x2360ED051FC65DA4)         # low, high word of PCG64's 128-bit multiplier


def _seed_words(seeds: Sequence[int]) -> np.ndarray:
    """uint32 [4, n]: the little-endian 32-bit words of each seed, zero-padded to the pool size (SeedSequence hashes a zero for
    every pool slot the entropy does not reach, so the padding changes nothing)."""
    s = [int(v) for v in seeds]
    if any(v < 0 for v in s):
        raise ValueError("seeds must be non-negative integers")
    return np.array([[(v >> (32 * k)) & 0xFFFFFFFF for v in s] for k in range(_POOL)], dtype=np.uint32).reshape(_POOL, len(s))


def seed_sequence_state(seeds: Sequence[int]) -> np.ndarray:
    """``SeedSequence(s).generate_state(4, np.uint64)`` for every s < 2^128 -> uint64 [4, n]."""
    ent = _seed_words(seeds)
    with np.errstate(over="ignore"):
        hc = [np.uint32(_INIT_A)]

        def hashmix(v):
            v = v ^ hc[0]
            hc[0] = np.uint32((int(hc[0]) * _MULT_A) & 0xFFFFFFFF)
            v = v * hc[0]
            return v ^ (v >> np.uint32(_XSHIFT))

        def mix(x, y):
            r = np.uint32(_MIX_L) * x - np.uint32(_MIX_R) * y
            return r ^ (r >> np.uint32(_XSHIFT))

        pool = [hashmix(ent[i]) for i in range(_POOL)]
        for i_src in range(_POOL):
            for i_dst in range(_POOL):
                if i_src != i_dst:
                    pool[i_dst] = mix(pool[i_dst], hashmix(pool[i_src]))
        hb, out = _INIT_B, []
        for i in range(8):                              # four uint64 = eight uint32, low word first
            v = pool[i % _POOL] ^ np.uint32(hb)
            hb = (hb * _MULT_B) & 0xFFFFFFFF
            v = v * np.uint32(hb)
            out.append((v ^ (v >> np.uint32(_XSHIFT))).astype(np.uint64))
    return np.stack([out[2 * k] | (out[2 * k + 1] << np.uint64(32)) for k in range(4)])


def _mulhi(a, b):
    a0, a1, b0, b1 = a & _M32, a >> np.uint64(32), b & _M32, b >> np.uint64(32)
    p00, p01, p10, p11 = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    mid = (p00 >> np.uint64(32)) + (p01 & _M32) + (p10 & _M32)
    return p11 + (p01 >> np.uint64(32)) + (p10 >> np.uint64(32)) + (mid >> np.uint64(32))


def _pcg_step(lo, hi, inc_lo, inc_hi):
    """state * MULT + inc (mod 2^128) on (low, high) uint64 arrays."""
    ml, mh = np.uint64(_PCG_MULT[0]), np.uint64(_PCG_MULT[1])
    nlo = lo * ml
    nhi = _mulhi(lo, ml) + hi * ml + lo * mh
    rlo = nlo + inc_lo
    return rlo, nhi + inc_hi + (rlo < nlo).astype(np.uint64)


def seed_states(seeds: Sequence[int]) -> np.ndarray:
    """Packed streams uint64 [5, n] of ``PCG64(SeedSequence(s))`` for every s in seeds."""
    seeds = [int(s) for s in seeds]
    if any(s >> 128 for s in seeds):
        return pack_states([np.random.PCG64(np.random.SeedSequence(s)).state for s in seeds])
    w = seed_sequence_state(seeds)              # PCG64 seeding: initstate = w0 << 64 | w1, initseq = w2 << 64 | w3
    with np.errstate(over="ignore"):
        inc_hi = (w[2] << np.uint64(1)) | (w[3] >> np.uint64(63))
        inc_lo = (w[3] << np.uint64(1)) | np.uint64(1)
        lo, hi = _pcg_step(np.zeros_like(inc_lo), np.zeros_like(inc_lo), inc_lo, inc_hi)
        lo2 = lo + w[1]
        hi = hi + w[0] + (lo2 < lo).astype(np.uint64)
        lo, hi = _pcg_step(lo2, hi, inc_lo, inc_hi)
    return np.stack([lo, hi, inc_lo, inc_hi, np.zeros_like(lo)])


def pack_states(states: Sequence[dict]) -> np.ndarray:
    """List of NumPy ``bit_generator.state`` dicts (PCG64) -> uint64 [5, n]."""
    out = np.zeros((NWORD, len(states)), dtype=np.uint64)
    m64 = (1 << 64) - 1
    for b, st in enumerate(states):
        if st.get("bit_generator") != "PCG64":
            raise ValueError(f"state {b}: expected a PCG64 bit_generator.state, got {st.get('bit_generator')!r}")
        s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
        out[:, b] = (s & m64, s >> 64, inc & m64, inc >> 64, (int(bool(st["has_uint32"])) << 32) | (int(st["uinteger"]) & 0xFFFFFFFF))
    return out


def unpack_states(words: np.ndarray) -> List[dict]:
    """uint64 [5, n] -> list of dicts that ``np.random.PCG64().state = d`` accepts."""
    w = np.asarray(words, dtype=np.uint64)
    cols = [[int(v) for v in row] for row in w]
    return [{"bit_generator": "PCG64", "state": {"state": (cols[1][b] << 64) | cols[0][b], "inc": (cols[3][b] << 64) | cols[2][b]},
             "has_uint32": (cols[4][b] >> 32) & 1, "uinteger": cols[4][b] & 0xFFFFFFFF} for b in range(w.shape[1])]
