"""Inputs and references for the planning-kernel edge tests (tests/test_gpu_plan_fork_accumulate.py, test_gpu_plan_select_edges.py,
test_gpu_plan_cem_edges.py, test_gpu_plan_scen_edges.py) and their host check (tests/test_plan_inputs_host.py).

The references are the NumPy restatements the host tests already hold the g++ instantiations to (test_plan_host.np_accumulate /
np_select, test_plan_cem_host.np_sample / np_elites / np_refit, test_plan_scen_host.np_scen_crop / py_aggregate,
test_plan_wscen_host.np_wscen), imported; three are added where none existed: fork_reference, accumulate_step (np_accumulate from given
accumulators, step_flags optional) and np_sample (the imported one plus the two "not followed" rules of gl_cem.hpp::reserved).  The
builders are seeded; every parent, child and row gets values of its own, which the references assert once per case, so that a wrong
index cannot land on an equal value.

The shapes are the smallest at which each kernel's indexing changes: one lane, one short of / exactly / one past a 64-lane wavefront
and a 256-thread block, a ragged last block (700, 513, 520), the 256-key staging tile of the elite ranking (255, 256, 257, 513, 1000),
a horizon whose last group of four steps is full or holds one step (4, 5, 8, 9), and H*6 beyond the 64 lanes of the sequence gather.

Device side (envlayer_inputs): SoA inputs have ld = n + PAD with NaN in the padding columns; every buffer is a `Guarded` one of exactly
the documented size, outputs start as 0xFF bytes."""
import ctypes as C

import numpy as np

from envlayer_inputs import Guarded, Handle, assert_rows_distinct, bits, crop_p0, soa  # noqa: F401  (re-exported)
from test_plan_cem_host import F32_STEP, make_returns, np_elites, np_refit, within_one_f32_ulp  # noqa: F401
from test_plan_cem_host import np_sample as np_sample_valid
from test_plan_host import SF_FAILED, np_accumulate, np_select
from test_plan_scen_host import AGG_SHAPES, aggregate_case, np_scen_crop, np_scen_words, py_aggregate, same_f64  # noqa: F401
from test_plan_wscen_host import SIGMA, np_wscen, table  # noqa: F401

SEED, DRAW, BASE = 0xDEADBEEF12345678, (7 << 32) | 41, (3 << 32) | 5     # all three with a non-zero high word
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
PAD = 5                                                                  # ld = n + PAD
NX, NU, NCROP, NINFO = 28, 6, 34, 11
INFO_VIOL = (8, 7, 9)                                                    # info rows behind viol[0..2]: co2, temp, rh


def distinct(a, what):
    a = np.asarray(a).reshape(-1)
    assert len(np.unique(a)) == len(a), f"{what}: two entries are equal: a value read from the wrong place could pass"


# ---------------------------------------------------------------------------------------------------------------------------
# fork
# ---------------------------------------------------------------------------------------------------------------------------
FORK_PLAIN = [(1, 1, 1), (255, 5, 51), (256, 4, 64), (257, 1, 257), (700, 7, 100), (257, 3, 100)]       # (C, P, K); the last: C < P*K
FORK_TABLE = [(1, 2, "random"), (255, 6, "random"), (256, 6, "random"), (257, 6, "bad"), (700, 9, "random")]   # (C, P, kind)
FORK_BAD_AT = (0, 100, 255, 256)                                         # children of the "bad" table: -1, P, INT32_MIN, INT32_MAX
FORK_OPTIONAL = ("both", "neither", "child_start_day_only", "child_crop_only", "parent_crop_only")


def fork_case(C, P, kind=None, seed=0):
    """-> (parents: x [P, 28], u [P, 6], crop [P, 34], timestep, w_off [P] int32, start_day [P] float32; parent table [C] int32 or
    None).  kind "random": a seeded parent per child, parent 1 never used (P >= 3), the others repeated; "bad": the same with the four
    children FORK_BAD_AT carrying an index outside 0..P-1."""
    rng = np.random.default_rng([seed, C, P])
    par = dict(x=rng.uniform(1, 2, (P, NX)), u=rng.uniform(0, 1, (P, NU)), crop=rng.uniform(1, 2, (P, NCROP)),
               timestep=rng.permutation(5000)[:P].astype(np.int32), w_off=(rng.permutation(5000)[:P] - 2500).astype(np.int32),
               start_day=(rng.permutation(364)[:P] + rng.uniform(0, 0.5, P)).astype(np.float32))
    parent = None
    if kind is not None:
        used = np.arange(P) if P < 3 else np.delete(np.arange(P), 1)
        parent = used[rng.integers(0, len(used), C)].astype(np.int32)
        if C > P:
            assert len(np.unique(parent)) < C and (P < 3 or 1 not in parent)
        if kind == "bad":
            parent[list(FORK_BAD_AT)] = [-1, P, INT32_MIN, INT32_MAX]
    return par, parent


def fork_reference(par, parent, C, K, T):
    """What glgym_plan_fork leaves in the children, by plain indexing: the parent of child c is parent[c], or c // K without a table; an
    index outside 0..P-1 copies parent 0 and starts with alive = 0, failed = 1; the accumulators are +0.0 / 0.  SoA members as [n, C] of
    dtype T."""
    P = len(par["timestep"])
    for k in ("timestep", "w_off", "start_day"):
        distinct(par[k], k)
    assert_rows_distinct(np.concatenate([par["x"], par["u"], par["crop"]], axis=1).astype(T))
    for k in ("x", "u", "crop"):
        distinct(par[k].astype(T), k)
    idx = np.arange(C, dtype=np.int64) // K if parent is None else parent.astype(np.int64)
    bad = (idx < 0) | (idx >= P)
    src = np.where(bad, 0, idx)
    out = {k: np.ascontiguousarray(par[k].astype(T)[src].T) for k in ("x", "u", "crop")}
    out.update({k: par[k][src] for k in ("timestep", "w_off", "start_day")})
    out.update(ret=np.zeros(C), viol=np.zeros((3, C)), n_steps=np.zeros(C, np.int32), alive=(~bad).astype(np.uint8), failed=bad.astype(np.uint8))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# accumulate
# ---------------------------------------------------------------------------------------------------------------------------
ACC_BATCHES = (1, 255, 256, 257, 700)
ACC_ALIVE = ("all", "none", "mixed")
ACC_WEIGHTS = (1.0, 0.99 * 0.99, 0.0)


def accumulate_inputs(B, with_flags, seed=0):
    """One env-step's outputs for B children: reward [B], info [11, B] (float64; the test rounds them to the handle's dtype), done [B]
    mixed, step_flags [B] or None: some entries carry bit 128 among other bits, the others other bits only."""
    rng = np.random.default_rng([seed, B, 11])
    reward = rng.normal(size=B) * 10.0 ** rng.integers(-3, 3, B)
    info = rng.uniform(0.5, 1.5, (NINFO, B))
    done = (rng.random(B) < 0.4).astype(np.uint8)
    flags = None
    if with_flags:
        flags = np.where(rng.random(B) < 0.3, SF_FAILED | 3 | (5 << 16), rng.integers(0, 127, B) | (5 << 16)).astype(np.int32)
        flags[0] = SF_FAILED | 64
    distinct(reward, "reward"); distinct(info, "info")
    return reward, info, done, flags


def accumulate_prior(B, alive_kind, seed=0):
    """Accumulators found before the call: random, non-zero; some children have failed already."""
    rng = np.random.default_rng([seed, B, 12])
    alive = {"all": np.ones(B, np.uint8), "none": np.zeros(B, np.uint8), "mixed": (rng.random(B) < 0.6).astype(np.uint8)}[alive_kind]
    prior = dict(ret=rng.uniform(1, 2, B) * rng.choice([-1.0, 1.0], B), viol=rng.uniform(1, 2, (3, B)), n_steps=rng.integers(1, 50, B).astype(np.int32),
                 alive=alive, failed=(rng.random(B) < 0.2).astype(np.uint8))
    distinct(prior["ret"], "ret"); distinct(prior["viol"], "viol")
    return prior


def accumulate_step(prior, w, reward, info, done, flags=None):
    """np_accumulate for ONE step from the accumulators `prior` (dict ret, viol [3, B], n_steps, alive, failed): the increments of a
    child that is alive come from np_accumulate on zero accumulators (0.0 + w*reward is w*reward rounded once, the product the header
    asks to be rounded before the sum), a child that was dead keeps everything.  flags = None: failed is left alone."""
    B = len(reward)
    f = np.zeros(B, np.int32) if flags is None else flags
    d_ret, d_viol, d_n, d_alive, d_failed = np_accumulate(np.array([w]), reward[None], info[list(INFO_VIOL)][None], done[None], f[None])
    m = prior["alive"] != 0
    out = {k: v.copy() for k, v in prior.items()}
    out["ret"][m] = prior["ret"][m] + d_ret[m]
    out["viol"][:, m] = prior["viol"][:, m] + d_viol[:, m]
    out["n_steps"][m] += d_n[m]
    out["failed"][m] |= d_failed[m].astype(np.uint8)
    out["alive"][m] = d_alive[m].astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# select
# ---------------------------------------------------------------------------------------------------------------------------
# every K of {1, 63, 64, 65, 128, 129, 640} and every H of {1, 10, 11, 22, 48} (H*6 = 6, 60, 66, 132, 288 against 64 lanes), P in {1, 3}
SELECT_SHAPES = [(1, 1, 1), (3, 63, 10), (1, 64, 11), (3, 65, 22), (1, 128, 48), (3, 129, 11), (1, 640, 22), (3, 640, 1), (1, 65, 48),
                 (3, 64, 10), (1, 129, 22), (3, 128, 11)]
SELECT_PATTERNS = ("random", "last", "ties", "zeros", "failed", "nan")
SELECT_TEMPERATURES = (1e-300, 0.05, 1.0, 1e300)
SMALLEST_SUBNORMAL = 5e-324


def select_case(P, K, H, pattern, seed=0):
    """-> ret [P*K] float64, failed [P*K] uint8, actions [H, P*K, 6] float32 (no two rows alike).  Every parent starts from
    make_returns (ties, failures, NaN, infinities); pattern "last": the best at k = K-1; "ties": the maximum twice, at (63, 64) --
    two lanes -- or (5, 69) -- one lane -- in turn, (0, K-1) where K is too small; "zeros": -0.0 at a lower k against +0.0, everything
    else negative; "failed" / "nan": no admissible candidate."""
    rng = np.random.default_rng([seed, P, K, H])
    ret, failed = make_returns(rng, P, K)
    actions = rng.uniform(-1, 1, (H, P * K, NU)).astype(np.float32)
    assert_rows_distinct(actions.reshape(-1, NU))
    for p in range(P):
        r, f = ret[p * K:(p + 1) * K], failed[p * K:(p + 1) * K]
        fin = r[np.isfinite(r)]
        top = (fin.max() if len(fin) else 0.0) + 1.0 + p
        if pattern == "random" and K == 1:
            r[0], f[0] = 0.5, 0
        elif pattern == "last":
            r[K - 1], f[K - 1] = top, 0
        elif pattern == "ties":
            a, b = tie_pair(p, K)
            r[a] = r[b] = top
            f[a] = f[b] = 0
        elif pattern == "zeros":
            r[:] = -1.0 - rng.uniform(0, 1, K)
            lo, hi = K // 3, K - 1
            r[hi], f[hi] = 0.0, 0
            r[lo], f[lo] = -0.0, 0                                       # K = 1: -0.0 alone
        elif pattern == "failed":
            f[:] = 1
        elif pattern == "nan":
            r[:] = np.nan
    return ret, failed, actions


def tie_pair(p, K):
    want = (63, 64) if (p + K) % 2 == 0 else (5, 69)
    return want if want[1] < K else (0, K - 1)


def select_reference(P, K, ret, failed, actions, temperature=None):
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        return np_select(P, K, ret, failed, actions, temperature)


# ---------------------------------------------------------------------------------------------------------------------------
# sample
# ---------------------------------------------------------------------------------------------------------------------------
# (P, K, H, beta): P*K = 1, 63, 64, 65, 128, 129 (the last: wavefront 0 holds parent 0 and the first 21 children of parent 1); the
# horizon goes in groups of four steps: 1 and 3 a short only group, 4 and 8 full groups, 5 and 9 a last group of one step
SAMPLE_COMBOS = [(1, 1, 1, 0.0), (7, 9, 3, 0.5), (2, 32, 4, 0.95), (5, 13, 5, 0.0), (1, 128, 8, 0.5), (3, 43, 9, 0.95)]
SAMPLE_N_ELITE = (4, 1, 0, 9)                                            # prev_n_elite of parent p: entry p % 4


def sample_case(P, K, H, seed=0):
    """-> mean, std [H, P, 6] float32 (some means outside the box), prev_actions [H, P*K, 6] float32 (no two rows alike)."""
    rng = np.random.default_rng([seed, P, K, H, 1])
    mean = rng.uniform(-1.2, 1.2, (H, P, NU)).astype(np.float32)
    std = rng.uniform(0.05, 0.6, (H, P, NU)).astype(np.float32)
    prev = rng.uniform(-1, 1, (H, P * K, NU)).astype(np.float32)
    assert_rows_distinct(prev.reshape(-1, NU))
    distinct(mean, "mean"); distinct(std, "std")
    return mean, std, prev


def carry_tables(P, K, invalid, seed=0):
    """-> carry = prev_E (4; 2 at K = 1), prev_elite_k [P, prev_E], prev_n_elite [P] (SAMPLE_N_ELITE in turn).  invalid: every row holds
    one -1 (slot 0) and one K (slot 2; slot 1 at K = 1) among valid indices."""
    rng = np.random.default_rng([seed, P, K, 2])
    prev_E = 2 if K == 1 else 4
    elite = np.stack([rng.permutation(K)[:prev_E] if K >= prev_E else rng.integers(0, K, prev_E) for _ in range(P)]).astype(np.int32)
    if invalid:
        elite[:, 0], elite[:, prev_E // 2] = -1, K
    n_elite = np.array([SAMPLE_N_ELITE[p % 4] for p in range(P)], np.int32)
    return prev_E, elite, n_elite


def np_sample(P, K, H, mean, std, beta, seed, D, carry=0, prev_E=0, prev_actions=None, prev_elite_k=None, prev_n_elite=None):
    """test_plan_cem_host.np_sample with the two rules of gl_cem.hpp::reserved it leaves out: candidate 1 <= k <= carry copies elite k-1
    of the previous population only if k-1 < prev_n_elite[p] (and < prev_E) AND that elite index lies in 0..K-1; otherwise it is not
    followed: the candidate is sampled.  With valid tables it returns what the imported function returns.
    -> the block in float64 before the cast [H, P*K, 6], a mask [P*K] of the candidates that are copies or the clipped mean (exact)."""
    v, exact = np_sample_valid(P, K, H, mean, std, beta, seed, D)
    v, exact = v.reshape(H, P, K, NU), exact.reshape(P, K)
    for p in range(P):
        for k in range(1, min(carry, K - 1) + 1):
            if k - 1 < prev_E and k - 1 < prev_n_elite[p] and 0 <= prev_elite_k[p, k - 1] < K:
                v[:, p, k] = prev_actions[:, p * K + prev_elite_k[p, k - 1]]
                exact[p, k] = True
    return v.reshape(H, P * K, NU), exact.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
# elites
# ---------------------------------------------------------------------------------------------------------------------------
ELITE_SHAPES = [(1, 1, 1), (2, 64, 64), (3, 65, 1), (2, 255, 255), (2, 256, 17), (3, 257, 257), (2, 513, 300), (1, 1000, 1000)]
ELITE_PATTERNS = ("random", "equal", "increasing", "pairs", "none", "E-1", "E", "E+1")


def elites_case(P, K, E, pattern, seed=0):
    """-> ret [P*K], failed [P*K].  "equal": a whole parent of equal returns; "increasing": strictly increasing; "pairs": everything
    distinct but the keys on the 63|64 chunk boundary and the 255|256 tile boundary, which are equal pairs; "none": nothing admissible;
    "E-1" / "E" / "E+1": exactly that many admissible candidates (cut to 0..K), distinct returns."""
    rng = np.random.default_rng([seed, P, K, E])
    ret, failed = make_returns(rng, P, K)
    for p in range(P):
        r, f = ret[p * K:(p + 1) * K], failed[p * K:(p + 1) * K]
        if pattern == "random" and K == 1:
            r[0], f[0] = 0.5, 0
        elif pattern == "equal":
            r[:], f[:] = 1.5 + p, 0
        elif pattern == "increasing":
            r[:], f[:] = p + 0.25 * np.arange(K), 0
        elif pattern == "pairs":
            r[:], f[:] = p + 0.5 * rng.permutation(K), 0
            for a, b in ((63, 64), (255, 256)):
                if b < K:
                    r[b] = r[a]
        elif pattern == "none":
            f[:] = 1
        elif pattern in ("E-1", "E", "E+1"):
            n = min(max(E + {"E-1": -1, "E": 0, "E+1": 1}[pattern], 0), K)
            adm = rng.permutation(K)[:n]
            f[:] = 1
            f[adm], r[adm] = 0, 0.5 * rng.permutation(K)[:n] - p
    return ret, failed


# ---------------------------------------------------------------------------------------------------------------------------
# refit
# ---------------------------------------------------------------------------------------------------------------------------
REFIT_SHAPES = [(1, 1, 1, 1), (2, 65, 1, 65), (3, 70, 5, 7), (2, 300, 2, 300), (2, 129, 11, 100)]
REFIT_PARAMS = [(0.0, 0.0), (0.25, 0.05), (0.999, 10.0)]                 # (alpha, min_std)
REFIT_VARIANTS = ("full", "clamp", "invalid")


def refit_case(P, K, H, E, variant, seed=0):
    """-> actions [H, P*K, 6], elite_k [P, E], n_elite [P] as handed to the kernel, n_ref [P]: the count the reference uses (n_elite cut
    to 0..E; 0 for a parent that must be kept), mean, std [H, P, 6].
    "full": n_elite = E, 0, 2 by parent, and the elite rows of parent 0 are made identical (spread exactly 0).
    "clamp": n_elite = E + 5, -3, 1: read as E, 0, 1.  E + 5 sits on parent 0 of P >= 2 only, so that a count taken unclamped would read
    the next parent's row, inside the buffer.
    "invalid": parent 0 has a -1 among its first n entries, parent 1 a K: both are kept; parent 2 is refitted.
    Entries past n are -1."""
    rng = np.random.default_rng([seed, P, K, H, E])
    actions = np.clip(rng.normal(0, 0.6, (H, P * K, NU)), -1, 1).astype(np.float32)
    mean = rng.uniform(-1, 1, (H, P, NU)).astype(np.float32)
    std = rng.uniform(0.05, 0.6, (H, P, NU)).astype(np.float32)
    distinct(mean, "mean"); distinct(std, "std")
    elite = np.stack([rng.permutation(K)[:E] for _ in range(P)]).astype(np.int32)
    wanted = {"full": (E, 0, min(2, E)), "clamp": (E + 5 if P >= 2 else E, -3, 1), "invalid": (E, min(2, E), E)}[variant]
    n_elite = np.array(wanted[:P], np.int32)
    n_ref = np.clip(n_elite, 0, E)
    for p in range(P):
        elite[p, n_ref[p]:] = -1
    if variant == "invalid":
        elite[0, n_ref[0] // 2] = -1
        n_ref[0] = 0
        if P >= 2:
            elite[1, 0] = K
            n_ref[1] = 0
    if variant == "full":
        rows = elite[0, :n_ref[0]]
        actions[:, rows] = actions[:, rows[0]][:, None, :]
    return actions, elite, n_elite, n_ref, mean, std


def refit_reference(P, K, H, actions, elite, n_ref, alpha, min_std, mean, std):
    with np.errstate(invalid="ignore"):
        return np_refit(P, K, H, actions, elite, n_ref, alpha, min_std, mean, std)[:2]


# ---------------------------------------------------------------------------------------------------------------------------
# scenario, aggregate
# ---------------------------------------------------------------------------------------------------------------------------
SCEN_SHAPES = [(5, 17, 3), (4, 8, 8), (1, 257, 1), (3, 19, 9), (1, 2, 256)]            # (P, K, S): 255, 256, 257, 513, 512 children
# (h_step, hold, scale, action pair, draw_base): every h_step of {0, 1, 65535}, hold of {0, 1}, scale of {0, 0.2}, with and without
SCEN_CALLS = [(0, 0, 0.2, True, True), (1, 0, 0.2, False, False), (65535, 0, 0.2, True, False), (1, 1, 0.2, True, True),
              (65535, 1, 0.0, False, True)]


def scenario_reference(P, K, S, h, hold, scale, seed, D):
    """np_scen_crop [34, C] float32.  The K candidates of a greenhouse share their S futures by design; what must differ is checked
    here: no two (greenhouse, scenario) pairs draw the same words."""
    assert_rows_distinct(np_scen_words(P, S, h, hold, seed, D))
    return np_scen_crop(P, K, S, h, hold, scale, seed, D, crop_p0())


def scenario_actions(P, K, seed=0):
    a = np.random.default_rng([seed, P, K, 3]).uniform(-1, 1, (P * K, NU)).astype(np.float32)
    assert_rows_distinct(a)
    return a


# (J, S, m, kind) on top of test_plan_scen_host.AGG_SHAPES: m strictly between 2 and S, J = 1 and 70, a candidate of S equal returns,
# one with -0.0 and +0.0 tied
AGG_EDGES = [(6, 5, 3, "case"), (6, 64, 17, "case"), (6, 65, 64, "case"), (6, 256, 100, "case"), (1, 5, 3, "equal"), (1, 64, 17, "zeros"),
             (1, 256, 256, "plain"), (70, 5, 4, "case"), (70, 65, 3, "case"), (1, 1, 1, "zeros")]
AGG_CASES = [(6, S, m, "case") for S, m in AGG_SHAPES] + AGG_EDGES      # the present (S, m) list first


def aggregate_edge_case(J, S, m, kind, seed=0):
    """-> ret, failed, viol [3, ld], n_steps, ld.  "case": aggregate_case (J >= 6), with candidate 5 holding S equal returns and, where
    J = 70, candidate 6 the zeros of either sign; "equal" / "zeros" / "plain": J = 1."""
    rng = np.random.default_rng([seed, J, S, m])
    if kind == "case":
        ret, failed, viol, n_steps, ld = aggregate_case(rng, J, S)
        ret[5 * S:6 * S] = 2.5
        if J > 6 and S >= 2:
            ret[6 * S:7 * S] = np.where(np.arange(S) % 2 == 0, -0.0, 0.0)
        return ret, failed, viol, n_steps, ld
    n, ld = J * S, J * S + 3
    ret = {"equal": np.full(n, -1.25), "zeros": np.where(np.arange(n) % 2 == 0, 0.0, -0.0), "plain": rng.normal(size=n)}[kind]
    viol = np.zeros((3, ld))
    viol[:, :n] = rng.uniform(0.5, 1.5, (3, n))
    return ret, np.zeros(n, np.uint8), viol, rng.integers(1, 49, n).astype(np.int32), ld


# ---------------------------------------------------------------------------------------------------------------------------
# weather windows
# ---------------------------------------------------------------------------------------------------------------------------
# (P, S, H, K, nd, rows, first kind): 248, 256, 264, 520 and 2048 lanes; every H of {1, 2, 7}, K of {1, 3}, nd of {10, 14, 16}; one table
# of a single row
WEATHER_CASES = [(31, 1, 7, 3, 10, 40, 0), (4, 8, 2, 1, 14, 40, 0), (3, 11, 7, 3, 16, 40, 4), (5, 13, 1, 1, 14, 40, 0), (1, 256, 2, 3, 10, 40, 0),
                 (1, 256, 2, 1, 16, 40, 1), (4, 8, 7, 3, 14, 1, 0)]
WEATHER_KINDS = ("negative", "straddle", "beyond", "far", "generic")
PHI = 0.7


def weather_parents(P, H, rows, first=0):
    """-> w_off, timestep [P] int32, kinds.  Parent p is of kind WEATHER_KINDS[(p + first) % 5]: "negative": w_off + timestep = -3, the
    first steps read row 0; "straddle": the window runs over the end of the table; "beyond": it starts behind it; "far": a large negative
    timestep (the sum is small; the child offset is ps*H + 2^30); "generic": inside."""
    w_off, ts, kinds = np.zeros(P, np.int32), np.zeros(P, np.int32), []
    for p in range(P):
        kd = WEATHER_KINDS[(p + first) % 5]
        w_off[p], ts[p] = {"negative": (-50 - p, 47 + p), "straddle": (rows - 1 - H // 2 - p, p), "beyond": (rows + 9, p),
                           "far": (2 ** 30 + 7 + p, -2 ** 30), "generic": (3 + p % 7, 2 + p % 5)}[kd]
        kinds.append(kd)
    return w_off, ts, kinds


def weather_reference(P, K, S, H, weather, w_off, ts, phi, seed, D):
    assert_rows_distinct(weather)
    return np_wscen(P, K, S, H, weather, w_off, ts, SIGMA, phi, seed, D)


def sigma_array():
    return (C.c_double * 7)(*SIGMA)


# ---------------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------------
def guarded(src):
    """{name: host array} -> {name: Guarded}"""
    return {k: Guarded(v) for k, v in src.items()}


def assert_only_read(ins, src):
    """The inputs hold the bits they were given (and their guards are whole)."""
    for k, g in ins.items():
        assert np.array_equal(bits(g.read()), bits(np.ascontiguousarray(src[k]))), f"input {k} was written"


def draw_word(base):
    """draw_base: a device word holding BASE, or None -> (Guarded or None, pointer or None, value added to the draw index)."""
    if not base:
        return None, None, 0
    g = Guarded(np.array([BASE], np.uint64))
    return g, g.ptr, BASE


def launch(hd, name, a, expect=0):
    """One entry point on the handle's stream, synchronised on both sides; -> the refusal's text."""
    hd.sync()
    rc = getattr(hd.lib, name)(hd.h, C.byref(a), hd.stream())
    hd.sync()
    assert rc == expect, (name, rc, hd.error())
    return hd.error() if rc else ""


def untouched_past(got, n):
    """[.., ld] -> the columns past n still hold the 0xFF bytes the buffer started with."""
    tail = np.ascontiguousarray(got[..., n:])
    return bool(np.all(tail.reshape(-1).view(np.uint8) == 0xFF))
