"""Inputs and the NumPy restatement of glgym_plan_constrain, shared by tests/test_plan_constr_host.py (the host instantiation of
csrc/gl_constr.hpp) and tests/test_gpu_plan_constr.py (the kernels).  The restatement is written from the comment in include/glgym.h,
not from the .hpp: every product, quotient and sum below is one correctly rounded double operation, in the header's order.

Inputs.  viol[i][c] = scale_i * level_j * (1 + 0.05 u_c) * n_steps[c] with one level per CANDIDATE j: the runs of a candidate sit close
together, so that with the budgets at the median of the per-run measure about half of the candidates are within budget in every run,
however many runs there are -- both classes are populated (the tests assert it).  The padding of viol between C and ld is NaN: a read
past the children shows."""
import numpy as np

INF = float("inf")
PENALTY, FEASIBLE_FIRST = 0, 1


def children(P, O, K, S):
    """[P*K, O*S] child index of run r = o*S + s of candidate j = p*K + k: c = ((p*O + o)*K + k)*S + s."""
    return np.arange(P * O * K * S).reshape(P, O, K, S).transpose(0, 2, 1, 3).reshape(P * K, O * S)


def np_constrain(P, O, K, S, per_step, n_allow, mode, budget, weight, rho, ret, failed, viol, n_steps):
    """The header's definition -> dict(score, failed_out, feasible, excess, n_viol, n_feasible)."""
    J, R = P * K, O * S
    c = children(P, O, K, S)
    d = np.maximum(n_steps[c], 1).astype(np.float64) if per_step else np.ones((J, R))
    g = np.zeros((J, R))
    nonfinite = np.zeros(J, bool)
    for i in range(3):
        v = viol[i][c]
        if budget[i] == INF:
            e = np.zeros((J, R))                                          # off, whatever viol holds
        else:
            fin = np.isfinite(v)
            nonfinite |= ~fin.all(axis=1)
            with np.errstate(invalid="ignore"):
                x = v / d - np.float64(budget[i])
            e = np.where(fin & (x > 0.0), x, 0.0)
        g = g + np.float64(weight[i]) * e
    n_viol = (g > 0.0).sum(axis=1).astype(np.int32)
    feasible = (n_viol <= n_allow).astype(np.uint8)
    lanes = np.zeros((J, 64))                                             # lane l: runs l, l + 64, ... in ascending r, from 0.0
    for r0 in range(0, R, 64):
        n = min(64, R - r0)
        lanes[:, :n] = lanes[:, :n] + g[:, r0:r0 + n]
    total = np.zeros(J)
    for lane in range(64):                                                # the lane sums in lane order, from 0.0
        total = total + lanes[:, lane]
    G = total / np.float64(R)
    failed_out = ((failed != 0) | nonfinite | ~np.isfinite(ret)).astype(np.uint8)
    score = np.full(J, np.nan)
    n_feasible = np.zeros(P, np.int32)
    for p in range(P):
        rows = np.arange(p * K, (p + 1) * K)
        adm = failed_out[rows] == 0
        ok = adm & (feasible[rows] == 1)
        n_feasible[p] = ok.sum()
        if mode == PENALTY:
            s = ret[rows] - np.float64(rho) * G[rows]
        else:
            floor_p = (ret[rows][ok].min() if ok.any() else 0.0) - 1.0
            s = np.where(feasible[rows] == 1, ret[rows], floor_p - G[rows])
        score[rows] = np.where(adm, s, np.nan)
    return dict(score=score, failed_out=failed_out, feasible=feasible, excess=G, n_viol=n_viol, n_feasible=n_feasible)


def lexicographic_order(K, ret, feasible, excess, failed_out):
    """Per group: feasible candidates by return descending, then infeasible ones by excess ascending, ties to the lower k; failed last."""
    order = []
    for p in range(len(ret) // K):
        ks = range(p * K, (p + 1) * K)
        key = [(2, 0.0) if failed_out[j] else (0, -ret[j]) if feasible[j] else (1, excess[j]) for j in ks]
        order.append(sorted(range(K), key=lambda k: key[k]))               # sorted() is stable
    return np.array(order)


def make_case(seed, P, O, K, S, per_step=1, n_allow=0, mode=FEASIBLE_FIRST, rho=0.0, weight=(1.0, 1.0, 1.0), off=(), zero_steps=False,
              budget_scale=1.0):
    """Fixed-seed inputs of one shape; budgets at budget_scale x the median of the per-run measure; `off`: constraints with a +inf
    budget, which get infinite violations under them."""
    rng = np.random.default_rng(seed)
    J, R, C = P * K, O * S, P * O * K * S
    ld = C + 3
    c = children(P, O, K, S)
    n_steps = rng.integers(1, 9, size=C).astype(np.int32)
    if zero_steps:
        n_steps[rng.random(C) < 0.25] = 0
    level = rng.uniform(0.5, 1.5, size=J)
    viol = np.full((3, ld), np.nan)
    for i, scale in enumerate((40.0, 0.7, 3.0)):
        v = np.empty(C)
        v[c] = scale * level[:, None] * (1.0 + 0.05 * rng.random((J, R))) * np.maximum(n_steps[c], 1)
        viol[i, :C] = v
    d = np.maximum(n_steps, 1).astype(np.float64) if per_step else np.ones(C)
    budget = [float(np.median(viol[i, :C] / d)) * budget_scale for i in range(3)]
    for i in off:
        budget[i] = INF
        viol[i, :C][rng.random(C) < 0.3] = INF
    ret = np.round(rng.normal(size=J) * 100.0 * 64.0) / 64.0             # |ret| far below 2^20, exact ties possible
    failed = np.zeros(J, np.uint8)
    return dict(P=P, O=O, K=K, S=S, ld=ld, per_step=per_step, n_allow=n_allow, mode=mode, budget=budget, weight=list(weight), rho=rho,
                ret=ret, failed=failed, viol=viol, n_steps=n_steps)


def expect(case):
    return np_constrain(case["P"], case["O"], case["K"], case["S"], case["per_step"], case["n_allow"], case["mode"], case["budget"],
                        case["weight"], case["rho"], case["ret"], case["failed"], case["viol"], case["n_steps"])


def _cases():
    out = {}
    for R in (1, 3, 8, 9, 64, 65, 257):                                    # the lane-strided sum: one run .. several passes; 8 | 9: the
                                                                           # last shape of the lane-per-candidate kernel, the first of the other
        out[f"S{R}"] = make_case(10 + R, 2, 1, 3, R)
    out["O257"] = make_case(9, 1, 257, 4, 1)
    out["share_all"] = make_case(1, 1, 3, 5, 2)                            # the strided indexing of P = 1, O = B
    out["share_all_wave"] = make_case(2, 1, 5, 7, 2)                       # ... and in the wavefront-per-candidate kernel (R = 10)
    for K in (1, 63, 65, 257):                                             # across the 256 threads of the group's block
        out[f"K{K}"] = make_case(20 + K, 3, 1, K, 2)
    out["K65_wave"] = make_case(31, 3, 1, 65, 9)                           # 195 candidates in the wavefront-per-candidate kernel: a ragged block
    for n_allow in (0, 1, 4):
        out[f"allow{n_allow}"] = make_case(3, 2, 1, 6, 4, n_allow=n_allow)
    nf = make_case(4, 2, 1, 5, 2)                                          # group 1: nobody within budget, floor from 0.0
    nf["viol"][:, children(2, 1, 5, 2)[5:].ravel()] *= 100.0
    out["no_feasible_group"] = nf
    af = make_case(5, 3, 1, 4, 2)                                          # group 1 all failed: one by flag, one NaN, one inf, one viol
    af["failed"][4] = 1
    af["ret"][5], af["ret"][6] = np.nan, INF
    af["viol"][2, children(3, 1, 4, 2)[7, 1]] = np.nan
    out["all_failed_group"] = af
    out["inf_budget_inf_viol"] = make_case(6, 2, 1, 6, 3, off=(1,))
    out["zero_steps"] = make_case(7, 2, 1, 6, 3, zero_steps=True)
    out["per_total"] = make_case(8, 2, 1, 6, 3, per_step=0)
    out["penalty"] = make_case(11, 2, 1, 6, 3, mode=PENALTY, rho=2.5, weight=(0.01, 1.0, 0.25))
    out["penalty_rho0"] = make_case(12, 2, 1, 6, 3, mode=PENALTY, rho=0.0)
    out["all_off"] = make_case(13, 2, 1, 6, 3, off=(0, 1, 2))
    return out


CASES = _cases()
# both classes must be populated in these (the others pin one class on purpose or are too small to promise it)
BOTH_CLASSES = [n for n in CASES if n not in ("all_off", "penalty_rho0", "K1", "allow4")]
