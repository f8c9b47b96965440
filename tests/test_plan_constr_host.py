"""CPU tests of constrained ranking's scalar logic: csrc/gl_constr.hpp (host instantiation, tests/constrhost/constrhost.cpp -- the
candidate's wavefront a loop over 64 lanes, the group's workgroup a loop over its candidates) against the NumPy restatement of
tests/plan_constr_inputs.py, written from include/glgym.h.

Bounds.  EXACT (uint64 views of score and excess, equality of the integer outputs): every operation of the definition is a correctly
rounded double operation, the order of the excess sum is part of the definition, and NumPy performs the same operations in that order.
A NaN score is the canonical quiet NaN on both sides."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import plan_constr_inputs as I

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "greenlight-gym2_amd" / "csrc"
SRC = ROOT / "tests" / "constrhost" / "constrhost.cpp"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """csrc/gl_constr.hpp built with g++ (-ffp-contract=off as the other host instantiations)."""
    path = tmp_path_factory.mktemp("constrhost") / "libconstrhost.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                           "-o", str(path), str(SRC)])
    lib = C.CDLL(str(path))
    lib.constrhost_sizeof.argtypes, lib.constrhost_sizeof.restype = [], C.c_int
    lib.constrhost_constrain.argtypes = [C.c_int] * 8 + [C.c_void_p] * 2 + [C.c_double] + [C.c_void_p] * 10
    lib.constrhost_constrain.restype = None
    return lib


def run_host(host, case, alias_failed=False, optional=True):
    J, P = case["P"] * case["K"], case["P"]
    budget, weight = np.asarray(case["budget"], np.float64), np.asarray(case["weight"], np.float64)
    out = dict(score=np.full(J, -7.0), failed_out=case["failed"].copy() if alias_failed else np.full(J, 9, np.uint8),
               feasible=np.full(J, 9, np.uint8), excess=np.full(J, -7.0), n_viol=np.full(J, -7, np.int32),
               n_feasible=np.full(P, -7, np.int32))
    failed_in = out["failed_out"] if alias_failed else case["failed"]
    opt = [out[k].ctypes.data if optional else None for k in ("feasible", "excess", "n_viol", "n_feasible")]
    host.constrhost_constrain(case["P"], case["O"], case["K"], case["S"], case["ld"], case["per_step"], case["n_allow"], case["mode"],
                              budget.ctypes.data, weight.ctypes.data, float(case["rho"]), case["ret"].ctypes.data, failed_in.ctypes.data,
                              case["viol"].ctypes.data, case["n_steps"].ctypes.data, out["score"].ctypes.data,
                              out["failed_out"].ctypes.data, *opt)
    return out


def assert_same(got, want, keys=("score", "excess", "n_viol", "feasible", "failed_out", "n_feasible")):
    for k in keys:
        g, w = got[k], want[k]
        if g.dtype == np.float64:
            g, w = g.view(np.uint64), w.view(np.uint64)
        assert np.array_equal(g, w), (k, got[k], want[k])


def test_struct_size_matches_the_binding(host):
    from gl_gym_amd import _lib as L
    assert host.constrhost_sizeof() == C.sizeof(L.PlanConstrainArgs)
    assert L.CONSTRAIN_MODES == {"penalty": I.PENALTY, "feasible_first": I.FEASIBLE_FIRST}
    hdr = (ROOT / "include" / "glgym.h").read_text()
    assert "GLGYM_CONSTRAIN_PENALTY = 0, GLGYM_CONSTRAIN_FEASIBLE_FIRST = 1" in hdr


@pytest.mark.parametrize("name", list(I.CASES))
def test_host_instantiation_equals_the_restatement(host, name):
    case = I.CASES[name]
    want = I.expect(case)
    assert_same(run_host(host, case), want)
    assert_same(run_host(host, case, alias_failed=True, optional=False), want, keys=("score", "failed_out"))


@pytest.mark.parametrize("name", I.BOTH_CLASSES)
def test_inputs_populate_both_classes(name):
    want = I.expect(I.CASES[name])
    adm = want["failed_out"] == 0
    assert (adm & (want["feasible"] == 1)).any() and (adm & (want["feasible"] == 0)).any(), name


def test_the_special_cases_are_what_they_claim():
    e = I.expect(I.CASES["no_feasible_group"])
    assert e["n_feasible"][0] > 0 and e["n_feasible"][1] == 0
    c = I.CASES["no_feasible_group"]
    rows = slice(c["K"], 2 * c["K"])
    assert np.array_equal(e["score"][rows], (0.0 - 1.0) - e["excess"][rows])            # the floor comes from 0.0
    e = I.expect(I.CASES["all_failed_group"])
    assert e["failed_out"][4:8].all() and np.isnan(e["score"][4:8]).all() and e["n_feasible"][1] == 0
    assert not e["failed_out"][:4].any() and not e["failed_out"][8:].any()
    c = I.CASES["inf_budget_inf_viol"]
    assert np.isinf(c["viol"][1, :c["ld"] - 3]).any() and not I.expect(c)["failed_out"].any()
    assert (I.CASES["zero_steps"]["n_steps"] == 0).any()
    c = I.CASES["penalty_rho0"]
    assert np.array_equal(I.expect(c)["score"].view(np.uint64), c["ret"].view(np.uint64))
    c = I.CASES["all_off"]
    e = I.expect(c)
    assert np.array_equal(e["score"].view(np.uint64), c["ret"].view(np.uint64)) and e["feasible"].all() and not e["n_viol"].any()
    a0, a1, a4 = (I.expect(I.CASES[f"allow{n}"])["feasible"] for n in (0, 1, 4))
    assert a4.all() and (a0 <= a1).all() and not a0.all()


@pytest.mark.parametrize("name", ["K63", "K257", "allow1", "S65", "share_all"])
def test_scores_sort_into_the_lexicographic_order(host, name):
    """On inputs whose excess values are distinct and at least 2^-20, with |ret| < 2^20, a stable descending sort of the scores is:
    feasible first by return, then infeasible by ascending excess.  The two conditions are checked here, on the CPU, first."""
    case = I.CASES[name]
    assert case["mode"] == I.FEASIBLE_FIRST
    want = I.expect(case)
    K = case["K"]
    assert (np.abs(case["ret"]) < 2.0 ** 20).all() and not want["failed_out"].any()
    for p in range(case["P"]):
        ex = want["excess"][p * K:(p + 1) * K][want["feasible"][p * K:(p + 1) * K] == 0]
        assert len(np.unique(ex)) == len(ex) and (ex >= 2.0 ** -20).all()
    got = run_host(host, case)
    order = np.argsort(-got["score"].reshape(case["P"], K), axis=1, kind="stable")
    assert np.array_equal(order, I.lexicographic_order(K, case["ret"], want["feasible"], want["excess"], want["failed_out"]))


# ---- host-API checks that need no device ------------------------------------------------------------------------------------------
def test_constraints_validation():
    from gl_gym_amd.planner import Constraints
    c = Constraints(rh=2.0)
    assert c.budgets == (I.INF, I.INF, 2.0) and c.per == "step" and c.mode == "feasible_first" and c.n_allow == 0 and c.rho == 0.0
    assert c.weights == (1.0, 1.0, 1.0)
    assert Constraints(co2=0.0, temp=1.5, per="total", weights=(2, 0, 1), n_allow=3, mode="penalty", rho=4.0).budgets == (0.0, 1.5, I.INF)
    for bad in (dict(co2=-1.0), dict(temp=float("nan")), dict(rh="x"), dict(per="episode"), dict(mode="lagrange"),
                dict(weights=(1, 1)), dict(weights=(1, -1, 1)), dict(weights=(1, I.INF, 1)), dict(weights=3), dict(n_allow=-1),
                dict(n_allow=1.5), dict(rho=-0.1), dict(rho=I.INF), dict(rho=float("nan"))):
        with pytest.raises(ValueError):
            Constraints(**bad)


class _FakeTorch:
    """As much of torch as Planner.__init__ touches, on NumPy: the constructor allocates and takes views, nothing else."""
    float32, float64, int32, int64, uint8 = np.float32, np.float64, np.int32, np.int64, np.uint8

    @staticmethod
    def zeros(*shape, dtype=None, device=None):
        class T(np.ndarray):
            def view(self, *s):
                return self.reshape(*s)

            def t(self):
                return self.T
        return np.zeros(shape, dtype=dtype).view(T)


class _FakeEnv:
    torch, B, device, tdtype, crop_T, uncertainty_scale, nd = _FakeTorch, 2, "cpu", np.float32, None, 0.0, 10


def test_without_constraints_the_scores_are_the_returns():
    from gl_gym_amd.planner import Constraints, Planner
    p = Planner(_FakeEnv(), 4, 3)
    assert p.constraints is None and p._score_t is p.ret_t and p._score_failed_t is p.failed_t
    p = Planner(_FakeEnv(), 4, 3, n_scenarios=2)
    assert p._score_t is p.ret_cand_t and p._score_failed_t is p.failed_cand_t
    with pytest.raises(ValueError):
        Constraints(rh=1.0, n_allow=3).attach(Planner(_FakeEnv(), 4, 3, n_scenarios=2))               # n_allow > R = 2
    with pytest.raises(TypeError):
        Planner(_FakeEnv(), 4, 3)._constrain({"rh": 1.0})
