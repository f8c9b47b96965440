"""glgym_plan_fork and glgym_plan_accumulate through the C ABI on guarded buffers of exactly the documented size, against
plan_inputs.fork_reference and plan_inputs.accumulate_step, bit for bit.  fork: batches of one lane, one short of / exactly / one past
a 256-thread block and a ragged third block; with a parent table (some parents unused, some repeated, four indices outside 0..P-1),
without one (C == P*K and C < P*K); every combination of the optional start_day and crop pairs.  accumulate: the same batches, alive
masks all / none / mixed, step_flags NULL or mixed, three weights, three calls in a row on the same accumulators.  Inputs are compared
before and after, padding columns and guards must keep their bytes.  Both handle dtypes."""
import numpy as np
import pytest

import plan_inputs as I

pytestmark = pytest.mark.gpu

SOA = (("x", I.NX), ("u", I.NU), ("crop", I.NCROP))


@pytest.fixture(scope="module")
def handles():
    hs = {False: I.Handle(False), True: I.Handle(True)}
    yield hs
    for h in hs.values():
        h.close()


def run_fork(hd, par, parent, C_, K, optional="both"):
    """One glgym_plan_fork -> {member: what the child buffers hold}, guards and inputs checked.  `optional`: which of the start_day /
    crop pointers are passed (plan_inputs.FORK_OPTIONAL)."""
    P, T = len(par["timestep"]), hd.T
    ldp, ldc = P + 3, C_ + I.PAD
    src = {f"{k}_parent": I.soa(par[k], ldp, T) for k, _ in SOA}
    src.update({f"{k}_parent": par[k] for k in ("timestep", "w_off", "start_day")})
    if parent is not None:
        src["parent"] = parent
    ins = I.guarded(src)
    outs = {k: I.Guarded(shape=(n, ldc), dtype=T) for k, n in SOA}
    outs.update(timestep=I.Guarded(shape=(C_,), dtype=np.int32), w_off=I.Guarded(shape=(C_,), dtype=np.int32),
                start_day=I.Guarded(shape=(C_,), dtype=np.float32), ret=I.Guarded(shape=(C_,), dtype=np.float64),
                viol=I.Guarded(shape=(3, ldc), dtype=np.float64), n_steps=I.Guarded(shape=(C_,), dtype=np.int32),
                alive=I.Guarded(shape=(C_,), dtype=np.uint8), failed=I.Guarded(shape=(C_,), dtype=np.uint8))
    p = {k: g.ptr for k, g in ins.items()}
    p.update({k: g.ptr for k, g in outs.items()})
    if optional in ("neither", "child_start_day_only"):
        p["start_day_parent"] = None
    if optional == "neither":
        p["start_day"] = None
    if optional in ("neither", "child_crop_only"):
        p["crop_parent"] = None
    if optional in ("neither", "parent_crop_only"):
        p["crop"] = None
    L = hd.L
    a = L.make_plan_args(L.PlanForkArgs, C_, P, K, ldp, ldc, p.get("parent"), p["x_parent"], p["u_parent"], p["timestep_parent"],
                         p["w_off_parent"], p["start_day_parent"], p["crop_parent"], p["x"], p["u"], p["timestep"], p["w_off"], p["start_day"],
                         p["crop"], p["ret"], p["viol"], p["n_steps"], p["alive"], p["failed"])
    I.launch(hd, "glgym_plan_fork", a)
    I.assert_only_read(ins, src)
    return {k: g.read() for k, g in outs.items()}


def check_fork(got, ref, C_, start_day=True, crop=True):
    for k in ("x", "u", "viol") + (("crop",) if crop else ()):
        assert np.array_equal(I.bits(got[k][:, :C_]), I.bits(ref[k])), k          # copies bit for bit; ret / viol +0.0 by their bits
        assert I.untouched_past(got[k], C_), f"{k}: a padding column was written"
    for k in ("timestep", "w_off", "ret", "n_steps", "alive", "failed") + (("start_day",) if start_day else ()):
        assert np.array_equal(I.bits(got[k]), I.bits(ref[k])), k
    if not start_day:
        assert I.untouched_past(got["start_day"], 0), "start_day was written without its pair"
    if not crop:
        assert I.untouched_past(got["crop"], 0), "crop was written without its pair"


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("C_,P,K", I.FORK_PLAIN)
def test_fork_without_a_table(handles, C_, P, K, f64):
    hd = handles[f64]
    par, _ = I.fork_case(C_, P)
    check_fork(run_fork(hd, par, None, C_, K), I.fork_reference(par, None, C_, K, hd.T), C_)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("C_,P,kind", I.FORK_TABLE)
def test_fork_with_a_parent_table(handles, C_, P, kind, f64):
    hd = handles[f64]
    par, parent = I.fork_case(C_, P, kind)
    got = run_fork(hd, par, parent, C_, 1)                                       # K is not used with a table
    ref = I.fork_reference(par, parent, C_, 1, hd.T)
    check_fork(got, ref, C_)
    if kind == "bad":                                                           # an index outside 0..P-1: parent 0, alive = 0, failed = 1
        at = list(I.FORK_BAD_AT)
        assert got["alive"][at].tolist() == [0] * 4 and got["failed"][at].tolist() == [1] * 4
        assert np.array_equal(I.bits(got["x"][:, at]), I.bits(np.repeat(par["x"].astype(hd.T)[0][:, None], 4, axis=1)))
        assert got["alive"].sum() == C_ - 4 and got["failed"].sum() == 4


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("optional", I.FORK_OPTIONAL)
def test_fork_optional_pairs(handles, optional, f64):
    hd, (C_, P, kind) = handles[f64], I.FORK_TABLE[3]
    par, parent = I.fork_case(C_, P, kind)
    got = run_fork(hd, par, parent, C_, 1, optional)
    check_fork(got, I.fork_reference(par, parent, C_, 1, hd.T), C_, start_day=optional not in ("neither", "child_start_day_only"),
               crop=optional not in ("neither", "child_crop_only", "parent_crop_only"))


# ---- accumulate ---------------------------------------------------------------------------------------------------------------------
class Accumulators:
    """The five accumulators of B children on the device, viol with NaN padding columns."""

    def __init__(self, prior, B):
        self.B, self.ld = B, B + I.PAD
        self.g = dict(ret=I.Guarded(prior["ret"]), viol=I.Guarded(I.soa(prior["viol"].T, self.ld, np.float64)), n_steps=I.Guarded(prior["n_steps"]),
                      alive=I.Guarded(prior["alive"]), failed=I.Guarded(prior["failed"]))

    def read(self):
        out = {k: g.read() for k, g in self.g.items()}
        assert np.isnan(out["viol"][:, self.B:]).all(), "viol: a padding column was written"
        out["viol"] = np.ascontiguousarray(out["viol"][:, :self.B])
        return out


def run_accumulate(hd, acc, w, reward, info, done, flags):
    """One glgym_plan_accumulate on the accumulators `acc`; reward / info are given as the handle's dtype stores them."""
    B, ld, T = acc.B, acc.ld, hd.T
    src = dict(reward=I.soa(reward[:, None], ld, T)[0], info=I.soa(info.T, ld, T), done=done)
    if flags is not None:
        src["step_flags"] = flags
    ins = I.guarded(src)
    L = hd.L
    a = L.make_plan_args(L.PlanAccumulateArgs, B, ld, w, ins["reward"].ptr, ins["info"].ptr, ins["done"].ptr,
                         ins["step_flags"].ptr if flags is not None else None, acc.g["ret"].ptr, acc.g["viol"].ptr, acc.g["n_steps"].ptr,
                         acc.g["alive"].ptr, acc.g["failed"].ptr)
    I.launch(hd, "glgym_plan_accumulate", a)
    I.assert_only_read(ins, src)
    return acc.read()


def rounded(hd, a):
    return a if hd.f64 else a.astype(np.float32).astype(np.float64)


def check_accumulate(got, exp, prior):
    for k in exp:
        assert np.array_equal(I.bits(got[k]), I.bits(exp[k])), k
    dead = prior["alive"] == 0
    for k in exp:
        assert np.array_equal(I.bits(got[k][..., dead]), I.bits(prior[k][..., dead])), f"{k}: a dead child's accumulator changed"
    assert (got["failed"] >= prior["failed"]).all(), "a child that had failed does not any more"


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("with_flags", [False, True], ids=["noflags", "flags"])
@pytest.mark.parametrize("alive_kind", I.ACC_ALIVE)
@pytest.mark.parametrize("B", I.ACC_BATCHES)
def test_accumulate_one_step(handles, B, alive_kind, with_flags, f64):
    hd = handles[f64]
    prior = I.accumulate_prior(B, alive_kind)
    reward, info, done, flags = I.accumulate_inputs(B, with_flags)
    reward, info = rounded(hd, reward), rounded(hd, info)
    for w in I.ACC_WEIGHTS:
        got = run_accumulate(hd, Accumulators(prior, B), w, reward, info, done, flags)
        check_accumulate(got, I.accumulate_step(prior, w, reward, info, done, flags), prior)
        if flags is None:
            assert np.array_equal(got["failed"], prior["failed"])
    if B > 1 and alive_kind == "mixed":
        assert 0 < prior["alive"].sum() < B and 0 < done.sum() < B and 0 < prior["failed"].sum() < B


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("B", I.ACC_BATCHES)
def test_accumulate_three_calls_with_the_running_product(handles, B, f64):
    hd = handles[f64]
    prior = I.accumulate_prior(B, "mixed" if B > 1 else "all")
    acc, w = Accumulators(prior, B), 1.0
    for call in range(3):
        reward, info, done, flags = I.accumulate_inputs(B, call != 1, seed=call)
        reward, info = rounded(hd, reward), rounded(hd, info)
        got = run_accumulate(hd, acc, w, reward, info, done, flags)
        exp = I.accumulate_step(prior, w, reward, info, done, flags)
        check_accumulate(got, exp, prior)
        prior, w = exp, w * 0.99
    assert w == 0.99 * 0.99 * 0.99
