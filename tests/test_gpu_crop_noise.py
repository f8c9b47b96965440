"""glgym_crop_noise (crop_noise_kernel) against test_controller_and_noise.expected_crop_noise, through ctypes on caller-owned buffers:
batches around the 256-thread block with ld = B + 7, seeds and draw indices whose high words are set, three scales, both handle dtypes.
The bound on a drawn entry is the project's 1.3e-7 relative (tests/test_gpu_parity.py): one float32 ulp for the contraction of
p + noise * p."""
import ctypes as C

import numpy as np
import pytest

import envlayer_inputs as E

pytestmark = pytest.mark.gpu

DRAWN = np.arange(34) != 16                    # row 16 (p144 = cLeafMax) is derived from rows 13 and 14
ULP32 = 2.0 ** -23


@pytest.fixture(scope="module")
def handles():
    hs = {False: E.Handle(False), True: E.Handle(True)}
    yield hs
    for h in hs.values():
        h.close()


def run_noise(hd, B, scale, seed, draw, ld=None, override=None, expect=0):
    """-> the whole SoA block [34, ld] as the call left it (0xFF bytes where it wrote nothing), guards checked."""
    ld = B + E.NOISE_PAD if ld is None else ld
    buf = E.Guarded(shape=(34, max(ld, 1)), dtype=hd.T)
    val = dict(crop_p=buf.ptr, B=B, ld=ld)
    val.update(override or {})
    hd.sync()
    rc = hd.lib.glgym_crop_noise(hd.h, val["crop_p"], val["B"], val["ld"], scale, seed, draw, hd.stream())
    hd.sync()
    assert rc == expect, (rc, hd.error())
    return buf.read()


def check_block(hd, blk, B, scale, seed, draw, what):
    pad = np.ascontiguousarray(blk[:, B:]).view(np.uint8)
    assert np.all(pad == 0xFF), f"{what}: a padding column was written"
    got = blk[:, :B]
    assert not np.isnan(got).any(), f"{what}: an entry was not written"
    g32 = got.astype(np.float32)
    assert np.array_equal(g32.astype(got.dtype), got), f"{what}: a value is not representable as float32"
    exp = E.crop_noise_reference(B, scale, seed, draw)
    rel = np.abs(g32.astype(np.float64) - exp) / np.abs(exp)
    print(f"{what}: drawn rows {rel[DRAWN].max():.3g} relative")
    assert rel[DRAWN].max() < 1.3e-7, (what, float(rel[DRAWN].max()))
    q = (g32[13] / g32[14]).astype(np.float64)                                    # the float quotient of the produced rows
    assert np.all(np.abs(g32[16] - q) <= np.spacing(np.abs(q).astype(np.float32))), f"{what}: cLeafMax is not laiMax / sla"
    if scale == 0.0:
        assert np.array_equal(g32[DRAWN], np.repeat(E.crop_p0()[DRAWN, None], B, axis=1)), f"{what}: scale 0 changed a parameter"
    return g32


CASES = [(s, d, sc) for s in E.NOISE_SEEDS for d in E.NOISE_DRAWS for sc in E.NOISE_SCALES]


@pytest.mark.parametrize("seed,draw,scale", CASES, ids=[f"seed{s:#x}-draw{d:#x}-scale{sc}" for s, d, sc in CASES])
def test_every_batch_against_the_definition(handles, seed, draw, scale):
    for B in E.NOISE_BATCHES:
        what = f"B={B}"
        g32 = check_block(handles[False], run_noise(handles[False], B, scale, seed, draw), B, scale, seed, draw, what + " f32")
        g64 = check_block(handles[True], run_noise(handles[True], B, scale, seed, draw), B, scale, seed, draw, what + " f64")
        assert np.array_equal(E.bits(g32), E.bits(g64)), f"{what}: the fp64 handle's block is not the fp32 handle's"
        if scale > 0 and B > 1:
            assert len(np.unique(g32[1])) > B // 2                               # the envs really differ


def test_high_words_of_draw_and_seed_separate_the_streams(handles):
    hd, B = handles[False], 257
    get = lambda seed, draw: run_noise(hd, B, 0.2, seed, draw)[:, :B][DRAWN]      # noqa: E731
    assert np.mean(get(4242, 2 ** 32 + 5) != get(4242, 5)) > 0.5
    hi = E.NOISE_SEEDS[1]
    assert hi >> 32 and np.mean(get(hi, 1) != get(hi & 0xFFFFFFFF, 1)) > 0.5
    assert np.mean(get(4242, 2 ** 40) != get(4242, 0)) > 0.5


REFUSALS = [("B", 0), ("B", -1), ("ld", 256), ("crop_p", None)]


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("field,value", REFUSALS, ids=[f"{f}={v}" for f, v in REFUSALS])
def test_refusals_write_nothing(handles, field, value, f64):
    hd = handles[f64]
    blk = run_noise(hd, 257, 0.2, 4242, 0, override={field: value}, expect=hd.L.EINVAL)
    assert np.all(np.ascontiguousarray(blk).view(np.uint8) == 0xFF)
    assert hd.lib.glgym_crop_noise(None, None, 1, 1, 0.2, 0, 0, None) == hd.L.EINVAL
