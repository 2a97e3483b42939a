"""sg_resample_u8 against the fp64 reference of tests/resample_refs.py.

fp32 output: |got - ref| <= (2 taps + 4) 2^-23 in normalised units (resample_refs.f32_tolerance).  uint8 output: equal to
round_half_even(clip(ref)) wherever the fp64 value is farther than 2e-3 from a half-integer, +-1 on the rest, and the near-tie
pixels (counted from the reference alone) are at most 2 % of a case (resample_refs.check_u8).  Pixels whose weights are all small
dyadic fractions (a 2:1 reduction, a replicated pixel) are held to the stricter rule instead: fp32 is exact there, so a tie is a
true tie and must round half to even; they do not count as near ties (resample_refs.exact_pixels)."""
import numpy as np
import pytest
import torch

from tests import margins
from tests import resample_refs as RR

pytestmark = pytest.mark.gpu

MODES = [RR.LINEAR, RR.AREA, RR.CUBIC]
MODE_IDS = ["linear", "area", "cubic"]
CANARY_U8, CANARY_F32 = 0x5C, 12345.0


def _rand(seed, h, w, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w), dtype=np.uint8)


def pack(images, pad_byte=0, gap=0):
    """Source buffer with every row padded to 16 bytes by pad_byte and `gap` (a multiple of 16) bytes of pad_byte between images."""
    strides = [(im.shape[1] + 15) & ~15 for im in images]
    offsets, at = [], gap
    for im, st in zip(images, strides):
        offsets.append(at)
        at += im.shape[0] * st + gap
    buf = np.full(at + 16, pad_byte, np.uint8)
    for im, st, off in zip(images, strides, offsets):
        h, w = im.shape
        buf[off:off + h * st].reshape(h, st)[:, :w] = im
    return torch.from_numpy(buf), np.array(offsets, np.int64), np.array(strides, np.int64)


def launch(dev, images, geo, mode, kind, fill=255, pad_byte=0, gap=0, order=None, out_gap=0):
    """geo: [(dh, dw, canvas_w)] per image.  -> (per-image [dh, canvas_w] arrays, the whole output buffer, the regions' mask)."""
    from scrabble_gan_amd import ops
    src, offsets, strides = pack(images, pad_byte, gap)
    n = len(images)
    order = list(range(n)) if order is None else order
    dst, at = [0] * n, out_gap
    for k in order:
        dst[k] = at
        at += (geo[k][0] * geo[k][2] + out_gap + 15) & ~15
    total = (at + 16 + 15) & ~15
    desc = ops.resample_desc(offsets, strides, [im.shape for im in images], dst, [g[0] for g in geo], [g[1] for g in geo], [g[2] for g in geo])
    if kind == RR.OUT_U8:
        out = torch.full((total,), CANARY_U8, dtype=torch.uint8, device=dev)
    else:
        out = torch.full((total,), CANARY_F32, dtype=torch.float32, device=dev)
    got = ops.resample_u8(src.to(dev), desc, mode, kind, out=out, fill=fill)
    assert got.data_ptr() == out.data_ptr()
    flat = out.cpu().numpy()
    mask = np.zeros(total, bool)
    per = []
    for k in range(n):
        dh, _, cw = geo[k]
        per.append(flat[dst[k]:dst[k] + dh * cw].reshape(dh, cw).copy())
        mask[dst[k]:dst[k] + dh * cw] = True
    return per, flat, mask


def check_f32(got, ref_grey, taps, what):
    tol = RR.f32_tolerance(taps)
    err = float(np.abs(got.astype(np.float64) - RR.normalise(ref_grey)).max())
    margins.record(what, err, tol)
    print("%s: max |got - ref| = %.3e, bound %.3e" % (what, err, tol))
    assert err <= tol, "%s: %.3e > %.3e" % (what, err, tol)


def check_case(dev, img, dh, dw, mode, what, kinds=(RR.OUT_U8, RR.OUT_F32)):
    ref = RR.resample_ref(img, dh, dw, mode)
    taps = RR.taps_per_output(mode, img.shape[0], img.shape[1], dh, dw)
    for kind in kinds:
        got = launch(dev, [img], [(dh, dw, dw)], mode, kind)[0][0]
        if kind == RR.OUT_U8:
            RR.check_u8(got, ref, what, RR.exact_pixels(img.shape[0], img.shape[1], dh, dw, dw, mode))
        else:
            check_f32(got, ref, taps, what)
    return ref


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_identity_is_exact(dev, mode):
    img = _rand(1, 32, 48)
    u8 = launch(dev, [img], [(32, 48, 48)], mode, RR.OUT_U8)[0][0]
    assert (u8 == img).all()
    want = ((img.astype(np.float32) - np.float32(127.5)) / np.float32(127.5))
    assert (want.astype(np.float64) == np.float64(np.float32(RR.normalise(img)))).all()       # fp32 expression = rounded fp64 value
    for kind in (RR.OUT_F32, RR.OUT_F32_QUANT):
        f = launch(dev, [img], [(32, 48, 48)], mode, kind)[0][0]
        assert f.dtype == np.float32 and (f == want).all()


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1)], ids=["1x1", "1x37", "37x1"])
def test_degenerate_sources(dev, mode, shape):
    img = _rand(2, *shape)
    check_case(dev, img, 32, 48, mode, "degenerate %dx%d mode %d" % (shape + (mode,)))


SHAPES = [(RR.LINEAR, 37, 91, 32, 48), (RR.LINEAR, 61, 203, 32, 16), (RR.LINEAR, 19, 23, 32, 160), (RR.LINEAR, 97, 389, 32, 368),
          (RR.AREA, 67, 211, 32, 100), (RR.AREA, 113, 397, 32, 112), (RR.AREA, 33, 161, 32, 156),
          (RR.CUBIC, 67, 211, 32, 100), (RR.CUBIC, 23, 41, 32, 57), (RR.CUBIC, 150, 300, 32, 64),
          # AREA's enlarging branch: both axes grow; one shrinks and one grows (both take the two-tap form)
          (RR.AREA, 19, 23, 32, 160), (RR.AREA, 64, 23, 32, 160)]


@pytest.mark.parametrize("case", SHAPES, ids=["%s-%dx%d-%dx%d" % ((MODE_IDS[MODES.index(c[0])],) + c[1:]) for c in SHAPES])
def test_shrink_and_enlarge_random(dev, case):
    mode, sh, sw, dh, dw = case
    check_case(dev, _rand(3 + sh + sw, sh, sw), dh, dw, mode, "random %s" % (case,))


@pytest.mark.parametrize("shape", [(64, 96, 32, 48), (96, 48, 32, 16)], ids=["2x2", "3x3"])
def test_area_exact_ties_round_half_to_even(dev, shape):
    sh, sw, dh, dw = shape
    img = _rand(4, sh, sw, 0, 4)
    ref = RR.resample_ref(img, dh, dw, RR.AREA)
    got = launch(dev, [img], [(dh, dw, dw)], RR.AREA, RR.OUT_U8)[0][0]
    if sh == 2 * dh:                                         # a 2 x 2 mean of {0..3} is a multiple of 1/4: exact ties exist
        assert (np.abs(ref - np.floor(ref) - 0.5) < 1e-12).any()
        want = np.rint(np.round(ref * 4.0) / 4.0)
    else:                                                    # a 3 x 3 mean is a multiple of 1/9: (fp64 ref is within 1e-13 of it)
        want = np.rint(np.round(ref * 9.0) / 9.0)
    assert (got == want.astype(np.uint8)).all()


def test_cubic_overshoot_saturates_u8_and_keeps_f32(dev):
    img = (((np.arange(23)[:, None] + np.arange(41)[None, :]) & 1) * 255).astype(np.uint8)
    ref = RR.resample_ref(img, 32, 57, RR.CUBIC)
    assert ref.max() > 256.0 and ref.min() < -1.0
    u8 = launch(dev, [img], [(32, 57, 57)], RR.CUBIC, RR.OUT_U8)[0][0]
    RR.check_u8(u8, ref, "cubic checkerboard")
    assert u8.max() == 255 and u8.min() == 0
    f = launch(dev, [img], [(32, 57, 57)], RR.CUBIC, RR.OUT_F32)[0][0]
    check_f32(f, ref, 4, "cubic checkerboard f32")
    assert f.max() > 1.0 and f.min() < -1.0


RAGGED_SRC = [(1, 1), (20, 333), (150, 40), (31, 17), (64, 64)]
RAGGED_GEO = [(32, 16, 16), (32, 48, 48 + 24), (32, 160, 160 - 8), (32, 368, 368), (32, 32, 32)]
RAGGED_ORDER = [3, 0, 4, 2, 1]


def ragged(dev, mode, kind, fill=200):
    images = [_rand(10 + k, h, w) for k, (h, w) in enumerate(RAGGED_SRC)]
    per, flat, mask = launch(dev, images, RAGGED_GEO, mode, kind, fill=fill, pad_byte=0xAA, gap=32, order=RAGGED_ORDER, out_gap=20)
    return images, per, flat, mask


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_ragged_batch_one_launch(dev, mode):
    for kind in (RR.OUT_U8, RR.OUT_F32):
        images, per, flat, mask = ragged(dev, mode, kind)
        for k, (img, (dh, dw, cw)) in enumerate(zip(images, RAGGED_GEO)):
            ref = RR.canvas_ref(img, dh, dw, cw, mode, fill=200)
            what = "ragged image %d mode %d" % (k, mode)
            if kind == RR.OUT_U8:
                RR.check_u8(per[k], ref, what, RR.exact_pixels(img.shape[0], img.shape[1], dh, dw, cw, mode))
                if cw > dw:
                    assert (per[k][:, dw:] == 200).all()
            else:
                check_f32(per[k], ref, RR.taps_per_output(mode, img.shape[0], img.shape[1], dh, dw), what)
                if cw > dw:
                    assert (per[k][:, dw:] == np.float32((np.float32(200) - np.float32(127.5)) / np.float32(127.5))).all()
        canary = CANARY_U8 if kind == RR.OUT_U8 else np.float32(CANARY_F32)
        assert (~mask).sum() > 100 and (flat[~mask] == canary).all()     # gaps between the regions and the tail are untouched


def test_ragged_batch_is_bitwise_reproducible(dev):
    for kind in (RR.OUT_U8, RR.OUT_F32):
        a = ragged(dev, RR.CUBIC, kind)[2]
        b = ragged(dev, RR.CUBIC, kind)[2]
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("mode", [RR.AREA, RR.LINEAR], ids=["area", "linear"])
@pytest.mark.parametrize("shape", [(1500, 40, 32, 8), (40, 5000, 32, 64)], ids=["tall", "wide"])
def test_streamed_sources(dev, mode, shape):
    sh, sw, dh, dw = shape
    check_case(dev, _rand(5, sh, sw), dh, dw, mode, "streamed %s mode %d" % (shape, mode))


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_quantised_f32_equals_u8_then_normalize(dev, mode):
    from scrabble_gan_amd import ops
    img = _rand(6, 67, 211)
    u8 = launch(dev, [img], [(32, 96, 96)], mode, RR.OUT_U8)[0][0]
    q = launch(dev, [img], [(32, 96, 96)], mode, RR.OUT_F32_QUANT)[0][0]
    want = ops.normalize_u8(torch.from_numpy(u8).to(dev)).cpu().numpy()
    assert q.tobytes() == want.tobytes()


def test_status_codes_and_wrapper_checks(dev, monkeypatch):
    from scrabble_gan_amd import _lib, ops
    fn = _lib.lib().sg_resample_u8
    src = torch.zeros(256, dtype=torch.uint8, device=dev)
    desc = torch.tensor([[0, 4, 4, 16, 0, 4, 4, 4]], dtype=torch.int64, device=dev)
    out = torch.zeros(64, dtype=torch.uint8, device=dev)
    s, d, o = src.data_ptr(), desc.data_ptr(), out.data_ptr()
    assert fn(s, d, 1, 0, 0, o, 255, None) == 0
    torch.cuda.synchronize()
    assert fn(None, d, 1, 0, 0, o, 255, None) == -1
    assert fn(s, None, 1, 0, 0, o, 255, None) == -1
    assert fn(s, d, 1, 0, 0, None, 255, None) == -1
    assert fn(s, d, -1, 0, 0, o, 255, None) == -1
    assert fn(s, d, 1, 3, 0, o, 255, None) == -1 and fn(s, d, 1, -1, 0, o, 255, None) == -1
    assert fn(s, d, 1, 0, 3, o, 255, None) == -1 and fn(s, d, 1, 0, -1, o, 255, None) == -1
    assert fn(s, d, 1, 0, 0, o, 256, None) == -1 and fn(s, d, 1, 0, 0, o, -1, None) == -1
    assert fn(None, None, 0, 0, 0, None, 255, None) == 0

    def no_call(*a, **k):
        raise AssertionError("the entry point was reached")
    monkeypatch.setattr(ops, "call", no_call)
    good = np.array([[0, 4, 4, 16, 0, 4, 4, 4], [64, 4, 4, 16, 16, 4, 4, 4]], np.int64)
    for col, val in ((0, 8), (3, 3), (4, 8)):               # misaligned offset; stride < sw; overlapping output regions
        bad = good.copy()
        bad[1, col] = val
        with pytest.raises(ValueError):
            ops.resample_u8(src, bad, 0, 0)
    with pytest.raises(AssertionError, match="entry point was reached"):
        ops.resample_u8(src, good, 0, 0)
