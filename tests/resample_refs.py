"""fp64 numpy reference of sg_resample_u8 (test infrastructure; written from the sampling definitions of include/scrabble_hip.h,
not from the kernel).  Per axis a dense weight matrix W [d, s]; an image is resampled as Wy @ img @ Wx.T.  Positions are exact
rationals (fractions.Fraction), so a tap index never depends on a floating-point floor; each weight is then one fp64 number.

LINEAR  x = (i + 0.5) s/d - 0.5; taps floor(x), floor(x)+1 with weights 1-f, f; indices clamped to [0, s-1]
CUBIC   the same x; taps floor(x)-1 .. floor(x)+2; Keys kernel, A = -0.75; indices clamped
AREA    both scales >= 1: output i averages [i s/d, (i+1) s/d) with fractional coverage
        either scale < 1: BOTH axes take sx = floor(i s/d), sx+1 with fx = (i+1) - (sx+1) d/s, fx <= 0 -> 0 else frac(fx);
        sx >= s-1 -> sx = s-1, fx = 0"""
from fractions import Fraction
from math import floor

import numpy as np

LINEAR, AREA, CUBIC = 0, 1, 2
OUT_U8, OUT_F32, OUT_F32_QUANT = 0, 1, 2
A = -0.75


def _keys(x: float) -> float:
    x = abs(x)
    if x <= 1.0:
        return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0
    if x < 2.0:
        return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A
    return 0.0


def axis_weights(mode: int, s: int, d: int, area_two_tap: bool = False) -> np.ndarray:
    """W [d, s] fp64.  area_two_tap: the image takes AREA's enlarging branch (either of its two scales is below 1)."""
    W = np.zeros((d, s), np.float64)
    scale = Fraction(s, d)
    for i in range(d):
        if mode in (LINEAR, CUBIC):
            x = (i + Fraction(1, 2)) * scale - Fraction(1, 2)
            fl = floor(x)
            f = float(x - fl)
            if mode == LINEAR:
                taps = [(fl, 1.0 - f), (fl + 1, f)]
            else:
                taps = [(fl - 1, _keys(1.0 + f)), (fl, _keys(f)), (fl + 1, _keys(1.0 - f)), (fl + 2, _keys(2.0 - f))]
        elif not area_two_tap:
            lo, hi = i * scale, (i + 1) * scale
            taps = []
            t = floor(lo)
            while t < hi:
                cover = min(hi, Fraction(t + 1)) - max(lo, Fraction(t))
                taps.append((t, float(cover / scale)))
                t += 1
        else:
            sx = floor(i * scale)
            fx = (i + 1) - (sx + 1) / scale
            fx = Fraction(0) if fx <= 0 else fx - floor(fx)
            if sx >= s - 1:
                sx, fx = s - 1, Fraction(0)
            taps = [(sx, float(1 - fx)), (sx + 1, float(fx))]
        for t, w in taps:
            W[i, min(max(t, 0), s - 1)] += w
    return W


def taps_per_output(mode: int, sh: int, sw: int, dh: int, dw: int) -> int:
    """Largest number of source pixels feeding one output along either axis (the `taps` of the fp32 tolerance)."""
    if mode == LINEAR:
        return 2
    if mode == CUBIC:
        return 4
    if sh < dh or sw < dw:
        return 2
    def box(s, d):      # source pixels that [i s/d, (i+1) s/d) touches, the most over i
        return max(-(-((i + 1) * s) // d) - (i * s) // d for i in range(d))
    return max(box(sh, dh), box(sw, dw))


def resample_ref(img: np.ndarray, dh: int, dw: int, mode: int) -> np.ndarray:
    """uint8 [sh, sw] -> fp64 [dh, dw] in grey levels, unrounded."""
    sh, sw = img.shape
    two = mode == AREA and (sh < dh or sw < dw)
    Wy = axis_weights(mode, sh, dh, two)
    Wx = axis_weights(mode, sw, dw, two)
    return Wy @ img.astype(np.float64) @ Wx.T


def canvas_ref(img: np.ndarray, dh: int, dw: int, canvas_w: int, mode: int, fill: int = 255) -> np.ndarray:
    """The written [dh, canvas_w] rows in grey levels: the resampled image cropped to canvas_w, or padded with fill."""
    ref = resample_ref(img, dh, dw, mode)
    out = np.full((dh, canvas_w), float(fill), np.float64)
    n = min(dw, canvas_w)
    out[:, :n] = ref[:, :n]
    return out


def normalise(v):
    return (np.asarray(v, np.float64) - 127.5) / 127.5


def f32_tolerance(taps: int) -> float:
    """|got - ref| <= (2 taps + 4) 2^-23 in normalised units: n u on values of magnitude <= 2 (u = 2^-24), two passes, + 4 for the
    weight roundings and the normalisation."""
    return (2 * taps + 4) * 2.0 ** -23


def exact_pixels(sh: int, sw: int, dh: int, dw: int, canvas_w: int, mode: int) -> np.ndarray:
    """[dh, canvas_w] bool: pixels whose row and column weights are all multiples of 2^-6.  There the fp32 evaluation is exact
    (8-bit pixels x 6-bit weights: 14 bits after the first pass, 20 after the second, partial sums below 2^10: within the 24-bit
    significand), the fp64 reference is exact too, so an exact tie is a TRUE tie and round-half-to-even is required, not allowed.
    Fill columns are exact."""
    two = mode == AREA and (sh < dh or sw < dw)
    def dyadic(W):
        return (W * 64.0 == np.round(W * 64.0)).all(axis=1)
    ey, ex = dyadic(axis_weights(mode, sh, dh, two)), dyadic(axis_weights(mode, sw, dw, two))
    cols = np.ones(canvas_w, bool)
    n = min(dw, canvas_w)
    cols[:n] = ex[:n]
    return ey[:, None] & cols[None, :]


def check_u8(got: np.ndarray, ref: np.ndarray, what: str, exact: np.ndarray = None, max_tie_share: float = 0.02):
    """Equality with round_half_even(clip(ref)) wherever ref is farther than 2e-3 from a half-integer AND on every pixel of `exact`
    (exact_pixels: fp32 and fp64 are both exact there, ties included); +-1 on the remaining near-tie pixels, which may be at most
    max_tie_share of the case (counted from the reference alone)."""
    clipped = np.clip(ref, 0.0, 255.0)
    want = np.rint(clipped)                                   # numpy rounds half to even
    near = np.abs(clipped - np.floor(clipped) - 0.5) <= 2e-3
    if exact is not None:
        near &= ~exact
    assert near.mean() <= max_tie_share, "%s: %.2f %% of the pixels are near ties" % (what, 100.0 * near.mean())
    diff = got.astype(np.int64) - want.astype(np.int64)
    assert (diff[~near] == 0).all(), "%s: %d pixels differ away from ties (max |diff| %d)" % (what, int((diff[~near] != 0).sum()), int(np.abs(diff).max()))
    assert (np.abs(diff[near]) <= 1).all(), "%s: a near-tie pixel differs by more than 1" % what
    return float(near.mean())
