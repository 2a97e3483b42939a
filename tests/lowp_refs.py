"""Host references of the bf16 / fp8 operand producers (include/scrabble_hip.h: sg_cvt_bf16, sg_cvt_bf16_bias, sg_pack_filter_bf16,
sg_amax_f32, sg_amax2_f32, sg_cvt_fp8, sg_cvt_fp8_bf16, sg_cvt_fp8_grad, sg_pack_filter_fp8, sg_avgpool2_bwd_bf16 / _fp8) -- test
infrastructure, numpy only.

The three conversions (fp32 -> bf16, OCP e4m3fn, OCP e5m2; round to nearest even, subnormals kept) are integer arithmetic on the fp32
bit pattern: no torch or ml_dtypes cast is called anywhere in this file, because those casts are what tests/test_lowp_refs_cpu.py
checks AGAINST these.  The per-entry-point references repeat the header's arithmetic in np.float32, one IEEE operation per step in the
order the header states (numpy neither fuses nor reassociates), with gradual underflow (the kernels are built with fp32 denormals on).
"""
import numpy as np

F32 = np.float32
E4M3 = dict(name="e4m3", ebits=4, mbits=3, bias=7, top=448.0, topcode=0x7e)
E5M2 = dict(name="e5m2", ebits=5, mbits=2, bias=15, top=57344.0, topcode=0x7b)


def _bits(x):
    return np.ascontiguousarray(x, dtype=F32).view(np.uint32)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=np.uint32).view(F32)


# ================================================================================================================================
# conversions
# ================================================================================================================================
def f32_to_bf16_bits(x):
    """Round to nearest even onto the upper 16 bits; a value past the largest finite bf16 becomes +-inf, as RNE prescribes."""
    b = _bits(x).astype(np.uint64)
    nan = ((b & 0x7f800000) == 0x7f800000) & ((b & 0x007fffff) != 0)
    r = (b + 0x7fff + ((b >> 16) & 1)) >> 16
    return np.where(nan, (b >> 16) | 0x40, r).astype(np.uint16)


def _f32_to_fp8_bits(x, fmt):
    """OCP fp8 (fmt = E4M3 / E5M2) of finite |x| <= fmt['top']: RNE, subnormals, carry into the exponent."""
    mbits, bias = fmt["mbits"], fmt["bias"]
    b = _bits(x).astype(np.int64)
    sign, e, m = (b >> 31) & 1, (b >> 23) & 0xff, b & 0x7fffff
    assert bool((e != 0xff).all()), "finite inputs only"
    sig = np.where(e > 0, m | 0x800000, m)                 # |x| = sig * 2^(ee - 150)
    ee = np.where(e > 0, e, 1)
    te = ee - 127 + bias                                   # biased target exponent; < 1: the subnormal quantum applies
    shift = np.minimum((23 - mbits) + np.where(te >= 1, 0, 1 - te), 40)       # (sig < 2^24: any shift >= 26 rounds to 0)
    q, rem, half = sig >> shift, sig & ((np.int64(1) << shift) - 1), np.int64(1) << (shift - 1)
    q = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
    code = np.where(te >= 1, ((te - 1) << mbits) + q, q)   # q carries the implicit bit; a carry out of q moves up one exponent
    assert bool((code <= fmt["topcode"]).all()), "|x| beyond the format's largest finite value"
    return ((sign << 7) | code).astype(np.uint8)


def f32_to_e4m3fn_bits(x):
    return _f32_to_fp8_bits(x, E4M3)


def f32_to_e5m2_bits(x):
    return _f32_to_fp8_bits(x, E5M2)


def bf16_bits_to_f32(h):
    return (np.ascontiguousarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def bf16_bits_to_f64(h):
    with np.errstate(invalid="ignore"):          # (widening a signalling NaN pattern)
        return bf16_bits_to_f32(h).astype(np.float64)


def _fp8_bits_to_f64(c, fmt):
    mbits, bias = fmt["mbits"], fmt["bias"]
    c = np.asarray(c).astype(np.int64)
    e, m = (c >> mbits) & ((1 << fmt["ebits"]) - 1), c & ((1 << mbits) - 1)
    mag = np.where(e > 0, np.ldexp((m + (1 << mbits)).astype(np.float64), e - bias - mbits), np.ldexp(m.astype(np.float64), 1 - bias - mbits))
    if fmt is E4M3:
        mag = np.where((c & 0x7f) == 0x7f, np.nan, mag)
    else:
        mag = np.where(e == 31, np.where(m == 0, np.inf, np.nan), mag)
    return np.where((c >> 7) & 1 == 1, -mag, mag)


def e4m3fn_bits_to_f64(c):
    return _fp8_bits_to_f64(c, E4M3)


def e5m2_bits_to_f64(c):
    return _fp8_bits_to_f64(c, E5M2)


ENC = {"e4m3": f32_to_e4m3fn_bits, "e5m2": f32_to_e5m2_bits, "bf16": f32_to_bf16_bits}
DEC = {"e4m3": e4m3fn_bits_to_f64, "e5m2": e5m2_bits_to_f64, "bf16": bf16_bits_to_f64}
FMT = {"e4m3": E4M3, "e5m2": E5M2}


# ================================================================================================================================
# tie sets (shared by the CPU test of these references and by the GPU test of the kernels)
# ================================================================================================================================
def fp8_ties(name):
    """For every pair of adjacent finite non-negative values of the format (0 and the smallest subnormal included): the midpoint
    (exact in fp32) and its two fp32 neighbours; then the value just below the clamp end and the clamp end itself; both signs.
    -> (values fp32, expected code uint8).  The expectation is written down from the definition of RNE, not computed by the encoder:
    the midpoint goes to the even code, each neighbour to its nearer side."""
    fmt = FMT[name]
    codes = np.arange(0, fmt["topcode"] + 1)
    v = _fp8_bits_to_f64(codes, fmt)
    lo, hi = codes[:-1], codes[1:]
    mid = ((v[:-1] + v[1:]) / 2).astype(F32)
    assert bool((mid.astype(np.float64) * 2 == v[:-1] + v[1:]).all())
    below, above = np.nextafter(mid, F32(0)), np.nextafter(mid, F32(np.inf))
    even = np.where(lo % 2 == 0, lo, hi)
    top = F32(fmt["top"])
    vals = np.concatenate([mid, below, above, [np.nextafter(top, F32(0)), top]]).astype(F32)
    want = np.concatenate([even, lo, hi, [fmt["topcode"], fmt["topcode"]]])
    return np.concatenate([vals, -vals]), np.concatenate([want, want | 0x80]).astype(np.uint8)


def bf16_ties():
    """fp32 patterns with low half 0x7fff / 0x8000 / 0x8001 over every finite upper half (even and odd, subnormals, 0x7f7f whose tie
    goes to inf), both signs.  -> (values fp32, expected bf16 bits uint16)."""
    h = np.arange(0, 0x7f80, dtype=np.uint32)
    pats = np.concatenate([(h << 16) | 0x7fff, (h << 16) | 0x8000, (h << 16) | 0x8001])
    want = np.concatenate([h, np.where(h % 2 == 0, h, h + 1), h + 1])
    pats = np.concatenate([pats, pats | 0x80000000])
    want = np.concatenate([want, want | 0x8000])
    return from_bits(pats), want.astype(np.uint16)


def log_uniform(rng, n, lo_exp, hi_exp):
    """n fp32 values sign * 2^u, u uniform in [lo_exp, hi_exp) with a random mantissa (log-uniform magnitudes)."""
    u = rng.uniform(lo_exp, hi_exp, n)
    return (np.exp2(u) * rng.choice([-1.0, 1.0], n)).astype(F32)


# ================================================================================================================================
# one reference per entry point
# ================================================================================================================================
def scale_of(amax, top):
    """s = fl(top / amax) if amax > 0 else 1 (fp32, correctly rounded division)."""
    a = F32(amax)
    with np.errstate(over="ignore"):
        return F32(top) / a if a > 0 else F32(1.0)


def _rows(rowscale, rowlen, n):
    return np.repeat(np.asarray(rowscale, dtype=F32), int(rowlen))[:n]


def _mul(a, b):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return (np.asarray(a, dtype=F32) * np.asarray(b, dtype=F32)).astype(F32)


def _relu(v):
    return np.where(v > 0, v, F32(0.0)).astype(F32)


def _quant(p, fmt):
    return _f32_to_fp8_bits(np.clip(p, F32(-fmt["top"]), F32(fmt["top"])), fmt)


def cvt_bf16(x, relu=False, rowscale=None, rowlen=8):
    """sg_cvt_bf16: bf16(relu?(fl(rowscale[i / rowlen] * x_i)))  -- row factor, then ReLU, then the rounding."""
    v = np.asarray(x, dtype=F32).ravel()
    if rowscale is not None:
        v = _mul(v, _rows(rowscale, rowlen, v.size))
    if relu:
        v = _relu(v)
    return f32_to_bf16_bits(v)


def colsums(p):
    """fp64 column sums of the fp32 products p [M, C] and the fp64 sums of their magnitudes (the error bound's scale)."""
    p64 = np.asarray(p, dtype=F32).astype(np.float64)
    return p64.sum(axis=0), np.abs(p64).sum(axis=0)


def cvt_bf16_bias(x, rowscale=None, rows_per_sample=1):
    """sg_cvt_bf16_bias on x [M, C] -> (out bits, out_plain bits, fp64 column sums of p, fp64 column sums of |p|), p = fl(rowscale * x)."""
    x = np.asarray(x, dtype=F32)
    M, C = x.shape
    p = x if rowscale is None else _mul(x, _rows(rowscale, rows_per_sample, M)[:, None])
    s, a = colsums(p)
    return f32_to_bf16_bits(p).reshape(M, C), f32_to_bf16_bits(x).reshape(M, C), s, a


def amax(x):
    v = np.asarray(x, dtype=F32)
    return F32(np.abs(v).max()) if v.size else F32(0.0)


def amax2(x, rowscale=None, rowlen=4):
    """sg_amax2_f32 -> (max |x|, max fl(|x| * |rowscale[i / rowlen]|)); both equal without a rowscale."""
    v = np.abs(np.asarray(x, dtype=F32).ravel())
    if v.size == 0:
        return F32(0.0), F32(0.0)
    if rowscale is None:
        return F32(v.max()), F32(v.max())
    return F32(v.max()), F32(_mul(v, np.abs(_rows(rowscale, rowlen, v.size))).max())


def cvt_fp8(x, amax_, relu=False):
    """sg_cvt_fp8: e4m3(clamp(fl(relu?(x) * s), +-448)), s = fl(448 / amax) or 1."""
    v = np.asarray(x, dtype=F32).ravel()
    if relu:
        v = _relu(v)
    return _quant(_mul(v, scale_of(amax_, 448.0)), E4M3)


def cvt_fp8_bf16(x16_bits, amax_, relu=False):
    """sg_cvt_fp8_bf16: the same from a bf16 tensor (widening to fp32 is exact)."""
    return cvt_fp8(bf16_bits_to_f32(np.asarray(x16_bits).ravel()), amax_, relu)


def cvt_fp8_grad(x, amax2_, rowscale=None, rows_per_sample=1):
    """sg_cvt_fp8_grad on x [M, C] -> (e5m2 bits of fl(fl(rowscale x) * s5), e4m3 bits of fl(x * s4), fp64 column sums of the products,
    fp64 column sums of their magnitudes); s4 = fl(448 / amax2[0]), s5 = fl(57344 / amax2[1]), each 1 when its amax is 0."""
    x = np.asarray(x, dtype=F32)
    M, C = x.shape
    p = x if rowscale is None else _mul(x, _rows(rowscale, rows_per_sample, M)[:, None])
    out5 = _quant(_mul(p, scale_of(amax2_[1], 57344.0)), E5M2).reshape(M, C)
    out4 = _quant(_mul(x, scale_of(amax2_[0], 448.0)), E4M3).reshape(M, C)
    s, a = colsums(p)
    return out5, out4, s, a


def _packed(w, taps, K, N, transpose):
    """fp32 [taps][K][N] (transpose = 1) or [taps][N][K] (transpose = 0) -> fp32 [taps][N][K]."""
    w = np.asarray(w, dtype=F32)
    return np.ascontiguousarray(w.reshape(taps, K, N).transpose(0, 2, 1)) if transpose else w.reshape(taps, N, K)


def pack_filter_bf16(w, taps, K, N, transpose):
    return f32_to_bf16_bits(_packed(w, taps, K, N, transpose)).reshape(taps, N, K)


def pack_filter_fp8(w, amax_, taps, K, N, transpose):
    return _quant(_mul(_packed(w, taps, K, N, transpose), scale_of(amax_, 448.0)), E4M3).reshape(taps, N, K)


def _pool_bwd(dout):
    """fl(0.25 * dout[b, y / 2, x / 2, c]) replicated 2 x 2: dout [B, Ho, Wo, C] -> [B, 2 Ho, 2 Wo, C] (exact unless it underflows)."""
    d = _mul(np.asarray(dout, dtype=F32), F32(0.25))
    return np.repeat(np.repeat(d, 2, axis=1), 2, axis=2)


def avgpool2_bwd_bf16(dout, rowscale=None):
    """-> (dx16 bits, dx16_scaled bits): bf16(v) and bf16(fl(rowscale[b] * v)), v = fl(0.25 * dout) replicated."""
    v = _pool_bwd(dout)
    p = v if rowscale is None else _mul(v, np.asarray(rowscale, dtype=F32)[:, None, None, None])
    return f32_to_bf16_bits(v).reshape(v.shape), f32_to_bf16_bits(p).reshape(v.shape)


def avgpool2_bwd_fp8(dout, amax_dout, rowscale=None):
    """-> (e4m3 bits, e5m2 bits, amax_dx pair): amax_dx = fl(0.25 * amax_dout), e4m3(fl(v * s4)), e5m2(fl(fl(rowscale[b] * v) * s5))."""
    v = _pool_bwd(dout)
    a0, a1 = _mul(F32(0.25), F32(amax_dout[0])), _mul(F32(0.25), F32(amax_dout[1]))
    p = v if rowscale is None else _mul(v, np.asarray(rowscale, dtype=F32)[:, None, None, None])
    out4 = _quant(_mul(v, scale_of(a0, 448.0)), E4M3).reshape(v.shape)
    out5 = _quant(_mul(p, scale_of(a1, 57344.0)), E5M2).reshape(v.shape)
    return out4, out5, (F32(a0), F32(a1))
