"""tests/lowp_refs.py checked without a device: the integer-arithmetic bf16 / e4m3fn / e5m2 conversions against the formats' own
definitions (exhaustive decode, re-encode, order, every round-to-nearest-even tie) and bitwise against torch's CPU casts; the
per-entry-point references against plain fp64 formulas at inputs where fp32 arithmetic is exact (power-of-two scales)."""
import numpy as np
import pytest
import torch

from tests import lowp_refs as L

F32 = np.float32
TORCH = {"bf16": (torch.bfloat16, torch.int16, np.uint16), "e4m3": (torch.float8_e4m3fn, torch.uint8, np.uint8),
         "e5m2": (torch.float8_e5m2, torch.uint8, np.uint8)}


def torch_bits(name, x):
    dt, view, npdt = TORCH[name]
    return torch.from_numpy(np.ascontiguousarray(x, dtype=F32)).to(dt).view(view).numpy().view(npdt)


def same_but_zero_sign(got, want, signbit):
    """Bitwise equal, except that a zero result may carry either sign (as tests/test_fp8_gpu.py compares)."""
    got, want = got.astype(np.int64), want.astype(np.int64)
    mag = signbit - 1
    return bool(((got & mag) == (want & mag)).all()) and bool((got == want)[(want & mag) != 0].all())


def test_fp32_subnormals_are_not_flushed_on_this_host():
    """The references rely on numpy's gradual underflow (a library built with fast-math can switch it off process-wide)."""
    tiny = np.array([2.0 ** -126], dtype=F32)
    assert (tiny * F32(0.5))[0] == F32(2.0 ** -127) and (tiny * F32(0.5))[0] != 0


@pytest.mark.parametrize("name", ["e4m3", "e5m2"])
def test_fp8_decode_reencode_order(name):
    fmt = L.FMT[name]
    codes = np.arange(256)
    v = L.DEC[name](codes)
    finite = np.isfinite(v)
    assert finite.sum() == 2 * (fmt["topcode"] + 1)
    assert v[fmt["topcode"]] == fmt["top"] and v[1] == 2.0 ** (1 - fmt["bias"] - fmt["mbits"]) and v[0] == 0 and v[0x80] == 0
    assert not np.isfinite(v[fmt["topcode"] + 1:128]).any() and not np.isfinite(v[128 + fmt["topcode"] + 1:]).any()
    if name == "e4m3":
        assert np.isnan(v[0x7f]) and np.isnan(v[0xff])
    else:
        assert v[0x7c] == np.inf and v[0xfc] == -np.inf and np.isnan(v[0x7d:0x80]).all()
    fc = codes[finite]
    assert np.array_equal(L.ENC[name](v[finite].astype(F32)), fc.astype(np.uint8))
    pos = v[:fmt["topcode"] + 1]
    assert (np.diff(pos) > 0).all() and np.array_equal(v[128:128 + fmt["topcode"] + 1], -pos)
    # against the definition: (-1)^s 2^(e - bias) (1 + m / 2^mbits), subnormals 2^(1 - bias) m / 2^mbits
    for c in (0x01, 0x07, 0x08, 0x35, fmt["topcode"]):
        e, m = c >> fmt["mbits"], c & ((1 << fmt["mbits"]) - 1)
        want = 2.0 ** (e - fmt["bias"]) * (1 + m / 2 ** fmt["mbits"]) if e else 2.0 ** (1 - fmt["bias"]) * m / 2 ** fmt["mbits"]
        assert v[c] == want


def test_bf16_decode_reencode_order():
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    v = L.bf16_bits_to_f64(h)
    finite = np.isfinite(v)
    assert finite.sum() == 2 * 0x7f80
    assert np.array_equal(L.f32_to_bf16_bits(v[finite].astype(F32)), h[finite])
    assert (np.diff(v[:0x7f80]) > 0).all() and np.array_equal(v[0x8000:0x8000 + 0x7f80], -v[:0x7f80])
    assert v[0x3f80] == 1.0 and v[0x0001] == 2.0 ** -133 and v[0x7f7f] == (2 - 2.0 ** -7) * 2.0 ** 127 and v[0x7f80] == np.inf
    assert L.f32_to_bf16_bits(np.array([np.inf, -np.inf], dtype=F32)).tolist() == [0x7f80, 0xff80]
    assert L.f32_to_bf16_bits(np.array([np.finfo(F32).max], dtype=F32))[0] == 0x7f80          # RNE: the largest fp32 rounds to inf


@pytest.mark.parametrize("name", ["e4m3", "e5m2", "bf16"])
def test_every_tie_goes_to_even_and_its_neighbours_to_their_side(name):
    vals, want = L.bf16_ties() if name == "bf16" else L.fp8_ties(name)
    got = L.ENC[name](vals)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (name, vals[bad[:4]], got[bad[:4]], want[bad[:4]])
    if name != "bf16":          # the midpoint between 0 and the smallest subnormal, and the clamp end, are in the set
        fmt = L.FMT[name]
        half_min = F32(2.0 ** (-fmt["bias"] - fmt["mbits"]))
        i = np.nonzero(vals == half_min)[0]
        assert i.size == 1 and got[i[0]] == 0 and L.ENC[name](np.nextafter(half_min, F32(1)).reshape(1))[0] == 1
        assert (vals == F32(fmt["top"])).sum() == 1 and (vals == np.nextafter(F32(fmt["top"]), F32(0))).sum() == 1


@pytest.mark.parametrize("name", ["e4m3", "e5m2", "bf16"])
def test_bitwise_agreement_with_torch_cpu(name):
    """The tie sets plus 2^20 random fp32 values spread log-uniformly over the format's range (fp8: down to a quarter of the smallest
    subnormal's midpoint, up to the largest finite value; bf16: the whole fp32 range, subnormals included)."""
    rng = np.random.default_rng(20)
    vals, _ = L.bf16_ties() if name == "bf16" else L.fp8_ties(name)
    if name == "bf16":
        rand = L.log_uniform(rng, 1 << 20, -151.0, 128.0)
        rand = rand[np.isfinite(rand)]
        signbit = 0x8000
    else:
        fmt = L.FMT[name]
        rand = L.log_uniform(rng, 1 << 20, 1 - fmt["bias"] - fmt["mbits"] - 3.0, np.log2(fmt["top"]))
        rand = np.clip(rand, -F32(fmt["top"]), F32(fmt["top"]))
        signbit = 0x80
    x = np.concatenate([vals, rand, np.array([0.0, -0.0], dtype=F32)])
    assert same_but_zero_sign(L.ENC[name](x), torch_bits(name, x), signbit)


# ---- composite references at exactly representable inputs ---------------------------------------------------------------------
def _exact_grid(rng, n, lo, hi, bits=6):
    """Values k * 2^e with |k| < 2^bits: products with powers of two and with each other's few bits stay exact in fp32."""
    return (rng.integers(-(1 << bits) + 1, 1 << bits, n) * np.exp2(rng.integers(lo, hi, n))).astype(F32)


def _ideal(v64, name):
    """Round fp64 values (exactly representable in fp32) to the format and decode: the plain formula."""
    return L.DEC[name](L.ENC[name](v64.astype(F32)))


def test_composites_match_fp64_formulas_at_power_of_two_scales():
    rng = np.random.default_rng(3)
    M, C, rps = 12, 16, 5
    x = _exact_grid(rng, M * C, -12, 3).reshape(M, C)
    # amax = a power-of-two multiple of 448 / 57344: the scales are 8 and 512, every product is exact
    a4, a5 = F32(448.0 * 2.0 ** -3), F32(57344.0 * 2.0 ** -9)
    x = np.clip(x, -a4, a4)
    x[0, 0], x[-1, -1] = a4, -a4
    rs = np.array([1.0, -0.5, 0.0], dtype=F32)
    x64, f64 = x.astype(np.float64), np.repeat(rs.astype(np.float64), rps)[:M][:, None]
    p64 = x64 * f64
    assert np.abs(p64).max() <= float(a5)
    # sg_cvt_fp8 / sg_cvt_fp8_bf16 / sg_pack_filter_fp8
    got = L.DEC["e4m3"](L.cvt_fp8(x, a4))
    assert np.array_equal(got, _ideal(x64.ravel() * 8.0, "e4m3"))
    got = L.DEC["e4m3"](L.cvt_fp8(x, a4, relu=True))
    assert np.array_equal(got, _ideal(np.maximum(x64.ravel(), 0) * 8.0, "e4m3"))
    x16 = L.f32_to_bf16_bits(x)
    assert np.array_equal(L.DEC["e4m3"](L.cvt_fp8_bf16(x16, a4)), _ideal(L.bf16_bits_to_f64(x16).ravel() * 8.0, "e4m3"))
    assert np.array_equal(L.cvt_fp8(np.zeros(8, F32), 0.0), np.zeros(8, np.uint8))            # amax == 0: scale 1
    assert np.array_equal(L.cvt_fp8(np.array([1.0, -2.0], F32), 0.0), L.ENC["e4m3"](np.array([1.0, -2.0], F32)))
    # sg_cvt_fp8_grad
    o5, o4, s, a = L.cvt_fp8_grad(x, (a4, a5), rs, rps)
    assert np.array_equal(L.DEC["e5m2"](o5), _ideal(p64 * 512.0, "e5m2")) and np.array_equal(L.DEC["e4m3"](o4), _ideal(x64 * 8.0, "e4m3"))
    assert np.array_equal(s, p64.sum(axis=0)) and np.array_equal(a, np.abs(p64).sum(axis=0))
    # sg_cvt_bf16 / sg_cvt_bf16_bias: row factor, then ReLU, then the rounding
    got = L.bf16_bits_to_f64(L.cvt_bf16(x, relu=True, rowscale=rs, rowlen=rps * C))
    assert np.array_equal(got, _ideal(np.maximum(p64, 0).ravel(), "bf16"))
    ob, op, s, a = L.cvt_bf16_bias(x, rs, rps)
    assert np.array_equal(L.bf16_bits_to_f64(ob), _ideal(p64, "bf16")) and np.array_equal(L.bf16_bits_to_f64(op), _ideal(x64, "bf16"))
    assert np.array_equal(s, p64.sum(axis=0))
    # sg_amax_f32 / sg_amax2_f32
    assert float(L.amax(x)) == np.abs(x64).max()
    assert [float(t) for t in L.amax2(x, rs, rps * C)] == [np.abs(x64).max(), np.abs(p64).max()]
    assert [float(t) for t in L.amax2(x)] == [np.abs(x64).max()] * 2


@pytest.mark.parametrize("transpose", [0, 1])
def test_pack_layout(transpose):
    """out[t][n][k] = w[t][k][n] (transpose = 1) or w[t][n][k] (transpose = 0), written element by element."""
    taps, K, N = 2, 3, 5
    w = np.arange(taps * K * N, dtype=F32)
    want = np.zeros((taps, N, K))
    for t in range(taps):
        for n in range(N):
            for k in range(K):
                want[t, n, k] = w[(t * K + k) * N + n] if transpose else w[(t * N + n) * K + k]
    assert np.array_equal(L.bf16_bits_to_f64(L.pack_filter_bf16(w, taps, K, N, transpose)), want)
    a = F32(448.0 / 4)          # scale 4: 4 * (0 .. 29) stays on e4m3's grid only partly -> compare through the plain formula
    assert np.array_equal(L.DEC["e4m3"](L.pack_filter_fp8(w, a, taps, K, N, transpose)), _ideal(want.ravel() * 4.0, "e4m3").reshape(want.shape))


def test_pool_references():
    rng = np.random.default_rng(5)
    B, Ho, Wo, C = 2, 1, 3, 8
    d = _exact_grid(rng, B * Ho * Wo * C, -6, 2).reshape(B, Ho, Wo, C)
    rs = np.array([-2.0, 0.25], dtype=F32)
    up = np.zeros((B, 2 * Ho, 2 * Wo, C))
    for y in range(2 * Ho):
        for x in range(2 * Wo):
            up[:, y, x] = 0.25 * d[:, y // 2, x // 2].astype(np.float64)
    sc = up * rs.astype(np.float64)[:, None, None, None]
    p, s = L.avgpool2_bwd_bf16(d, rs)
    assert np.array_equal(L.bf16_bits_to_f64(p), _ideal(up, "bf16")) and np.array_equal(L.bf16_bits_to_f64(s), _ideal(sc, "bf16"))
    a_in = (F32(448.0 * 2.0 ** 1), F32(57344.0 * 2.0 ** -4))          # 0.25 x those: scales 2 and 64
    d = np.clip(d, -a_in[0], a_in[0])
    o4, o5, a_dx = L.avgpool2_bwd_fp8(d, a_in, rs)
    assert [float(t) for t in a_dx] == [0.25 * float(a_in[0]), 0.25 * float(a_in[1])]
    assert np.array_equal(L.DEC["e4m3"](o4), _ideal(up * 2.0, "e4m3"))
    assert np.abs(sc).max() * 64.0 <= 57344.0 and np.array_equal(L.DEC["e5m2"](o5), _ideal(sc * 64.0, "e5m2"))
