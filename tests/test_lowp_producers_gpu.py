"""Bit-exact edge tests of the bf16 / fp8 operand producers against tests/lowp_refs.py (an integer-arithmetic host reference that
tests/test_lowp_refs_cpu.py checks without a device): sg_cvt_bf16, sg_cvt_bf16_bias, sg_pack_filter_bf16, sg_amax_f32, sg_amax2_f32,
sg_cvt_fp8, sg_cvt_fp8_bf16, sg_cvt_fp8_grad, sg_pack_filter_fp8, sg_avgpool2_bwd_bf16, sg_avgpool2_bwd_fp8.

The kernels are called through the C entry points (ops.call), every output lies between two guard blocks, and output bytes are compared
bitwise.  The only tolerance is the sign bit of a ZERO result, case by case:
  * ReLU runs, at elements whose value before the ReLU is <= 0 (max(-0.0, 0) and max(x, 0) may be either zero);
  * fp8 outputs, at non-zero products that round to a zero code (a flushed product);
everything else -- a -0.0 input, 0 * negative factor, every bf16 result without ReLU -- is compared with its sign.

Data (one builder per target format, shared by every sweep kernel): every round-to-nearest-even midpoint of the format with both fp32
neighbours, scaled by the power of two that makes the kernel's scale exact (amax = 448 * 2^k = 57344 * 2^(k - 7), k in {0, -3, 5});
non-power-of-two amax (3.7, 1e-3) with log-uniform magnitudes from below the format's smallest subnormal up to amax, where the
reference's double rounding must be reproduced; +-0, the largest finite fp32 (bf16: RNE gives inf), the amax element first and last,
an all-zero tensor.

Column sums: |dbias - (start + fp64 sum)| <= M * 2^-24 * sum_m |fl(rowscale * x[m, c])| per column, the worst case of any fp32
summation order.  The non-zero start is fl(-sum / 4): non-zero wherever the sum is, and of the opposite sign, so that the one addition
that involves it rounds a number no larger than the sum itself and stays inside that bound.  One column cancels exactly under terms of
40 (a bar relative to max |ref| would mean nothing there); its start is 2^-6, counted as one more summand (start_and_scale).  The
share of the bound used goes to tests/margins.py.

Every designed tie reaches every fp8-writing kernel at every k: the "all-ties" sizes of the flat sweeps, test_cvt_fp8_grad_all_ties,
the last pool shape and the larger filters hold a whole pool, and assert that on the data.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lowp_refs as L  # noqa: E402
from tests import margins  # noqa: E402

F32 = np.float32
GUARD, FILL, ERR_ARG = 4096, 0xA5, -1
FMAX = np.finfo(F32).max
FACTORS = np.array([-0.5, 0.0, 1.0, 3e-39, 0.75, -1.0], dtype=F32)      # a negative, a zero, 1, one that underflows the product
SIZES = [8, 16, 8 * 255, 8 * 256, 8 * 257]
BIG = 8 * (4096 * 256 + 3)                                             # past the 4096-workgroup cap: the grid-stride loop runs twice
AMAXES = [448.0, 448.0 / 8, 448.0 * 32, 3.7, 1e-3]
POOL8 = 5616                                                           # size of pool_fp8 at a power-of-two amax = 117 * 48 = 3 * 2 * 3 * 312


# ================================================================================================================================
# plumbing
# ================================================================================================================================
def _ops():
    from scrabble_gan_amd import ops
    return ops


def _raw(args):
    """An In / Buf passed as an argument stands for its pointer (and stays alive until the launch has finished)."""
    return [a.ptr if isinstance(a, (In, Buf)) else a for a in args]


def run(name, *args):
    ops = _ops()
    ops.call(name, *_raw(args), ops._stream())
    torch.cuda.synchronize()


def rc_of(name, *args):
    ops = _ops()
    rc = getattr(ops.lib(), name)(*_raw(args), ops._stream())
    torch.cuda.synchronize()
    return rc


class Buf:
    """nbytes of output between two guard blocks of FILL; init: a numpy array whose bytes are the payload's start contents."""

    def __init__(self, dev, nbytes, init=None):
        self.n = int(nbytes)
        self.buf = torch.full((2 * GUARD + self.n,), FILL, dtype=torch.uint8, device=dev)
        if init is not None:
            raw = np.ascontiguousarray(init).view(np.uint8).ravel()
            assert raw.size == self.n
            self.buf[GUARD:GUARD + self.n].copy_(torch.from_numpy(raw.copy()))
        self.ptr = self.buf.data_ptr() + GUARD

    def read(self, dtype):
        return self.buf[GUARD:GUARD + self.n].cpu().numpy().view(dtype)

    def check(self, name):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == FILL).all(), "%s: wrote in front of its output" % name
        assert (h[GUARD + self.n:] == FILL).all(), "%s: wrote behind its output" % name

    def untouched(self, name):
        assert (self.buf.cpu().numpy() == FILL).all(), "%s: wrote although it had to refuse / had nothing to do" % name


class In:
    """A host array on the device (kept alive); .ptr is never null, also for an empty array."""

    def __init__(self, dev, a):
        a = np.ascontiguousarray(a)
        raw = a.view(np.uint8).ravel()
        self.t = torch.from_numpy(np.concatenate([raw, np.zeros(16, np.uint8)])).to(dev)
        self.ptr = self.t.data_ptr()


def same_bits(got, want, name, zero_free=None, signbit=0x80):
    got, want = np.asarray(got).ravel().astype(np.int64), np.asarray(want).ravel().astype(np.int64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    diff = got != want
    if zero_free is not None:
        mag = signbit - 1
        diff &= ~(np.asarray(zero_free).ravel() & ((got & mag) == 0) & ((want & mag) == 0))
    bad = np.nonzero(diff)[0]
    assert bad.size == 0, "%s: %d of %d elements differ; first at %d: got %#x, want %#x" % (name, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def flushed(p, want):
    """Non-zero fp32 products whose reference code is a zero."""
    return (np.asarray(p).ravel() != 0) & ((np.asarray(want).ravel() & 0x7f) == 0)


def free8(p, want, relu_src=None):
    z = flushed(p, want)
    return z if relu_src is None else z | ~(np.asarray(relu_src).ravel() > 0)


# ================================================================================================================================
# data
# ================================================================================================================================
@functools.lru_cache(maxsize=None)
def pool_bf16():
    rng = np.random.default_rng(16)
    ties = L.bf16_ties()[0]
    special = np.array([0.0, -0.0, FMAX, -FMAX, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126, 1.0], dtype=F32)
    return np.concatenate([special, rng.permutation(np.concatenate([ties, L.log_uniform(rng, 8184, -149.0, 127.9)]))])


@functools.lru_cache(maxsize=None)
def pool_fp8(amax):
    """|values| <= amax.  amax = 448 * 2^k: every e4m3 tie * 2^k and every e5m2 tie * 2^(k - 7) (exact), so that both scales
    448 / amax and 57344 / amax are powers of two and the products are the ties themselves."""
    rng = np.random.default_rng(int(F32(amax).view(np.uint32)))          # (another permutation for every amax)
    parts = list(scaled_ties(amax))
    fill = (POOL8 if parts else 4104) - 4 - sum(p.size for p in parts)          # (sizes that are multiples of 8)
    parts.append(np.clip(L.log_uniform(rng, fill, -36.0, 0.0) * F32(amax), -F32(amax), F32(amax)))
    # the first and the last element are spare zeros: take() puts +amax / -amax there without displacing a tie
    pool = np.concatenate([np.array([0.0, 0.0, -0.0], dtype=F32), rng.permutation(np.concatenate(parts)), np.zeros(1, F32)]).astype(F32)
    assert pool.size % 8 == 0
    return pool


def scaled_ties(amax):
    """[e4m3 ties * 2^k, e5m2 ties * 2^(k - 7)] for amax = 448 * 2^k, [] for any other amax."""
    k = np.log2(amax / 448.0) if amax > 0 else 0.5
    if k != np.round(k):
        return []
    return [np.ldexp(L.fp8_ties(name)[0], kk).astype(F32) for name, kk in (("e4m3", int(k)), ("e5m2", int(k) - 7))]


def assert_holds_ties(x, amax, which=(0, 1)):
    """The tensor holds every designed tie of the format(s) (e4m3: 0, e5m2: 1) with both fp32 neighbours, bit for bit."""
    have = np.asarray(x, dtype=F32).ravel().view(np.uint32)
    for i in which:
        t = scaled_ties(amax)[i].view(np.uint32)
        assert np.isin(t, have).all(), "%d designed ties missing from the data" % int((~np.isin(t, have)).sum())


@functools.lru_cache(maxsize=None)
def pool_grad16():
    """bf16 ties and log-uniform values of moderate size (column sums of them mean something)."""
    rng = np.random.default_rng(17)
    ties = L.bf16_ties()[0]
    ties = ties[(np.abs(ties) >= 2.0 ** -14) & (np.abs(ties) < 8.0)]
    return np.concatenate([np.array([0.0, -0.0], dtype=F32), rng.permutation(np.concatenate([ties[::7], L.log_uniform(rng, 4096, -20.0, 3.0)]))])


def take(pool, n, amax=None, pos=0):
    x = np.resize(pool, n).astype(F32) if n else np.zeros(0, F32)
    if amax is not None and n:
        x[pos] = F32(amax) if pos == 0 else -F32(amax)
    return x


def grad_data(M, C, pool, amax):
    """[M, C]: the pool, +-amax first and last, column 1 cancelling exactly in pairs under terms of 40 (an odd last row adds 0.125)."""
    x = take(pool, M * C).reshape(M, C)
    x[0, 0], x[-1, -1] = F32(amax), -F32(amax)
    m = np.arange(M)
    col = np.where(m % 2 == 0, 1.0, -1.0) * (40.0 + (m // 2) * 2.0 ** -6)
    if M % 2:
        col[-1] = 0.125
    x[:, 1] = col.astype(F32)
    return x


def factors(n):
    return np.resize(FACTORS, n).astype(F32)


# ================================================================================================================================
# flat sweeps
# ================================================================================================================================
@pytest.mark.parametrize("n", [0] + SIZES + ["all-ties"])
def test_cvt_bf16_flat(dev, n):
    """Without ReLU bitwise, signs of zeros included (FMAX -> inf, subnormals kept); all-ties: every bf16 midpoint and its neighbours."""
    n = pool_bf16().size // 8 * 8 if n == "all-ties" else n
    x = take(pool_bf16(), n)
    xi = In(dev, x)
    for relu in (0, 1):
        out = Buf(dev, 2 * n)
        run("sg_cvt_bf16", xi.ptr, out.ptr, n, relu, None, 8)
        name = "sg_cvt_bf16 n=%d relu=%d" % (n, relu)
        out.check(name)
        if n == 0:
            out.untouched(name)
            continue
        same_bits(out.read(np.uint16), L.cvt_bf16(x, relu), name, ~(x > 0) if relu else None, 0x8000)


@pytest.mark.parametrize("rowlen", [8, 24, 8 * 257])
def test_cvt_bf16_row_factors(dev, rowlen):
    """Row factor, THEN ReLU, then the rounding: a negative factor turns the positives of its row into zeros.  Consecutive groups of 8
    on both sides of a row boundary take different factors."""
    rows = 7
    x, f = take(pool_bf16(), rows * rowlen), factors(rows)
    xi, fi = In(dev, x), In(dev, f)
    p = L._mul(x, np.repeat(f, rowlen))
    for relu in (0, 1):
        out = Buf(dev, 2 * x.size)
        run("sg_cvt_bf16", xi.ptr, out.ptr, x.size, relu, fi.ptr, rowlen)
        name = "sg_cvt_bf16 rowlen=%d relu=%d" % (rowlen, relu)
        out.check(name)
        want = L.cvt_bf16(x, relu, f, rowlen)
        same_bits(out.read(np.uint16), want, name, ~(p > 0) if relu else None, 0x8000)
        if relu:
            assert (want[(np.repeat(f, rowlen) < 0) & (x > 0)] == 0).all()


def _amax_slot(dev, x, name):
    """sg_amax_f32 into a zeroed guarded slot: must be exactly max |x|."""
    slot = Buf(dev, 4, np.zeros(1, F32))
    run("sg_amax_f32", In(dev, x), x.size, slot.ptr)
    slot.check(name + " amax")
    assert slot.read(F32)[0] == L.amax(x), (name, slot.read(F32)[0], L.amax(x))
    return slot


@pytest.mark.parametrize("n", [0] + SIZES + ["all-ties"])
def test_cvt_fp8_flat(dev, n):
    n_ = n
    """sg_amax_f32 + sg_cvt_fp8: designed ties (power-of-two scales), non-power-of-two amax, the amax element first / last, all zeros.
    all-ties: the whole pool of each amax, i.e. at 448 * 2^k every e4m3 midpoint with both neighbours, the value just below the clamp
    end and the clamp end (asserted on the data)."""
    for amax in AMAXES + [0.0]:
        n = n_ if n_ != "all-ties" else pool_fp8(amax).size if amax > 0 else 8
        for pos in (0, -1):
            x = take(pool_fp8(amax), n, amax, pos) if amax > 0 else take(np.array([0.0, -0.0, 0.0], F32), n)
            if n_ == "all-ties" and scaled_ties(amax):
                assert_holds_ties(x, amax)
            if n == 0 and (amax != AMAXES[0] or pos):
                continue
            name = "sg_cvt_fp8 n=%d amax=%g pos=%d" % (n, amax, pos)
            xi = In(dev, x)
            slot = _amax_slot(dev, x, name) if n else Buf(dev, 4, np.array([amax], F32))
            a = slot.read(F32)[0]
            assert n == 0 or a == F32(amax)
            for relu in (0, 1):
                out = Buf(dev, n)
                run("sg_cvt_fp8", xi.ptr, out.ptr, n, relu, slot.ptr)
                out.check(name)
                if n == 0:
                    out.untouched(name)
                    continue
                want = L.cvt_fp8(x, a, relu)
                got = out.read(np.uint8)
                same_bits(got, want, "%s relu=%d" % (name, relu), free8(L._mul(x, L.scale_of(a, 448.0)), want, x if relu else None))
                if amax == 0.0:
                    assert ((got & 0x7f) == 0).all(), name + ": amax == 0 means scale 1, every byte a zero"


@pytest.mark.parametrize("n", [0] + SIZES + ["all-ties"])
def test_cvt_fp8_bf16_flat(dev, n):
    """The same conversion from a bf16 tensor: the bf16 roundings of the same data, scale from their own maximum.  all-ties: the whole
    pool of each amax; every e4m3 midpoint is a bf16 value (its fp32 neighbours round onto it), so the midpoints arrive exactly."""
    n_ = n
    for amax in AMAXES + [0.0]:
        n = n_ if n_ != "all-ties" else pool_fp8(amax).size if amax > 0 else 8
        if n == 0 and amax != AMAXES[0]:
            continue
        x16 = L.f32_to_bf16_bits(take(pool_fp8(amax), n, amax, -1) if amax > 0 else take(np.array([0.0, -0.0, 0.0], F32), n))
        xv = L.bf16_bits_to_f32(x16)
        a = L.amax(xv)
        xi, ai = In(dev, x16), In(dev, np.array([a], F32))
        for relu in (0, 1):
            name = "sg_cvt_fp8_bf16 n=%d amax=%g relu=%d" % (n, amax, relu)
            out = Buf(dev, n)
            run("sg_cvt_fp8_bf16", xi.ptr, out.ptr, n, relu, ai.ptr)
            out.check(name)
            if n == 0:
                out.untouched(name)
                continue
            want = L.cvt_fp8_bf16(x16, a, relu)
            same_bits(out.read(np.uint8), want, name, free8(L._mul(xv, L.scale_of(a, 448.0)), want, xv if relu else None))


@pytest.mark.parametrize("n", [0, 4, 8, 4 * 255, 4 * 256, 4 * 257])
def test_amax_slots(dev, n):
    """The maximum at each position of the LAST float4; a preset slot stays when larger and is raised when smaller; launches
    accumulate; sg_amax2_f32 without rowscale fills both slots alike."""
    base = take(pool_fp8(3.7), n)
    if n == 0:
        s1, s2 = Buf(dev, 4, np.array([2.5], F32)), Buf(dev, 8, np.array([2.5, 1.5], F32))
        run("sg_amax_f32", In(dev, base), 0, s1.ptr)
        run("sg_amax2_f32", In(dev, base), 0, None, 4, s2.ptr)
        s1.check("amax n=0"), s2.check("amax2 n=0")
        assert s1.read(F32).tolist() == [2.5] and s2.read(F32).tolist() == [2.5, 1.5]
        return
    for j in range(4):
        x = base.copy()
        x[n - 4 + j] = F32(-7.5 - j)
        xi = In(dev, x)
        for preset, want in ((0.0, 7.5 + j), (100.0, 100.0), (1.0, 7.5 + j)):
            s1, s2 = Buf(dev, 4, np.array([preset], F32)), Buf(dev, 8, np.array([preset, 0.0], F32))
            run("sg_amax_f32", xi.ptr, n, s1.ptr)
            run("sg_amax2_f32", xi.ptr, n, None, 4, s2.ptr)
            s1.check("amax"), s2.check("amax2")
            assert s1.read(F32).tolist() == [want], (n, j, preset, s1.read(F32))
            assert s2.read(F32).tolist() == [want, 7.5 + j], (n, j, preset, s2.read(F32))
    # two launches into one slot: a smaller tensor leaves it, a larger one raises it
    slot = Buf(dev, 4, np.zeros(1, F32))
    seen = []
    for peak in (5.0, 4.0, 9.0):
        x = base.copy()
        x[0] = F32(peak)
        run("sg_amax_f32", In(dev, x), n, slot.ptr)
        seen.append(float(slot.read(F32)[0]))
    assert seen == [5.0, 5.0, 9.0], seen


@pytest.mark.parametrize("rowlen", [8, 24, 8 * 257])
def test_amax2_row_factors(dev, rowlen):
    """max |x| and max fl(|x| |rowscale|) in one sweep: negative factors count by magnitude; the pair accumulates over launches."""
    rows = 7
    f = factors(rows)
    for peak_row in (0, 1, 5):          # the row that holds the largest |x| has factor -0.5 / 0 / -1
        x = take(pool_fp8(3.7), rows * rowlen)
        x[peak_row * rowlen + rowlen - 1] = F32(-6.0)
        slot = Buf(dev, 8, np.zeros(2, F32))
        run("sg_amax2_f32", In(dev, x), x.size, In(dev, f), rowlen, slot.ptr)
        slot.check("amax2")
        want = L.amax2(x, f, rowlen)
        assert slot.read(F32).tolist() == [want[0], want[1]], (rowlen, peak_row, slot.read(F32), want)
        assert want[0] == F32(6.0)
        y = (x * F32(0.5)).astype(F32)          # a second, smaller tensor leaves both
        run("sg_amax2_f32", In(dev, y), y.size, In(dev, f), rowlen, slot.ptr)
        assert slot.read(F32).tolist() == [want[0], want[1]]


def test_grid_stride_bf16(dev):
    """n = 8 (4096 * 256 + 3): the sweep's second trip through its grid-stride loop, three groups long (34 MB, the largest case here)."""
    x = take(pool_bf16(), BIG)
    xi, out = In(dev, x), Buf(dev, 2 * BIG)
    run("sg_cvt_bf16", xi.ptr, out.ptr, BIG, 0, None, 8)
    out.check("sg_cvt_bf16 big")
    same_bits(out.read(np.uint16), L.cvt_bf16(x), "sg_cvt_bf16 n=%d" % BIG, None, 0x8000)


def test_grid_stride_fp8(dev):
    x = take(pool_fp8(3.7), BIG)
    xi = In(dev, x)
    xt = xi.t[:4 * BIG].view(torch.float32)
    s1, s2 = Buf(dev, 4, np.zeros(1, F32)), Buf(dev, 8, np.zeros(2, F32))
    for j in range(4):                  # the maximum at each position of the last float4, growing so that every launch must raise the slot
        xt[BIG - 4 + j] = 4.0 + j
        x[BIG - 4 + j] = F32(4.0 + j)
        run("sg_amax_f32", xi.ptr, BIG, s1.ptr)
        run("sg_amax2_f32", xi.ptr, BIG, None, 4, s2.ptr)
        assert s1.read(F32).tolist() == [4.0 + j] and s2.read(F32).tolist() == [4.0 + j] * 2, (j, s1.read(F32), s2.read(F32))
    s1.check("amax big"), s2.check("amax2 big")
    a = F32(7.0)
    out = Buf(dev, BIG)
    run("sg_cvt_fp8", xi.ptr, out.ptr, BIG, 0, s1.ptr)
    out.check("sg_cvt_fp8 big")
    want = L.cvt_fp8(x, a)
    same_bits(out.read(np.uint8), want, "sg_cvt_fp8 n=%d" % BIG, flushed(x, want))
    x16 = L.f32_to_bf16_bits(x)
    out = Buf(dev, BIG)
    run("sg_cvt_fp8_bf16", In(dev, x16), out.ptr, BIG, 0, s1.ptr)
    out.check("sg_cvt_fp8_bf16 big")
    want = L.cvt_fp8_bf16(x16, a)
    same_bits(out.read(np.uint8), want, "sg_cvt_fp8_bf16 n=%d" % BIG, flushed(L.bf16_bits_to_f32(x16), want))


# ================================================================================================================================
# [M, C] sweeps with column sums
# ================================================================================================================================
CS = [8, 24, 40, 256, 2056]          # C / 8 = 1, 3, 5, 32, 257: one column lane, counts that are no power of two, a second column pass
MS = [1, 31, 32, 33, 65]
BIG_M = 32 * 1024 + 1                # rows_per_block = 33 > 32
MC = [(M, C) for C in CS for M in MS] + [(BIG_M, 8), (BIG_M, 24)]


def row_variants(M):
    """(rowscale or None, rows_per_sample): none, one factor per row, a sample boundary inside a block, no boundary at all."""
    out = [(None, 1)]
    for rps in (1, 5, M):
        if rps <= M and all(rps != r for _, r in out[1:]):
            out.append((factors(-(-M // rps)), rps))
    return out


def check_colsum(got, d0, s, a, M, name):
    ref = d0.astype(np.float64) + s
    err = np.abs(got.astype(np.float64) - ref)
    bound = M * 2.0 ** -24 * a
    share = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print("%s: largest share of M 2^-24 sum|p| used by a column: %.3f" % (name, share))
    margins.record("dbias share of M 2^-24 sum|p|: " + name, share, 1.0)
    assert share <= 1.0, "%s: a column sum misses its bound (share %.3f; column %d)" % (name, share, int(np.argmax(err - bound)))
    return share


def start_of(s):
    return (-0.25 * s).astype(F32)


def start_and_scale(s, a):
    """-> (start values, the bound's sum of magnitudes).  Every column starts at fl(-sum / 4) except column 1, the cancelling one,
    whose sum may be exactly 0: it starts at 2^-6, and -- being one more summand of unrelated sign -- that start's magnitude joins the
    column's sum |p| (M additions of M + 1 numbers: M 2^-24 (|start| + sum |p|) is the worst case of any order)."""
    d0, a = start_of(s), a.copy()
    d0[1] = F32(2.0 ** -6)
    a[1] += 2.0 ** -6
    return d0, a


@pytest.mark.parametrize("M,C", MC, ids=["M%d-C%d" % mc for mc in MC])
def test_cvt_bf16_bias(dev, M, C):
    ops = _ops()
    x = grad_data(M, C, pool_grad16(), 7.0)
    xi = In(dev, x)
    for f, rps in row_variants(M):
        fi = None if f is None else In(dev, f)
        want, want_plain, s, a = L.cvt_bf16_bias(x, f, rps)
        d0, a = start_and_scale(s, a)
        for with_plain in (False, True):
            seen = []
            for det in (False, True, True):
                name = "sg_cvt_bf16_bias M=%d C=%d rps=%s plain=%d det=%d" % (M, C, "-" if f is None else rps, with_plain, det)
                out, plain, db = Buf(dev, 2 * M * C), Buf(dev, 2 * M * C), Buf(dev, 4 * C, d0)
                try:
                    ops.set_deterministic(det)
                    run("sg_cvt_bf16_bias", xi.ptr, out.ptr, plain.ptr if with_plain else None, M, C, None if f is None else fi.ptr, rps, db.ptr)
                finally:
                    ops.set_deterministic(False)
                for b in (out, plain, db):
                    b.check(name)
                same_bits(out.read(np.uint16), want, name + " scaled copy", None, 0x8000)
                if with_plain:
                    same_bits(plain.read(np.uint16), want_plain, name + " plain copy", None, 0x8000)
                else:
                    plain.untouched(name)
                check_colsum(db.read(F32), d0, s, a, M, name)
                if det:
                    seen.append(db.read(np.uint32).copy())
            assert np.array_equal(seen[0], seen[1]), "deterministic mode: dbias differs between two calls"


@pytest.mark.parametrize("M,C", MC, ids=["M%d-C%d" % mc for mc in MC])
def test_cvt_fp8_grad(dev, M, C):
    ops = _ops()
    A = 448.0 / 8
    x = grad_data(M, C, pool_fp8(A), A)
    xi = In(dev, x)
    for f, rps in row_variants(M):
        fi = None if f is None else In(dev, f)
        a2 = L.amax2(x, f, rps * C)
        slot = Buf(dev, 8, np.zeros(2, F32))
        run("sg_amax2_f32", xi.ptr, M * C, None if f is None else fi.ptr, rps * C, slot.ptr)
        assert slot.read(F32).tolist() == [a2[0], a2[1]], (slot.read(F32), a2)
        want5, want4, s, a = L.cvt_fp8_grad(x, a2, f, rps)
        p = x if f is None else L._mul(x, np.repeat(f, rps)[:M][:, None])
        free5, free4 = flushed(L._mul(p, L.scale_of(a2[1], 57344.0)), want5), flushed(L._mul(x, L.scale_of(a2[0], 448.0)), want4)
        d0, a = start_and_scale(s, a)
        for with4 in (False, True):
            for with_db in (False, True):
                seen = []
                for det in (False, True, True):
                    name = "sg_cvt_fp8_grad M=%d C=%d rps=%s e4m3=%d dbias=%d det=%d" % (M, C, "-" if f is None else rps, with4, with_db, det)
                    o5, o4, db = Buf(dev, M * C), Buf(dev, M * C), Buf(dev, 4 * C, d0)
                    try:
                        ops.set_deterministic(det)
                        run("sg_cvt_fp8_grad", xi.ptr, o5.ptr, o4.ptr if with4 else None, M, C, None if f is None else fi.ptr, rps, slot.ptr,
                            db.ptr if with_db else None)
                    finally:
                        ops.set_deterministic(False)
                    for b in (o5, o4, db):
                        b.check(name)
                    same_bits(o5.read(np.uint8), want5, name + " e5m2 copy", free5)
                    if with4:
                        same_bits(o4.read(np.uint8), want4, name + " e4m3 copy", free4)
                    else:
                        o4.untouched(name)
                    if with_db:
                        check_colsum(db.read(F32), d0, s, a, M, name)
                        if det:
                            seen.append(db.read(np.uint32).copy())
                    else:
                        assert np.array_equal(db.read(F32), d0), name + ": dbias written although none was passed"
                if with_db:
                    assert np.array_equal(seen[0], seen[1]), "deterministic mode: dbias differs between two calls"


@pytest.mark.parametrize("k", [0, -3, 5])
def test_cvt_fp8_grad_all_ties(dev, k):
    """The whole pool of amax = 448 * 2^k = 57344 * 2^(k - 7) as one [117, 48] gradient: every e4m3 tie reaches the e4m3 copy and every
    e5m2 tie the e5m2 copy with exact products (asserted on the data) -- without row factors and with factors of magnitude 1, which
    keep max |factor x| = amax and only flip signs."""
    A = 448.0 * 2.0 ** k
    M, C, rps = 117, 48, 13
    x = take(pool_fp8(A), M * C, A, -1).reshape(M, C)
    assert x.size == pool_fp8(A).size
    assert_holds_ties(x, A)
    xi = In(dev, x)
    for f in (None, np.resize(np.array([1.0, -1.0], F32), M // rps)):
        fi = None if f is None else In(dev, f)
        slot = Buf(dev, 8, np.zeros(2, F32))
        run("sg_amax2_f32", xi, M * C, fi, rps * C, slot)
        assert slot.read(F32).tolist() == [A, A], slot.read(F32)
        want5, want4, _, _ = L.cvt_fp8_grad(x, (F32(A), F32(A)), f, rps)
        name = "sg_cvt_fp8_grad all ties k=%d factors=%d" % (k, f is not None)
        o5, o4 = Buf(dev, M * C), Buf(dev, M * C)
        run("sg_cvt_fp8_grad", xi, o5, o4, M, C, fi, rps, slot, None)
        o5.check(name), o4.check(name)
        same_bits(o5.read(np.uint8), want5, name + " e5m2 copy", flushed(L._mul(x, L.scale_of(A, 57344.0)), want5))
        same_bits(o4.read(np.uint8), want4, name + " e4m3 copy", flushed(L._mul(x, L.scale_of(A, 448.0)), want4))


# ================================================================================================================================
# filter packing
# ================================================================================================================================
@pytest.mark.parametrize("taps", [1, 9])
@pytest.mark.parametrize("K,N", [(1, 1), (31, 33), (32, 32), (33, 31), (40, 72)])
def test_pack_filters(dev, K, N, taps):
    n = taps * K * N
    for transpose in (0, 1):
        w = take(pool_bf16(), n)
        out = Buf(dev, 2 * n)
        run("sg_pack_filter_bf16", In(dev, w), out.ptr, taps, K, N, transpose)
        name = "sg_pack_filter_bf16 %dx%dx%d transpose=%d" % (taps, K, N, transpose)
        out.check(name)
        same_bits(out.read(np.uint16), L.pack_filter_bf16(w, taps, K, N, transpose), name, None, 0x8000)
        for amax in (448.0, 448.0 / 8, 448.0 * 32, 3.7):
            w = take(pool_fp8(amax), n, amax, -1)
            if n >= 2 * pool_fp8(amax).size and scaled_ties(amax):          # (40 x 72 x 9: the pool several times over)
                assert_holds_ties(w, amax, (0,))
            name = "sg_pack_filter_fp8 %dx%dx%d transpose=%d amax=%g" % (taps, K, N, transpose, amax)
            slot = _amax_slot(dev, np.resize(w, (n + 3) // 4 * 4), name)
            out = Buf(dev, n)
            run("sg_pack_filter_fp8", In(dev, w), out.ptr, slot.ptr, taps, K, N, transpose)
            out.check(name)
            want = L.pack_filter_fp8(w, amax, taps, K, N, transpose)
            same_bits(out.read(np.uint8), want, name, flushed(L._mul(L._packed(w, taps, K, N, transpose), L.scale_of(amax, 448.0)), want))


# ================================================================================================================================
# pool backward written as operand copies
# ================================================================================================================================
POOL_SHAPES = [(1, 2, 2, 8), (3, 2, 6, 24), (2, 4, 2, 264)]


@pytest.mark.parametrize("B,H,W,C", POOL_SHAPES)
def test_avgpool2_bwd_bf16(dev, B, H, W, C):
    d = take(pool_bf16(), B * (H // 2) * (W // 2) * C).reshape(B, H // 2, W // 2, C)
    di, n = In(dev, d), B * H * W * C
    for f in (None, factors(B)):
        fi = None if f is None else In(dev, f)
        want_p, want_s = L.avgpool2_bwd_bf16(d, f)
        for has_p, has_s in ((True, True), (True, False), (False, True)):
            name = "sg_avgpool2_bwd_bf16 %s scale=%d plain=%d scaled=%d" % ((B, H, W, C), f is not None, has_p, has_s)
            op, os_ = Buf(dev, 2 * n), Buf(dev, 2 * n)
            run("sg_avgpool2_bwd_bf16", di.ptr, op.ptr if has_p else None, os_.ptr if has_s else None, None if f is None else fi.ptr, B, H, W, C)
            op.check(name), os_.check(name)
            same_bits(op.read(np.uint16), want_p, name + " plain", None, 0x8000) if has_p else op.untouched(name)
            same_bits(os_.read(np.uint16), want_s, name + " scaled", None, 0x8000) if has_s else os_.untouched(name)


ALL_TIES_POOL = (3, 4, 6, 312)          # dout [3, 2, 3, 312] = 5616 values: one whole pool_fp8


@pytest.mark.parametrize("B,H,W,C", POOL_SHAPES + [ALL_TIES_POOL])
def test_avgpool2_bwd_fp8(dev, B, H, W, C):
    """amax_dout = 4 * 448 * 2^k, k in {0, -3, 5}: amax_dx = 448 * 2^k, the scales are powers of two and 0.25 dout times the scale are
    the designed ties themselves (e5m2: in the runs without row factors); the last shape holds every one of them (asserted on the
    data).  3.7: the double rounding."""
    n = B * H * W * C
    for A in (448.0 * 4, 448.0 / 2, 448.0 * 128, 3.7):
        d = take(pool_fp8(A), n // 4, A, -1).reshape(B, H // 2, W // 2, C)
        if (B, H, W, C) == ALL_TIES_POOL and scaled_ties(A):
            assert d.size == pool_fp8(A).size
            assert_holds_ties(d, A)
        di = In(dev, d)
        for f in (None, factors(B)):
            fi = None if f is None else In(dev, f)
            a2 = L.amax2(d, f, (H // 2) * (W // 2) * C)
            a2i = In(dev, np.array(a2, F32))
            want4, want5, a_dx = L.avgpool2_bwd_fp8(d, a2, f)
            v = L._pool_bwd(d)
            p = v if f is None else L._mul(v, f[:, None, None, None])
            free4, free5 = flushed(L._mul(v, L.scale_of(a_dx[0], 448.0)), want4), flushed(L._mul(p, L.scale_of(a_dx[1], 57344.0)), want5)
            for has4, has5 in ((True, True), (True, False), (False, True)):
                name = "sg_avgpool2_bwd_fp8 %s amax=%g scale=%d e4m3=%d e5m2=%d" % ((B, H, W, C), A, f is not None, has4, has5)
                o4, o5, adx = Buf(dev, n), Buf(dev, n), Buf(dev, 8)
                run("sg_avgpool2_bwd_fp8", di.ptr, o4.ptr if has4 else None, o5.ptr if has5 else None, None if f is None else fi.ptr, a2i.ptr,
                    adx.ptr, B, H, W, C)
                for b in (o4, o5, adx):
                    b.check(name)
                assert adx.read(F32).tolist() == [a_dx[0], a_dx[1]] == [F32(0.25) * a2[0], F32(0.25) * a2[1]], name
                same_bits(o4.read(np.uint8), want4, name + " e4m3", free4) if has4 else o4.untouched(name)
                same_bits(o5.read(np.uint8), want5, name + " e5m2", free5) if has5 else o5.untouched(name)


# ================================================================================================================================
# very small amax
# ================================================================================================================================
def check_ideal(codes, x64, amax64, fmt, name):
    """No NaN code, zero -> zero, |decode(code) amax / top - x| <= amax / 28 (e4m3), amax / 14 (e5m2): half the coarsest step."""
    codes = np.asarray(codes).ravel()
    x64 = np.asarray(x64, dtype=np.float64).ravel()
    dec = L.DEC[fmt](codes)
    top, div = (448.0, 28.0) if fmt == "e4m3" else (57344.0, 14.0)
    assert np.isfinite(dec).all(), "%s: %d NaN / inf codes" % (name, int((~np.isfinite(dec)).sum()))
    err = np.abs(dec * (amax64 / top) - x64)
    nz = int(((codes & 0x7f) != 0)[x64 == 0].sum())
    print("%s: %d of %d zeros left zero; worst |error| = %.3f amax (bound %.4f amax)" % (name, int((x64 == 0).sum()) - nz, int((x64 == 0).sum()),
                                                                                      err.max() / amax64, 1.0 / div))
    assert nz == 0, "%s: %d zero inputs became non-zero codes (first code %#x)" % (name, nz, codes[(x64 == 0) & ((codes & 0x7f) != 0)][0])
    assert (err <= amax64 / div).all(), "%s: worst error %.3f amax > amax / %g" % (name, err.max() / amax64, div)


@pytest.mark.parametrize("amax", [1e-30, 1e-36, 1e-37, 2.0 ** -126], ids=["1e-30", "1e-36", "1e-37", "smallest-normal"])
def test_very_small_amax(dev, amax):
    """fl(448 / amax) overflows fp32 below amax = 448 / FLT_MAX = 1.32e-36, fl(57344 / amax) below 1.7e-34: 1e-30 is above both
    thresholds, 1e-36, 1e-37 and the smallest normal fp32 below both.  An infinite scale would send every non-zero element to the
    clamp end and every zero to 0 * inf = NaN.  Reference: the ideal fp64 scaling."""
    a = F32(amax)
    a64 = float(a)
    mags = np.array([1.0, 0.5, 0.3, 1.0, 0.5, 0.3, 0.5, 0.3]) * np.array([1, -1, 1, -1, 1, -1, -1, 1])
    x = np.zeros(64, dtype=np.float64)
    x[1::2] = np.resize(mags, 32) * a64
    x = x.astype(F32)
    x[1] = a
    x64 = x.astype(np.float64)
    xi, ai = In(dev, x), In(dev, np.array([a, a], F32))
    out = Buf(dev, 64)
    run("sg_cvt_fp8", xi.ptr, out.ptr, 64, 0, ai.ptr)
    out.check("sg_cvt_fp8")
    check_ideal(out.read(np.uint8), x64, a64, "e4m3", "sg_cvt_fp8 amax=%g" % amax)
    x16 = L.f32_to_bf16_bits(x)
    xv = L.bf16_bits_to_f32(x16)
    out = Buf(dev, 64)
    run("sg_cvt_fp8_bf16", In(dev, x16), out.ptr, 64, 0, In(dev, np.array([L.amax(xv)], F32)))
    out.check("sg_cvt_fp8_bf16")
    check_ideal(out.read(np.uint8), xv.astype(np.float64), float(L.amax(xv)), "e4m3", "sg_cvt_fp8_bf16 amax=%g" % amax)
    o5, o4 = Buf(dev, 64), Buf(dev, 64)
    run("sg_cvt_fp8_grad", xi.ptr, o5.ptr, o4.ptr, 8, 8, None, 1, ai.ptr, None)
    o5.check("sg_cvt_fp8_grad"), o4.check("sg_cvt_fp8_grad")
    check_ideal(o5.read(np.uint8), x64, a64, "e5m2", "sg_cvt_fp8_grad e5m2 amax=%g" % amax)
    check_ideal(o4.read(np.uint8), x64, a64, "e4m3", "sg_cvt_fp8_grad e4m3 amax=%g" % amax)
    out = Buf(dev, 64)
    run("sg_pack_filter_fp8", xi.ptr, out.ptr, ai.ptr, 1, 8, 8, 0)
    out.check("sg_pack_filter_fp8")
    check_ideal(out.read(np.uint8), x64, a64, "e4m3", "sg_pack_filter_fp8 amax=%g" % amax)
    o4, o5, adx = Buf(dev, 128), Buf(dev, 128), Buf(dev, 8)          # dout = the first 32 values as [1, 1, 4, 8] -> dx [1, 2, 8, 8]
    run("sg_avgpool2_bwd_fp8", xi.ptr, o4.ptr, o5.ptr, None, ai.ptr, adx.ptr, 1, 2, 8, 8)
    for b in (o4, o5, adx):
        b.check("sg_avgpool2_bwd_fp8")
    up = np.repeat(np.repeat(0.25 * x64[:32].reshape(1, 1, 4, 8), 2, axis=1), 2, axis=2)
    assert adx.read(F32).astype(np.float64).tolist() == [0.25 * a64] * 2
    check_ideal(o4.read(np.uint8), up, 0.25 * a64, "e4m3", "sg_avgpool2_bwd_fp8 e4m3 amax=%g" % amax)
    check_ideal(o5.read(np.uint8), up, 0.25 * a64, "e5m2", "sg_avgpool2_bwd_fp8 e5m2 amax=%g" % amax)


# ================================================================================================================================
# refusals
# ================================================================================================================================
def test_refusals(dev):
    """SG_ERR_ARG and untouched outputs for null pointers, n off its multiple by one, rowlen off its multiple or <= 0 with a rowscale,
    C % 8 != 0, odd H / W and a pool launch without any output."""
    x = In(dev, take(pool_fp8(3.7), 4096))
    f = In(dev, factors(8))
    a = In(dev, np.array([3.7, 3.7], F32))
    o1, o2, o3 = Buf(dev, 8192), Buf(dev, 8192), Buf(dev, 64)
    X, F, A, O1, O2, O3 = x.ptr, f.ptr, a.ptr, o1.ptr, o2.ptr, o3.ptr
    cases = [
        ("sg_cvt_bf16", (None, O1, 64, 0, None, 8)), ("sg_cvt_bf16", (X, None, 64, 0, None, 8)), ("sg_cvt_bf16", (X, O1, 63, 0, None, 8)),
        ("sg_cvt_bf16", (X, O1, 65, 0, None, 8)), ("sg_cvt_bf16", (X, O1, 64, 0, F, 9)), ("sg_cvt_bf16", (X, O1, 64, 0, F, 7)),
        ("sg_cvt_bf16", (X, O1, 64, 0, F, 0)), ("sg_cvt_bf16", (X, O1, 64, 0, F, -8)),
        ("sg_cvt_bf16_bias", (None, O1, O2, 4, 16, None, 1, O3)), ("sg_cvt_bf16_bias", (X, None, O2, 4, 16, None, 1, O3)),
        ("sg_cvt_bf16_bias", (X, O1, O2, 4, 16, None, 1, None)), ("sg_cvt_bf16_bias", (X, O1, O2, 4, 15, None, 1, O3)),
        ("sg_cvt_bf16_bias", (X, O1, O2, 4, 17, None, 1, O3)), ("sg_cvt_bf16_bias", (X, O1, O2, 4, 16, F, 0, O3)),
        ("sg_pack_filter_bf16", (None, O1, 1, 8, 8, 0)), ("sg_pack_filter_bf16", (X, None, 1, 8, 8, 1)),
        ("sg_amax_f32", (None, 64, O3)), ("sg_amax_f32", (X, 64, None)), ("sg_amax_f32", (X, 63, O3)), ("sg_amax_f32", (X, 65, O3)),
        ("sg_amax2_f32", (None, 64, None, 4, O3)), ("sg_amax2_f32", (X, 64, None, 4, None)), ("sg_amax2_f32", (X, 63, None, 4, O3)),
        ("sg_amax2_f32", (X, 65, None, 4, O3)), ("sg_amax2_f32", (X, 64, F, 5, O3)), ("sg_amax2_f32", (X, 64, F, 3, O3)),
        ("sg_amax2_f32", (X, 64, F, 0, O3)), ("sg_amax2_f32", (X, 64, F, -4, O3)),
        ("sg_cvt_fp8", (None, O1, 64, 0, A)), ("sg_cvt_fp8", (X, None, 64, 0, A)), ("sg_cvt_fp8", (X, O1, 64, 0, None)),
        ("sg_cvt_fp8", (X, O1, 63, 0, A)), ("sg_cvt_fp8", (X, O1, 65, 0, A)),
        ("sg_cvt_fp8_bf16", (None, O1, 64, 0, A)), ("sg_cvt_fp8_bf16", (X, None, 64, 0, A)), ("sg_cvt_fp8_bf16", (X, O1, 64, 0, None)),
        ("sg_cvt_fp8_bf16", (X, O1, 63, 0, A)), ("sg_cvt_fp8_bf16", (X, O1, 65, 0, A)),
        ("sg_cvt_fp8_grad", (None, O1, O2, 4, 16, None, 1, A, O3)), ("sg_cvt_fp8_grad", (X, None, O2, 4, 16, None, 1, A, O3)),
        ("sg_cvt_fp8_grad", (X, O1, O2, 4, 16, None, 1, None, O3)), ("sg_cvt_fp8_grad", (X, O1, O2, 4, 15, None, 1, A, O3)),
        ("sg_cvt_fp8_grad", (X, O1, O2, 4, 17, None, 1, A, O3)), ("sg_cvt_fp8_grad", (X, O1, O2, 4, 16, F, 0, A, O3)),
        ("sg_pack_filter_fp8", (None, O1, A, 1, 8, 8, 0)), ("sg_pack_filter_fp8", (X, None, A, 1, 8, 8, 0)), ("sg_pack_filter_fp8", (X, O1, None, 1, 8, 8, 1)),
        ("sg_avgpool2_bwd_bf16", (None, O1, O2, None, 1, 2, 2, 8)), ("sg_avgpool2_bwd_bf16", (X, None, None, None, 1, 2, 2, 8)),
        ("sg_avgpool2_bwd_bf16", (X, O1, O2, None, 1, 3, 2, 8)), ("sg_avgpool2_bwd_bf16", (X, O1, O2, None, 1, 2, 3, 8)),
        ("sg_avgpool2_bwd_bf16", (X, O1, O2, None, 1, 2, 2, 9)), ("sg_avgpool2_bwd_bf16", (X, O1, O2, None, 1, 2, 2, 7)),
        ("sg_avgpool2_bwd_fp8", (None, O1, O2, None, A, O3, 1, 2, 2, 8)), ("sg_avgpool2_bwd_fp8", (X, None, None, None, A, O3, 1, 2, 2, 8)),
        ("sg_avgpool2_bwd_fp8", (X, O1, O2, None, None, O3, 1, 2, 2, 8)), ("sg_avgpool2_bwd_fp8", (X, O1, O2, None, A, None, 1, 2, 2, 8)),
        ("sg_avgpool2_bwd_fp8", (X, O1, O2, None, A, O3, 1, 3, 2, 8)), ("sg_avgpool2_bwd_fp8", (X, O1, O2, None, A, O3, 1, 2, 3, 8)),
        ("sg_avgpool2_bwd_fp8", (X, O1, O2, None, A, O3, 1, 2, 2, 9)),
    ]
    for name, args in cases:
        assert rc_of(name, *args) == ERR_ARG, "%s%s did not return SG_ERR_ARG" % (name, args)
        for b in (o1, o2, o3):
            b.untouched("%s%s" % (name, args))


# ================================================================================================================================
# the ops wrappers at the same data
# ================================================================================================================================
def _dev32(dev, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dev)


def _host(t, dtype):
    return t.contiguous().view(torch.uint8).cpu().numpy().view(dtype)


def test_wrappers(dev):
    """ops.fp8_of, grad_operand_fp8, cvt_bf16, cvt_bf16_bias, packed_filter, packed_filter_fp8, avgpool2_bwd_operands produce the same
    bytes as the references (they pick rowlen / rows_per_sample / transpose themselves)."""
    ops = _ops()
    try:
        ops.new_step()
        B, H, W, C = 6, 2, 3, 40
        # fp8_of
        x = take(pool_fp8(3.7), 8 * 257, 3.7, -1)
        for relu in (False, True):
            got, a = ops.fp8_of(_dev32(dev, x), relu=relu)
            want = L.cvt_fp8(x, L.amax(x), relu)
            assert a.item() == float(L.amax(x))
            same_bits(_host(got, np.uint8), want, "ops.fp8_of relu=%d" % relu, free8(L._mul(x, L.scale_of(L.amax(x), 448.0)), want, x if relu else None))
        # grad_operand_fp8
        A = 448.0 / 8
        dy, f = grad_data(B * H * W, C, pool_fp8(A), A), factors(B)
        o5, a5, cs = ops.grad_operand_fp8(_dev32(dev, dy.reshape(B, H, W, C)), _dev32(dev, f), True)
        a2 = L.amax2(dy, f, H * W * C)
        want5, want4, s, a = L.cvt_fp8_grad(dy, a2, f, H * W)
        assert a5.item() == float(a2[1])
        p = L._mul(dy, np.repeat(f, H * W)[:, None])
        same_bits(_host(o5, np.uint8), want5, "ops.grad_operand_fp8", flushed(L._mul(p, L.scale_of(a2[1], 57344.0)), want5))
        check_colsum(cs.cpu().numpy(), np.zeros(C, F32), s, a, B * H * W, "ops.grad_operand_fp8")
        # cvt_bf16 / cvt_bf16_bias
        t = take(pool_bf16(), B * H * W * C)
        for relu in (False, True):
            got = ops.cvt_bf16(_dev32(dev, t.reshape(B, H, W, C)), relu=relu, rowscale=_dev32(dev, f))
            pp = L._mul(t, np.repeat(f, H * W * C))
            same_bits(_host(got, np.uint16), L.cvt_bf16(t, relu, f, H * W * C), "ops.cvt_bf16 relu=%d" % relu, ~(pp > 0) if relu else None, 0x8000)
        g = grad_data(B * H * W, C, pool_grad16(), 7.0)
        want, want_plain, s, a = L.cvt_bf16_bias(g, f, H * W)
        db = _dev32(dev, start_of(s))
        got, plain = ops.cvt_bf16_bias(_dev32(dev, g.reshape(B, H, W, C)), _dev32(dev, f), db, want_plain=True)
        same_bits(_host(got, np.uint16), want, "ops.cvt_bf16_bias", None, 0x8000)
        same_bits(_host(plain, np.uint16), want_plain, "ops.cvt_bf16_bias plain", None, 0x8000)
        check_colsum(db.cpu().numpy(), start_of(s), s, a, B * H * W, "ops.cvt_bf16_bias")
        # packed filters: [kh, kw, Cin, Cout] -> 'fwd' [tap][Cout][Cin], 'bwd' [tap][Cin][Cout]
        kh, kw, Cin, Cout = 3, 3, 33, 31
        w = take(pool_bf16(), kh * kw * Cin * Cout)
        wd = _dev32(dev, w.reshape(kh, kw, Cin, Cout))
        same_bits(_host(ops.packed_filter(wd, "fwd"), np.uint16), L.pack_filter_bf16(w, 9, Cin, Cout, 1), "ops.packed_filter fwd", None, 0x8000)
        same_bits(_host(ops.packed_filter(wd, "bwd"), np.uint16), L.pack_filter_bf16(w, 9, Cout, Cin, 0), "ops.packed_filter bwd", None, 0x8000)
        n8 = kh * kw * 32 * 40
        w = take(pool_fp8(3.7), n8, 3.7, -1)
        wd = _dev32(dev, w.reshape(kh, kw, 32, 40))
        for kind, (K, N, tr) in (("fwd", (32, 40, 1)), ("bwd", (40, 32, 0))):
            got, a = ops.packed_filter_fp8(wd, kind)
            want = L.pack_filter_fp8(w, 3.7, 9, K, N, tr)
            assert a.item() == float(F32(3.7))
            same_bits(_host(got, np.uint8), want, "ops.packed_filter_fp8 " + kind, flushed(L._mul(L._packed(w, 9, K, N, tr), L.scale_of(3.7, 448.0)), want))
        # avgpool2_bwd_operands: bf16 mode C = 64, fp8 mode C = 256
        for mode, Cp in (("bf16", 64), ("fp8", 256)):
            ops.set_conv_dtype(mode)
            Bp, Ho, Wo = 3, 1, 3
            A = 448.0 / 2
            d = take(pool_fp8(A), Bp * Ho * Wo * Cp, A, -1).reshape(Bp, Ho, Wo, Cp)
            fp = factors(Bp)
            dd, fd = _dev32(dev, d), _dev32(dev, fp)
            gh = ops.avgpool2_bwd_operands(dd, fd, True)
            assert ops._is_ghost(gh), "the pooled-gradient handle carries no ghost mark (%s mode)" % mode
            with pytest.raises(RuntimeError):       # no fp32 contents, and no e4m3 copy of relu(d_c2) was asked of the producer
                ops.fp8_of(gh, relu=True)
            if mode == "bf16":
                want_p, want_s = L.avgpool2_bwd_bf16(d, fp)
                same_bits(_host(ops.bf16_of(gh), np.uint16), want_p, "ops.avgpool2_bwd_operands bf16 plain", None, 0x8000)
                same_bits(_host(ops.grad_operand(gh, fd, True)[0], np.uint16), want_s, "ops.avgpool2_bwd_operands bf16 scaled", None, 0x8000)
            else:
                a2 = L.amax2(d, fp, Ho * Wo * Cp)
                want4, want5, a_dx = L.avgpool2_bwd_fp8(d, a2, fp)
                v = L._pool_bwd(d)
                pv = L._mul(v, fp[:, None, None, None])
                o5, a5, _ = ops.grad_operand_fp8(gh, fd, True)
                o4, a4 = ops.fp8_of(gh)
                assert [a4.item(), a5.item()] == [float(a_dx[0]), float(a_dx[1])]
                same_bits(_host(o4, np.uint8), want4, "ops.avgpool2_bwd_operands e4m3", flushed(L._mul(v, L.scale_of(a_dx[0], 448.0)), want4))
                same_bits(_host(o5, np.uint8), want5, "ops.avgpool2_bwd_operands e5m2", flushed(L._mul(pv, L.scale_of(a_dx[1], 57344.0)), want5))
    finally:
        ops.set_conv_dtype("f32")
        ops.new_step()
        ops.end_step()
