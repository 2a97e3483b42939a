"""fp64 references of the convolutions' epilogue contract (include/scrabble_hip.h) composed on top of oracle.scrabble_oracle.conv2d /
conv2d_transpose, and the input / guard-buffer helpers of tests/test_conv_flags_gpu.py (test infrastructure; torch-CPU unless a
device is passed in).

Every reference returns the CONV TERM (the fp64 convolution + biases, before mask / accumulate / output activation) beside the full
result: the parity checks measure their error against max |conv term|, so a large accumulate operand cannot hide a wrong
convolution."""
import math

import torch

from oracle import scrabble_oracle as O

EPS32 = 2.0 ** -24          # half an ulp of fp32, relative: the rounding of ONE fp32 addition prev + conv


def f32(t):
    """fp64 tensor holding fp32-representable values (what the GPU receives is exactly what the oracle sees)."""
    return t.float().double()


def rnd(gen, *shape):
    return f32(torch.randn(*shape, generator=gen, dtype=torch.float64))


def make_mask(gen, *shape):
    """A ReLU-mask operand with every kind of entry: positives, negatives, +0.0 and -0.0 (a tenth each of the two zeros)."""
    m = torch.randn(*shape, generator=gen, dtype=torch.float64).float()
    sel = torch.rand(*shape, generator=gen, dtype=torch.float64)
    m[sel < 0.1] = 0.0
    m[(sel >= 0.1) & (sel < 0.2)] = -0.0
    return m


def check_mask(m):
    """At least a quarter non-positive, at least a quarter positive, both zeros and a negative present."""
    n = m.numel()
    bits = m.contiguous().view(torch.int32)
    assert (m <= 0).sum().item() * 4 >= n and (m > 0).sum().item() * 4 >= n, "mask lacks a quarter of one kind"
    assert (bits == 0).any() and (bits == -2 ** 31).any() and (m < 0).any() and (m > 0).any(), "mask lacks +0.0 / -0.0 / a negative / a positive"


def make_prev(gen, shape, term_scale, big):
    """The accumulate operand: max |prev| = term_scale (big: 100 x term_scale), normally distributed."""
    p = torch.randn(*shape, generator=gen, dtype=torch.float64)
    return f32(p * ((100.0 if big else 1.0) * term_scale / p.abs().max().item()))


def bound(tol, term, prev=None):
    """tol * max |conv term| (+ 2^-24 * max |prev|: the fp32 rounding of prev + conv itself, which no kernel can avoid)."""
    return tol * term.abs().max().item() + (EPS32 * prev.abs().max().item() if prev is not None else 0.0)


# ---- operand roundings of the low-precision routes (what the kernels' conversion sweeps do, on the host) -------------------------
def r16(t):
    return t.detach().float().to(torch.bfloat16).to(torch.float64)


def q8(t, relu=False):
    """sg_amax_f32 + sg_cvt_fp8 / sg_pack_filter_fp8: e4m3(clamp(relu?(v) * 448 / amax)) dequantised (fp64).  The amax is taken
    over t itself, the ReLU folded into the conversion."""
    t32 = t.detach().float()
    amax = t32.abs().max()
    s = (torch.tensor(448.0) / amax).float() if amax > 0 else torch.tensor(1.0)
    v = torch.relu(t32) if relu else t32
    q = (v * s).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float64)
    return q * (amax.double() / 448.0)


def q5(t, amax=None):
    """sg_cvt_fp8_grad's e5m2 operand dequantised: e5m2(clamp(v * 57344 / amax)) (v already carries its row factor)."""
    t32 = t.detach().float()
    amax = t32.abs().max() if amax is None else amax
    s = (torch.tensor(57344.0) / amax.float()).float() if amax > 0 else torch.tensor(1.0)
    return (t32 * s).clamp(-57344.0, 57344.0).to(torch.float8_e5m2).to(torch.float64) * (amax.double() / 57344.0)


def operands(rounding, a, w, relu=False):
    """The two matrix operands as the route's kernels see them: 'f32' exact, 'bf16' round-to-nearest-even, 'fp8' per-tensor e4m3."""
    if rounding == "f32":
        return (torch.relu(a) if relu else a), w
    if rounding == "bf16":
        return r16(torch.relu(a) if relu else a), r16(w)
    assert rounding == "fp8"
    return q8(a, relu), q8(w)


# ---- the flag contract ---------------------------------------------------------------------------------------------------------
def fwd(x, w, bias=None, bias2=None, relu_in=False, relu_out=False, tanh_out=False, prev=None, same=True, rounding="f32"):
    """sg_conv2d_fwd: y = act(conv(relu?(x), w) + bias + bias2 (+ prev)), act = ReLU / tanh AFTER the accumulate.  -> (term, y)"""
    a, wq = operands(rounding, x, w, relu_in)
    term = O.conv2d(a, wq, None, padding="same" if same else "valid")
    for b in (bias, bias2):
        if b is not None:
            term = term + b
    y = term if prev is None else term + prev
    if relu_out:
        y = torch.relu(y)
    if tanh_out:
        y = torch.tanh(y)
    return term, y


def dgrad(dy, w, in_hw, mask=None, prev=None, same=True, rounding="f32"):
    """sg_conv2d_bwd_data: dx = (mask > 0 ? conv_data_grad(dy, w) : 0) (+ prev); w [kh,kw,Cin,Cout].  -> (term, keep, dx)"""
    d, wq = operands(rounding, dy, w)
    xz = torch.zeros(dy.shape[0], in_hw[0], in_hw[1], w.shape[2], dtype=torch.float64, requires_grad=True)
    O.conv2d(xz, wq, None, padding="same" if same else "valid").backward(d)
    term = xz.grad
    keep = torch.ones_like(term, dtype=torch.bool) if mask is None else (mask > 0)
    dx = term * keep
    return term, keep, (dx if prev is None else dx + prev)


def wgrad(x, dy, wshape, relu_in=False, sample_scale=None, same=True, rounding="f32"):
    """sg_conv2d_bwd_weight: (dw, db) of sum_b sample_scale[b] <conv(relu?(x_b), w), dy_b>.  The low-precision kernels round relu(x)
    and the fp32 product sample_scale[b] * dy; the bias gradient sums the fp32 products."""
    dys = dy if sample_scale is None else f32(dy.float() * sample_scale.float().view(-1, 1, 1, 1))
    a = torch.relu(x) if relu_in else x
    if rounding == "bf16":
        a, d = r16(a), r16(dys)
    elif rounding == "fp8":
        a, d = q8(x, relu_in), q5(dys)
    else:
        d = dys
    wz = torch.zeros(*wshape, dtype=torch.float64, requires_grad=True)
    O.conv2d(a, wz, None, padding="same" if same else "valid").backward(d)
    return wz.grad, dys.sum(dim=(0, 1, 2))


def t_fwd(x, w, bias=None, bias2=None, stride=(2, 2), prev=None, rounding="f32"):
    """sg_conv2d_transpose_fwd: y = conv_transpose(x, w) + bias + bias2 (+ prev); w [kh,kw,Cout,Cin].  -> (term, y)"""
    a, wq = operands(rounding, x, w)
    term = O.conv2d_transpose(a, wq, None, stride)
    for b in (bias, bias2):
        if b is not None:
            term = term + b
    return term, (term if prev is None else term + prev)


def t_dgrad(dy, w, stride=(2, 2), mask=None, prev=None, rounding="f32"):
    d, wq = operands(rounding, dy, w)
    sh, sw = stride
    xz = torch.zeros(dy.shape[0], dy.shape[1] // sh, dy.shape[2] // sw, w.shape[3], dtype=torch.float64, requires_grad=True)
    O.conv2d_transpose(xz, wq, None, stride).backward(d)
    term = xz.grad
    keep = torch.ones_like(term, dtype=torch.bool) if mask is None else (mask > 0)
    dx = term * keep
    return term, keep, (dx if prev is None else dx + prev)


def t_wgrad(x, dy, wshape, stride=(2, 2), rounding="f32"):
    a, d = (r16(x), r16(dy)) if rounding == "bf16" else (x, dy)
    wz = torch.zeros(*wshape, dtype=torch.float64, requires_grad=True)
    O.conv2d_transpose(a, wz, None, stride).backward(d)
    return wz.grad


# ---- an output inside a larger buffer ------------------------------------------------------------------------------------------
SENTINEL = -1234.5678


class Guarded:
    """A contiguous fp32 tensor of `shape` between two guard blocks of SENTINEL, each one 256-row tile of the output's rows
    (256 * shape[-1] floats, at least 1024).  check() asserts that both guards are bitwise what they were."""

    def __init__(self, shape, device, init=None):
        n = int(math.prod(shape))
        self.g = max(256 * int(shape[-1]), 1024)
        self.buf = torch.full((2 * self.g + n,), SENTINEL, device=device, dtype=torch.float32)
        self.t = self.buf[self.g:self.g + n].view(*shape)
        if init is not None:
            self.t.copy_(init.float())
        self.ref = torch.full((self.g,), SENTINEL, dtype=torch.float32).view(torch.int32)

    def check(self, name=""):
        before = self.buf[:self.g].cpu().view(torch.int32)
        after = self.buf[self.g + self.t.numel():].cpu().view(torch.int32)
        assert torch.equal(before, self.ref), "%s: the launch wrote in front of its output" % name
        assert torch.equal(after, self.ref), "%s: the launch wrote behind its output" % name
