"""Edge shapes and dynamic range of the NON-convolution kernels against the fp64 oracle.

tests/test_ops_gpu.py holds BatchNorm, softmax + CTC, the loss head, Adam / RMSprop, attention and the pooling / elementwise
sweeps to the oracle at one friendly shape each with N(0,1)-sized data; tests/test_fullsize_nonconv_gpu.py repeats that at the
step's launch geometry.  This file runs the branches neither reaches: channel counts whose float4 column count is no power of
two (idle threads beside the row lanes), fewer rows than lanes, one row, tails of 1..3 elements, lengths shorter than the
buffers, the kernels' own size limits, refusals, and data at the ends of the number range (means far from zero, softmax
underflow, logits of several hundred, the hinge kink, saturated sigmoids, signed zeros, pooling windows of equal values).

Bounds are those of the tests the bodies come from (`close`: max|gpu - ref| <= tol * max|ref|); where a reference is zero or a
bound is derived, the test says how.  Operands whose rounding to fp32 would otherwise be charged to the kernel (logits of
several hundred, means of 8 under a deviation of 0.05, the optimizers' beta / rho) are rounded to fp32 BEFORE the fp64
reference is evaluated: the reference then sees exactly the numbers the kernel sees."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import legibility_refs as R  # noqa: E402
from tests import margins  # noqa: E402
from tests.test_ops_gpu import close, g32, rnd  # noqa: E402

from oracle import scrabble_oracle as O  # noqa: E402  (checker only)


def _gen(seed=1234):
    return torch.Generator().manual_seed(seed)


def _f32(t):
    """The fp64 tensor of the values `t` has after rounding to fp32 (operand-rounded reference inputs)."""
    return t.float().double()


def _f32s(v):
    return float(torch.tensor(v, dtype=torch.float32).item())


def _within(got, ref, allow, name):
    """|got - ref| <= allow elementwise (allow: a number or a tensor); the largest used share of it goes on record."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    allow = torch.as_tensor(allow, dtype=torch.float64).expand_as(ref)
    share = ((got - ref).abs() / allow.clamp_min(1e-300)).max().item()
    margins.record(name, share, 1.0)
    assert share <= 1.0, "%s: the error uses %.3f of its allowance" % (name, share)


class _deterministic:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from scrabble_gan_amd import ops
        if self.on:
            ops.set_deterministic(True)

    def __exit__(self, *exc):
        from scrabble_gan_amd import ops
        if self.on:
            ops.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ 1. BatchNorm
BN_SHAPES = [
    (3, 4, 10, 48), (2, 3, 7, 96), (2, 5, 5, 192),   # C/4 = 12 / 24 / 48: 16 / 8 / 4 row lanes, 64 idle threads beside them
    (2, 3, 5, 4),                                    # C = 4: 256 row lanes, 30 rows
    (1, 1, 3, 4),                                    # fewer rows than lanes
    (2, 2, 3, 1024),                                 # one row lane (no tree): the widest channel count the kernels take
    (1, 1, 1, 64),                                   # one row: var = 0, rstd = 1 / sqrt(eps)
    (1, 3, 11, 64), (5, 1, 13, 64),                  # 33 / 65 rows: one past a statistics block (32 rows); HW = 33 / 13 off the
]                                                    # backward's 16-row blocks


def _bn_case(dev, gen, B, H, W, C, per_sample, relu):
    """The body of test_ops_gpu.test_batchnorm at a free shape (same bounds); M = 1 has its own dx check (the reference is 0)."""
    from scrabble_gan_amd import ops
    x = (rnd(gen, B, H, W, C) * 1.7 + 0.3).requires_grad_(True)
    gamma = rnd(gen, B if per_sample else 1, C).requires_grad_(True)
    beta = rnd(gen, B if per_sample else 1, C).requires_grad_(True)
    x_hat, mean, var = O.batch_norm_train(x)
    y = x_hat * gamma.view(-1, 1, 1, C) + beta.view(-1, 1, 1, C)
    if relu:
        y = torch.relu(y)
    dy = rnd(gen, B, H, W, C)
    y.backward(dy)
    xg, gg, bg, dyg = g32(x, dev), g32(gamma, dev), g32(beta, dev), g32(dy, dev)
    sums = ops.bn_stats_sums(xg)
    assert sums.dtype == torch.float64 and sums.shape == (2 * C,)          # the SyncBN contract: fp64 sums ranks can all-reduce
    n = B * H * W
    mg, vg = ops.bn_stats_finalize(sums, n, xg)
    close(mg, mean, name="mean")
    close(vg, var, name="var")
    yg = ops.bn_apply(xg, mg, vg, gg, bg, per_sample, relu)
    close(yg, y, name="apply")
    dgam, dbet, chan = ops.bn_bwd_reduce(dyg, yg, xg, mg, vg, gg, per_sample, relu)
    dxg = ops.bn_bwd_apply(dyg, yg, xg, mg, vg, gg, per_sample, chan, n, relu, True)
    if n == 1:
        # x_hat = 0 and dz * gamma - mean(dz * gamma) = 0: the oracle's dx is identically zero and `close` has no scale
        scale = (dy * gamma.detach().view(-1, 1, 1, C)).abs().max().item() / math.sqrt(O.BN_EPS)
        err = dxg.double().abs().max().item()
        assert x.grad.abs().max().item() == 0.0 and math.isfinite(err)
        margins.record("dx (M = 1)", err / scale, 5e-5)
        assert err <= 5e-5 * scale, (err, scale)
    else:
        close(dxg, x.grad, tol=5e-5, name="dx")
    if per_sample:
        close(dgam, gamma.grad, tol=5e-5, name="dgamma")
        close(dbet, beta.grad, tol=5e-5, name="dbeta")
    else:
        close(chan[2 * C:3 * C].float(), gamma.grad[0], tol=5e-5, name="dgamma_c")
        close(chan[3 * C:].float(), beta.grad[0], tol=5e-5, name="dbeta_c")
    # inference-mode BN backward (frozen recognizer): dx = dz * gamma * rstd
    mm, mv = rnd(gen, C) * 0.1, torch.rand(C, generator=gen, dtype=torch.float64) + 0.5
    xr = x.detach().clone().requires_grad_(True)
    g1, b1 = gamma.detach()[0], beta.detach()[0]
    yi = (xr - mm) * torch.rsqrt(mv + O.BN_EPS) * g1 + b1
    yi.backward(dy)
    mmg, mvg, g1g, b1g = g32(mm, dev), g32(mv, dev), g32(g1, dev), g32(b1, dev)
    close(ops.bn_apply(xg, mmg, mvg, g1g, b1g, False, False), yi, name="inference apply")
    close(ops.bn_bwd_apply(dyg, None, xg, mmg, mvg, g1g, False, None, 1, False, False), xr.grad, name="inference dx")
    # moving statistics (Bessel's correction needs two rows)
    m0, v0 = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    ops.bn_update_moving(m0, v0, mg, vg, n)
    close(m0, 0.01 * mean, name="mm")
    close(v0, 0.99 + 0.01 * var * (n / (n - 1) if n > 1 else 1.0), name="mv")


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("per_sample", [True, False])
@pytest.mark.parametrize("B,H,W,C", BN_SHAPES)
def test_batchnorm_edge_shapes(dev, B, H, W, C, per_sample, relu):
    _bn_case(dev, _gen(), B, H, W, C, per_sample, relu)


@pytest.mark.parametrize("per_sample,relu", [(True, True), (False, False)])
@pytest.mark.parametrize("B,H,W,C", [(3, 4, 10, 48), (2, 2, 3, 1024)])
def test_batchnorm_edge_shapes_deterministic(dev, B, H, W, C, per_sample, relu):
    """One workgroup per sample in the backward reduce (rows_per_block = HW) at C/4 = 12 and at one row lane."""
    from scrabble_gan_amd import ops
    ops.set_deterministic(True)
    try:
        _bn_case(dev, _gen(), B, H, W, C, per_sample, relu)
    finally:
        ops.set_deterministic(False)


@pytest.mark.parametrize("std,offset", [(1.0, 8.0), (0.05, 3.0)])
def test_batchnorm_mean_far_from_zero(dev, std, offset):
    """The statistics kernel accumulates sum x and sum x^2 in fp32 per block and finishes E[x^2] - mean^2 in fp64, so its
    variance error is relative to E[x^2] = mean^2 + var, not to var: |var_gpu - var_ref| <= 2e-5 * max_c(mean^2 + var).  (A plain
    fp32 E[x^2] - mean^2 at offset 8 is off by 1.8e-5 of var, i.e. 3e-7 of E[x^2], on the CPU: the bound is far from the
    reference's own error.)  The error relative to var itself goes on record under its own name."""
    from scrabble_gan_amd import ops
    gen = _gen()
    B, H, W, C = 4, 8, 10, 64
    x = _f32(rnd(gen, B, H, W, C) * std + offset)
    gamma, beta = _f32(rnd(gen, B, C)), _f32(rnd(gen, B, C))
    x_hat, mean, var = O.batch_norm_train(x)
    y = x_hat * gamma.view(-1, 1, 1, C) + beta.view(-1, 1, 1, C)
    xg = g32(x, dev)
    mg, vg = ops.bn_stats_finalize(ops.bn_stats_sums(xg), B * H * W, xg)
    close(mg, mean, name="mean")
    dv = 2e-5 * (mean * mean + var).max().item()
    verr = (vg.double().cpu() - var).abs().max().item()
    print("std %g offset %g: max var error %.3e = %.3e of max var, bound %.3e" % (std, offset, verr, verr / var.max().item(), dv))
    margins.record("var error / max(mean^2 + var)", verr / (mean * mean + var).max().item(), 2e-5)
    margins.record("var error / max var", verr / var.max().item(), dv / var.max().item())
    assert torch.isfinite(vg).all() and verr <= dv, (verr, dv)
    # apply: y = (x - mean) * rstd * gamma + beta with rstd = (var + eps)^(-1/2), so d rstd / rstd = -d var / (2 (var + eps)) and a
    # variance error of up to dv moves y by up to |(x - mean) * rstd * gamma| * dv / (2 (var + eps)) = |x_hat * gamma| * dv / (2 (var + eps))
    allow = 2e-5 * y.abs().max().item() + (x_hat * gamma.view(-1, 1, 1, C)).abs() * dv / (2.0 * (var + O.BN_EPS))
    _within(ops.bn_apply(xg, mg, vg, g32(gamma, dev), g32(beta, dev), True, False), y, allow, "apply (2e-5 + implied rstd error)")


def test_bn_update_moving_edges(dev):
    from scrabble_gan_amd import ops
    gen, C = _gen(), 48
    mean, var = _f32(rnd(gen, C)), _f32(torch.rand(C, generator=gen, dtype=torch.float64) + 0.1)
    mm0, mv0 = _f32(rnd(gen, C)), _f32(torch.rand(C, generator=gen, dtype=torch.float64) + 0.5)
    mg, vg = g32(mean, dev), g32(var, dev)
    for count, mom, name in ((1, 0.99, "count 1"), (12, 0.5, "momentum 0.5"), (12, 0.0, "momentum 0"), (1, 0.0, "momentum 0, count 1")):
        corr = count / (count - 1.0) if count > 1 else 1.0               # count = 1: no Bessel correction
        mm, mv = g32(mm0, dev), g32(mv0, dev)
        ops.bn_update_moving(mm, mv, mg, vg, count, mom)
        close(mm, mom * mm0 + (1 - mom) * mean, tol=1e-6, name="mm, " + name)
        close(mv, mom * mv0 + (1 - mom) * var * corr, tol=1e-6, name="mv, " + name)
        if mom == 0.0 and count == 1:        # the standing-statistics first step i / (i + 1) at i = 0: the batch values themselves
            assert torch.equal(mm, mg) and torch.equal(mv, vg)


@pytest.mark.parametrize("C", [6, 1028])
def test_bn_stats_refuses_channel_counts(dev, C):
    """C % 4 != 0 and C / 4 > 256 (more float4 columns than threads) are refused on the host: SG_ERR_ARG, nothing is launched."""
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import ScrabbleHipError
    with pytest.raises(ScrabbleHipError, match="SG_ERR_ARG"):
        ops.bn_stats_sums(torch.zeros(2, 3, C, device=dev))


# ------------------------------------------------------------------------------------------------ 2. softmax + CTC
def _ctc_ref(logits, labels, T_in, L, dtype=torch.float64):
    lg = logits.to(dtype).clone().requires_grad_(True)
    cost = O.ctc_batch_cost(labels, torch.softmax(lg, -1), T_in, L)
    cost.sum().backward()
    return cost[:, 0].detach(), lg.grad


def _ctc_gpu(dev, logits, labels, T_in, L, need_grad=True):
    from scrabble_gan_amd import ops
    return ops.softmax_ctc(g32(logits, dev), labels.int().to(dev).contiguous(), T_in, L, need_grad)


def _ctc_problem(gen, B, T, C, L, gain=2.0):
    logits = _f32(rnd(gen, B, T, C) * gain)
    labels = torch.randint(0, C - 1, (B, L), generator=gen)
    labels[0, :] = labels[0, 0]          # repeated characters force the blank transitions
    return logits, labels


@pytest.mark.parametrize("B,T,C,L,T_in", [(4, 11, 53, 2, 7), (3, 9, 6, 4, 8)])
def test_ctc_input_length_below_T(dev, B, T, C, L, T_in):
    logits, labels = _ctc_problem(_gen(), B, T, C, L)
    cost, grad = _ctc_ref(logits, labels, T_in, L)
    assert grad[:, T_in:].abs().max().item() == 0.0
    loss, dl = _ctc_gpu(dev, logits, labels, T_in, L)
    close(loss, cost, name="ctc loss")
    close(dl, grad, tol=1e-4, name="ctc dlogits")
    assert (dl[:, T_in:] == 0).all()                     # frames past input_length: exactly zero


def test_ctc_label_buffer_wider_than_label_length(dev):
    """labels [B, 8] with label_length 3: the unused columns (here -1 and C + 5) are never read -- bitwise the result of the
    call on the first three columns, and no sample is poisoned by them."""
    B, T, C, L = 4, 11, 53, 3
    logits, lab3 = _ctc_problem(_gen(), B, T, C, L)
    wide = torch.full((B, 8), -1, dtype=torch.int64)
    wide[:, 5:] = C + 5
    wide[:, :L] = lab3
    loss_w, dl_w = _ctc_gpu(dev, logits, wide, T, L)
    loss_n, dl_n = _ctc_gpu(dev, logits, lab3, T, L)
    assert torch.equal(loss_w, loss_n) and torch.equal(dl_w, dl_n)
    cost, grad = _ctc_ref(logits, lab3, T, L)
    close(loss_w, cost, name="ctc loss")
    close(dl_w, grad, tol=1e-4, name="ctc dlogits")


def test_ctc_widest_label_and_class_count(dev):
    """L = 31 (S = 63 of 64 lanes), C = 64 (every lane a class), T = 123: about 122 KB of dynamic LDS.  The gradient bound is not
    taken from the kernel: the oracle itself, evaluated in float32 on the same inputs, is off from its fp64 self by 2.8e-4 of
    max|grad| (seed 1, computed below on every run); the kernel runs the same fp32 log-space recursion lengths in another
    summation order and is allowed four times that figure.  Measured: fp32 oracle 2.775e-4, kernel on the MI355X 2.736e-4
    (a quarter of its allowance of 1.11e-3)."""
    B, T, C, L = 4, 123, 64, 31
    logits, labels = _ctc_problem(_gen(1), B, T, C, L)
    cost, grad = _ctc_ref(logits, labels, T, L)
    cost32, grad32 = _ctc_ref(logits, labels, T, L, torch.float32)
    ref32 = (grad32.double() - grad).abs().max().item() / grad.abs().max().item()
    loss, dl = _ctc_gpu(dev, logits, labels, T, L)
    kern = (dl.double().cpu() - grad).abs().max().item() / grad.abs().max().item()
    print("L = 31 gradient error / max|grad|: fp32 oracle %.3e, kernel %.3e" % (ref32, kern))
    margins.record("ctc dlogits, fp32 oracle vs fp64 oracle (no bound: the yardstick)", ref32, ref32)
    assert 1e-5 < ref32 < 1e-3, ref32                # the yardstick itself: an fp32 recursion over 123 frames, not a free parameter
    close(loss, cost, name="ctc loss")
    close(dl, grad, tol=4 * ref32, name="ctc dlogits (4 x fp32 oracle)")


def test_ctc_two_classes(dev):
    B, T, C, L = 3, 9, 2, 3                             # one character plus blank: every label is 0
    logits = _f32(rnd(_gen(), B, T, C) * 2)
    labels = torch.zeros(B, L, dtype=torch.int64)
    cost, grad = _ctc_ref(logits, labels, T, L)
    loss, dl = _ctc_gpu(dev, logits, labels, T, L)
    close(loss, cost, name="ctc loss")
    close(dl, grad, tol=1e-4, name="ctc dlogits")


def test_ctc_single_path(dev):
    """T = L = 5, five distinct labels: the only alignment is one label per frame, so loss = -sum_t lp[t, label_t]."""
    B, T, C, L = 3, 5, 53, 5
    gen = _gen()
    logits = _f32(rnd(gen, B, T, C) * 2)
    labels = torch.stack([torch.randperm(C - 1, generator=gen)[:L] for _ in range(B)])
    cost, grad = _ctc_ref(logits, labels, T, L)
    lp = torch.from_numpy(R.log_probs_ref(logits.numpy()))
    by_hand = -lp.gather(2, labels.view(B, T, 1)).sum((1, 2))
    assert (by_hand - cost).abs().max().item() < 1e-9
    loss, dl = _ctc_gpu(dev, logits, labels, T, L)
    close(loss, cost, name="ctc loss")
    close(loss, by_hand, name="ctc loss vs -sum lp")
    close(dl, grad, tol=1e-4, name="ctc dlogits")


def test_ctc_every_row_repeats(dev):
    B, C, L = 4, 53, 10
    T = 4 * L - 1
    logits, labels = _ctc_problem(_gen(), B, T, C, L)
    labels[:] = labels[:, :1]                           # aaaaaaaaaa: a blank between every pair
    cost, grad = _ctc_ref(logits, labels, T, L)
    loss, dl = _ctc_gpu(dev, logits, labels, T, L)
    close(loss, cost, name="ctc loss")
    close(dl, grad, tol=1e-4, name="ctc dlogits")


def test_ctc_saturated_logits(dev):
    """30 * randn: the fp32 softmax underflows to exact zeros, log(p + 1e-7) sits on its floor and the gradient divides by
    p + 1e-7 with p = 0.  The oracle is finite there (costs of 140..160, max|grad| about 1); same bounds as everywhere."""
    B, T, C, L = 2, 11, 53, 3
    logits, labels = _ctc_problem(_gen(), B, T, C, L, gain=30.0)
    assert (torch.softmax(logits.float(), -1) == 0).any()
    cost, grad = _ctc_ref(logits, labels, T, L)
    assert torch.isfinite(cost).all() and torch.isfinite(grad).all()
    loss, dl = _ctc_gpu(dev, logits, labels, T, L)
    close(loss, cost, name="ctc loss")
    close(dl, grad, tol=1e-4, name="ctc dlogits")


def test_ctc_infeasible_alignment(dev):
    """[1, 1, 2] needs four frames (a blank between the repeats) and gets three: cost +inf.  The oracle's autograd then turns the
    whole batch's gradient to NaN, so the feasible sample is checked against an oracle call of its own; the infeasible sample's
    gradient is exactly zero (no state carries probability mass: the kernel's `acc == -inf` branch, and what TF returns)."""
    B, T, C, L = 2, 3, 6, 3
    logits = _f32(rnd(_gen(), B, T, C) * 2)
    labels = torch.tensor([[1, 1, 2], [0, 1, 2]])
    cost, _ = _ctc_ref(logits, labels, T, L)
    assert cost[0].item() == math.inf and math.isfinite(cost[1].item())
    cost1, grad1 = _ctc_ref(logits[1:], labels[1:], T, L)
    loss, dl = _ctc_gpu(dev, logits, labels, T, L)
    assert torch.equal(torch.isposinf(loss).cpu(), torch.isposinf(cost))
    close(loss[1:], cost[1:], name="ctc loss (feasible sample)")
    close(dl[1:], grad1, tol=1e-4, name="ctc dlogits (feasible sample)")
    assert torch.isfinite(dl[0]).all() and (dl[0] == 0).all()


def test_ctc_poisoned_labels(dev):
    """A label equal to the blank (C - 1) or negative: that sample's cost is +inf and its gradient rows are all NaN (never train on
    a clamped target); its neighbours in the batch are untouched."""
    B, T, C, L = 4, 11, 53, 3
    logits, labels = _ctc_problem(_gen(), B, T, C, L)
    labels[1, 1] = C - 1
    labels[2, 2] = -1
    clean = [0, 3]
    cost, grad = _ctc_ref(logits[clean], labels[clean], T, L)
    loss, dl = _ctc_gpu(dev, logits, labels, T, L)
    assert torch.isposinf(loss[[1, 2]]).all() and torch.isnan(dl[[1, 2]]).all()
    close(loss[clean], cost, name="ctc loss (clean samples)")
    close(dl[clean], grad, tol=1e-4, name="ctc dlogits (clean samples)")
    loss2, none = _ctc_gpu(dev, logits, labels, T, L, need_grad=False)
    assert none is None and torch.equal(loss2, loss)


def test_ctc_refusals(dev):
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import ScrabbleHipError
    B, T, C = 2, 9, 53
    lg, lab = torch.zeros(B, T, C, device=dev), torch.zeros(B, 4, dtype=torch.int32, device=dev)
    for T_in, L in ((T, 0), (T + 1, 2), (T, 5)):                  # the wrapper: lengths outside the buffers
        with pytest.raises(ValueError):
            ops.softmax_ctc(lg, lab, T_in, L)
    with pytest.raises(ScrabbleHipError, match="SG_ERR_ARG"):     # the kernel's own limits: S = 2 L + 1 <= 64 states, C <= 64 classes
        ops.softmax_ctc(torch.zeros(B, 127, C, device=dev), torch.zeros(B, 32, dtype=torch.int32, device=dev), 127, 32)
    with pytest.raises(ScrabbleHipError, match="SG_ERR_ARG"):
        ops.softmax_ctc(torch.zeros(B, T, 65, device=dev), lab, T, 2)


# ------------------------------------------------------------------------------------------------ 3. Adam / RMSprop
# beta_1, beta_2 and rho reach the kernels as fp32 arguments (as in TF, which casts them to the variable's type), and
# 1 - float32(0.999) differs from 0.001 by 1.3e-5 of itself: the references below take the fp32-rounded values as THE
# hyper-parameters, so that v is compared at 1e-6 against the update the kernel was asked for.
def _adam_ref(p, grads, lr_ts, b1, b2, eps=1e-7):
    p, m, v = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
    for g, lr_t in zip(grads, lr_ts):
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr_t * m / (v.sqrt() + eps)
    return p, m, v


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1021, 4097])      # tails of 1..3 after 0, 1, 255 and 1024 float4 groups
@pytest.mark.parametrize("beta_1", [0.5, 0.9])
def test_adam_beta1_and_tails(dev, beta_1, n):
    from scrabble_gan_amd import ops
    gen = _gen()
    lr, b1, b2 = 2e-4, _f32s(beta_1), _f32s(0.999)
    p0 = _f32(rnd(gen, n))
    grads = [_f32(rnd(gen, n) * (1 + t)) for t in range(5)]
    P, st = {"w": p0.clone()}, {}
    pg, m, v = g32(p0, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    pd, md, vd = g32(p0, dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)      # lr_t read from device memory
    lr_ts = []
    for t, g in enumerate(grads, 1):
        O.adam_update(P, {"w": g}, st, lr, b1, b2)
        lr_ts.append(lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t))
        gg = g32(g, dev)
        ops.adam_update(pg, gg, m, v, lr_ts[-1], b1, b2)
        ops.adam_update(pd, gg, md, vd, torch.tensor([lr_ts[-1]], dtype=torch.float32, device=dev), b1, b2)
    close(pg, P["w"], tol=1e-6, name="adam p")
    close(m, st["m.w"], tol=1e-6, name="adam m")
    close(v, st["v.w"], tol=1e-6, name="adam v")
    rp, rm, rv = _adam_ref(p0, grads, lr_ts, b1, b2)                  # the oracle against the ten-line loop
    assert (rp - P["w"]).abs().max().item() < 1e-12 and (rm - st["m.w"]).abs().max().item() < 1e-12
    assert torch.equal(pd, pg) and torch.equal(md, m) and torch.equal(vd, v)


def test_adam_optimizer_class(dev):
    """optimizers.Adam(2e-4, 0.9, 0.999).apply_gradients over two variables, three steps; a None gradient is skipped."""
    from scrabble_gan_amd import optimizers
    gen = _gen()
    opt = optimizers.Adam(2e-4, 0.9, 0.999)
    p0 = [_f32(rnd(gen, 5)), _f32(rnd(gen, 64)), _f32(rnd(gen, 8))]
    grads = [[_f32(rnd(gen, k.numel()) * (1 + t)) for t in range(3)] for k in p0]
    var = [g32(k, dev) for k in p0]                                   # (kept alive: the slots are keyed by address)
    lr_ts = []
    for t in range(3):
        opt.apply_gradients([(g32(grads[0][t], dev), var[0]), (g32(grads[1][t], dev), var[1]), (None, var[2])])
        lr_ts.append(2e-4 * math.sqrt(1 - 0.999 ** (t + 1)) / (1 - 0.9 ** (t + 1)))        # lr_t is computed on the host, in double
    assert opt.iterations == 3
    for i in (0, 1):
        rp, rm, rv = _adam_ref(p0[i], grads[i], lr_ts, _f32s(0.9), _f32s(0.999))
        m, v = opt._slot(var[i])
        close(var[i], rp, tol=1e-6, name="Adam p%d" % i)
        close(m, rm, tol=1e-6, name="Adam m%d" % i)
        close(v, rv, tol=1e-6, name="Adam v%d" % i)
    assert torch.equal(var[2].cpu(), p0[2].float())
    assert (var[2].data_ptr(), 8) not in opt._slots or all(s.abs().max().item() == 0 for s in opt._slot(var[2]))


def test_adam_gradient_edge_values(dev):
    from scrabble_gan_amd import ops
    lr, b1, b2, eps = 2e-4, _f32s(0.9), _f32s(0.999), 1e-7
    gs = _f32(torch.tensor([1e6, -1e-3, 1e-12, 0.0] * 2, dtype=torch.float64))
    p0 = _f32(rnd(_gen(), 8))
    pg, m, v = g32(p0, dev), torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    lr_t = _f32s(lr * math.sqrt(1 - b2) / (1 - b1))
    ops.adam_update(pg, g32(gs, dev), m, v, lr_t, b1, b2, eps)
    zero = gs == 0
    assert torch.equal(pg.cpu()[zero], p0.float()[zero])              # zero gradient on zero slots: p bitwise unchanged
    assert (m.cpu()[zero] == 0).all() and (v.cpu()[zero] == 0).all()
    pz, mz, vz = torch.zeros(8, device=dev), torch.zeros(8, device=dev), torch.zeros(8, device=dev)
    ops.adam_update(pz, g32(gs, dev), mz, vz, lr_t, b1, b2, eps)      # from p = 0 the step itself is the result
    want = -lr_t * ((1 - b1) * gs) / (((1 - b2) * gs * gs).sqrt() + _f32s(eps))
    rel = ((pz.double().cpu() - want).abs() / want.abs().clamp_min(1e-300))[~zero].max().item()
    margins.record("adam first step, gradients 1e6 .. 1e-12 (elementwise relative)", rel, 2e-6)
    assert torch.isfinite(pz).all() and rel <= 2e-6, (pz, want)
    assert (pz.cpu()[zero] == 0).all()


@pytest.mark.parametrize("rho", [0.9, 0.5])
@pytest.mark.parametrize("n", [1, 3, 5, 1021])
def test_rmsprop_sizes_and_rho(dev, n, rho):
    from scrabble_gan_amd import ops
    gen = _gen()
    rho = _f32s(rho)
    p0, g = _f32(rnd(gen, n)), _f32(rnd(gen, n))
    P, st = {"w": p0.clone()}, {}
    pg, ms = g32(p0, dev), torch.zeros(n, device=dev)
    for t in (1, 2, 3):
        O.rmsprop_update(P, {"w": g * t}, st, 2e-4, rho)
        if rho == _f32s(0.9):
            ops.rmsprop_update(pg, g32(g * t, dev), ms, 2e-4)         # the default rho
        else:
            ops.rmsprop_update(pg, g32(g * t, dev), ms, 2e-4, rho)
    close(pg, P["w"], tol=1e-6, name="rmsprop p")
    close(ms, st["ms.w"], tol=1e-6, name="rmsprop ms")


# ------------------------------------------------------------------------------------------------ 4. loss head
def _loss_inputs(gen, B):
    v = [_f32(rnd(gen, B, 1) * 1.5) for _ in range(5)]
    r_f = _f32(torch.rand(B, 1, generator=gen, dtype=torch.float64) * 30 + 5)
    r_r = _f32(torch.rand(B, 1, generator=gen, dtype=torch.float64) * 30)
    return v, r_f, r_r


def _loss_ref(v, r_f, r_r, mode, balance):
    """-> (16 scalars, 7 per-sample upstream gradients) as test_ops_gpu.test_loss_head forms them."""
    B = v[0].shape[0]
    v = [t.clone().requires_grad_(True) for t in v]
    r_f = r_f.clone().requires_grad_(True)
    fn = O.hinge if mode == 0 else O.not_saturating
    d_loss, d_lr, d_lf, g_loss, s_loss, s_a, s_b = fn(*v)
    g_bal, r_bal, alpha, r_std, g_std = O.apply_gradient_balancing(r_f, g_loss)
    g_added = g_loss + r_f
    g_final = g_bal if balance else g_added
    ref = [r_f.mean(), r_r.mean(), r_bal.mean(), g_loss.mean(), g_added.mean(), g_bal.mean(), d_loss.mean(), d_lr.mean(),
           d_lf.mean(), g_final.mean(), torch.tensor(1.0, dtype=torch.float64), r_std, g_std, s_loss.mean(), s_a.mean(), s_b.mean()]
    gD = torch.autograd.grad(d_loss.sum(), [v[0], v[1]], retain_graph=True)
    gS = torch.autograd.grad(s_loss.sum(), [v[2], v[3]], retain_graph=True)
    gG = torch.autograd.grad(g_final.sum(), [v[1], v[3], r_f], retain_graph=True, allow_unused=True)
    refs = [gD[0], gD[1], gS[0], gS[1], gG[0], gG[1] if gG[1] is not None else torch.zeros(B, 1, dtype=torch.float64), gG[2]]
    return torch.stack([t.detach().reshape(()) for t in ref]), [r.reshape(-1) for r in refs]


def _loss_gpu(dev, v, r_f, r_r, mode, balance):
    from scrabble_gan_amd import ops
    dv = [g32(t.reshape(-1), dev) for t in v]
    rfg, rrg = g32(r_f.reshape(-1), dev), g32(r_r.reshape(-1), dev)
    sums = ops.loss_sums(*dv, rfg, rrg, mode)
    return ops.loss_grads(*dv, rfg, mode, balance, 1.0, sums)


def _check_shared(outs, refs, B, tol):
    # shared-sweep factors: u * w = d sum(d_loss)/d d_f (resp. s_loss/s_f), u * x = d sum(g_final)/d d_f (resp. s_f); |w|,|x| <= 1
    for sh, a, c, nm in ((outs[7], refs[1], refs[4], "D"), (outs[8], refs[3], refs[5], "S")):
        assert sh.shape == (3, B) and sh[1:].abs().max().item() <= 1.0 + 1e-6
        close(sh[0] * sh[1], a, tol=tol, name="shared w " + nm)
        close(sh[0] * sh[2], c, tol=tol, name="shared x " + nm)


def _loss_case(dev, B, mode, balance, transform=None):
    """The body of test_ops_gpu.test_loss_head at a free batch size, same bounds; `transform` edits the inputs in place."""
    v, r_f, r_r = _loss_inputs(_gen(), B)
    if transform is not None:
        transform(v)
    scal_ref, refs = _loss_ref(v, r_f, r_r, mode, balance)
    scalars, outs = _loss_gpu(dev, v, r_f, r_r, mode, balance)
    tol = 2e-4 if balance else 1e-5
    close(scalars, scal_ref, tol=1e-5, name="scalars")
    for i, (o, r) in enumerate(zip(outs, refs)):
        close(o, r, tol=tol, name="upstream%d" % i)
    _check_shared(outs, refs, B, tol)
    return v, outs, refs


@pytest.mark.parametrize("mode,balance", [(0, False), (0, True), (1, False), (1, True)])
@pytest.mark.parametrize("B", [2, 255, 256, 257, 1000])       # 1000: four passes of the sums loop, four blocks of the grads kernel
def test_loss_head_batch_sizes(dev, B, mode, balance):
    _loss_case(dev, B, mode, balance)


@pytest.mark.parametrize("mode", [0, 1])
def test_loss_head_single_sample(dev, mode):
    """B = 1, balance off.  Both standard deviations are 0, so the two BALANCED means (reported whether or not balancing is on)
    are 0/0 in the reference as well: NaN on both sides; every other scalar is held to 1e-5.  With balancing ON every output
    is 0/0 in the reference too -- out of scope."""
    v, r_f, r_r = _loss_inputs(_gen(), 1)
    scal_ref, refs = _loss_ref(v, r_f, r_r, mode, False)
    scalars, outs = _loss_gpu(dev, v, r_f, r_r, mode, False)
    nan = [2, 5]                                             # r_bal.mean(), g_bal.mean()
    keep = [i for i in range(16) if i not in nan + [11, 12]]
    assert torch.isnan(scal_ref[nan]).all() and torch.isnan(scalars[nan]).all()
    assert (scal_ref[[11, 12]] == 0).all() and (scalars[[11, 12]] == 0).all()
    close(scalars[keep], scal_ref[keep], tol=1e-5, name="scalars")
    for i, (o, r) in enumerate(zip(outs, refs)):
        close(o, r, tol=1e-5, name="upstream%d" % i)
    _check_shared(outs, refs, 1, 1e-5)


def _kink(v):
    v[0][0], v[1][1], v[2][2], v[3][3] = 1.0, -1.0, 1.0, -1.0     # d_r, d_f, s_my, s_f: each hinge argument exactly 0 once


@pytest.mark.parametrize("balance", [False, True])
def test_loss_head_hinge_on_the_kink(dev, balance):
    """relu'(0) = 0 (torch's convention, the kernel's strict `>`)."""
    from scrabble_gan_amd import ops
    B = 37
    v, outs, refs = _loss_case(dev, B, 0, balance, _kink)
    for k in range(4):
        assert refs[k][k].item() == 0.0 and outs[k][k].item() == 0.0
    for sh, a, c in ((outs[7], outs[1], outs[4]), (outs[8], outs[3], outs[5])):
        both = (a == 0) & (c == 0)
        assert (sh[0][both] == 1).all() and (sh[0] != 0).all()
    terms = ops.loss_terms(*[g32(t.reshape(-1), dev) for t in v], 0)
    close(terms, torch.stack([t.reshape(-1) for t in O.hinge(*v)]), tol=1e-5, name="loss_terms")
    assert terms[1, 0].item() == 0.0 and terms[2, 1].item() == 0.0 and terms[5, 2].item() == 0.0 and terms[6, 3].item() == 0.0


def test_loss_head_saturated_sigmoid(dev):
    """not_saturating at +-50 and +-100: sce(x, z) = max(x, 0) - x z + log1p(exp(-|x|)) never forms exp of a positive number; the
    kernel's sigmoid 1 / (1 + exp(-x)) goes through exp(100) = inf to exactly 0.  Losses: 1e-5 of max(1, |ref|) per element
    against the fp64 softplus form; gradients: 1e-5 absolute against sigmoid(x) or sigmoid(x) - 1."""
    from scrabble_gan_amd import ops
    vals = torch.tensor([50.0, -50.0, 100.0, -100.0], dtype=torch.float64)
    B = 16
    idx = torch.arange(B)
    v = [vals[(idx // k) % 4].reshape(B, 1).clone() for k in (1, 4, 1, 4, 2)]       # every pairing of d_r / d_f and of s_my / s_f
    v[2] = v[2].flip(0)
    gen = _gen()
    r_f = _f32(torch.rand(B, 1, generator=gen, dtype=torch.float64) * 30 + 5)
    r_r = _f32(torch.rand(B, 1, generator=gen, dtype=torch.float64) * 30)
    sp = torch.nn.functional.softplus
    d_r, d_f, s_my, s_f, s_r = [t.reshape(-1) for t in v]
    want = torch.stack([sp(-d_r) + sp(d_f), sp(-d_r), sp(d_f), sp(-d_f) + sp(-s_r), sp(-s_my) + sp(s_f), sp(-s_my), sp(s_f)])
    assert (want - torch.stack([t.reshape(-1) for t in O.not_saturating(*v)])).abs().max().item() < 1e-12
    terms = ops.loss_terms(*[g32(t.reshape(-1), dev) for t in v], 1)
    _within(terms, want, 1e-5 * want.abs().clamp_min(1.0), "loss_terms, saturated (1e-5 of max(1, |ref|))")
    scal_ref, refs = _loss_ref(v, r_f, r_r, 1, False)
    scalars, outs = _loss_gpu(dev, v, r_f, r_r, 1, False)
    close(scalars, scal_ref, tol=1e-5, name="scalars")
    sg = torch.sigmoid
    grads = [sg(d_r) - 1, sg(d_f), sg(s_my) - 1, sg(s_f), sg(d_f) - 1, torch.zeros(B, dtype=torch.float64), torch.ones(B, dtype=torch.float64)]
    for i, (o, r, a) in enumerate(zip(outs, grads, refs)):
        assert (r - a).abs().max().item() < 1e-12                     # the closed forms are the oracle's autograd
        _within(o, r, 1e-5, "upstream%d, saturated (1e-5 absolute)" % i)
    for sh, a, c in ((outs[7], outs[1], outs[4]), (outs[8], outs[3], outs[5])):
        assert torch.isfinite(sh).all() and sh[1:].abs().max().item() <= 1.0 + 1e-6
        both = (a == 0) & (c == 0)
        assert (sh[0][both] == 1).all()
        _within(sh[0] * sh[1], a, 1e-6, "shared w, saturated")
        _within(sh[0] * sh[2], c, 1e-6, "shared x, saturated")
    assert ((outs[3] == 0) & (outs[5] == 0)).any()                    # s_f = -100: both targets of the S sweep are exactly 0


# ------------------------------------------------------------------------------------------------ 5. attention
def _attn_case(dev, th, ph, g, d, check_lse=False):
    from scrabble_gan_amd import ops
    th, ph, g = th.clone().requires_grad_(True), ph.clone().requires_grad_(True), g.clone().requires_grad_(True)
    logits = th @ ph.transpose(1, 2)
    out = torch.softmax(logits, dim=-1) @ g
    out.backward(d)
    thg, phg, gg = g32(th.detach(), dev), g32(ph.detach(), dev), g32(g.detach(), dev)
    og, lse = ops.attention_fwd(thg, phg, gg)
    close(og, out, name="attn out")
    if check_lse:
        close(lse, torch.logsumexp(logits.detach(), -1), name="attn lse")
    dth, dph, dg = ops.attention_bwd(thg, phg, gg, og, lse, g32(d, dev))
    return (og, dth, dph, dg), (out.detach(), th.grad, ph.grad, g.grad)


@pytest.mark.parametrize("B,Nq,Nk", [(1, 1, 1), (2, 33, 1), (2, 1, 33), (3, 31, 2), (2, 65, 31)])
def test_attention_ragged_and_tiny(dev, B, Nq, Nk):
    gen = _gen()
    th, ph, g, d = _f32(rnd(gen, B, Nq, 8) * 1.5), _f32(rnd(gen, B, Nk, 8) * 1.5), _f32(rnd(gen, B, Nk, 32)), _f32(rnd(gen, B, Nq, 32))
    (og, dth, dph, dg), (out, rth, rph, rg) = _attn_case(dev, th, ph, g, d)
    close(dg, rg, tol=5e-5, name="dg")
    if Nk == 1:
        # one key: the softmax is 1, out = g broadcast over the queries and both logit gradients vanish (`close` has no scale)
        assert torch.equal(out, g.expand(B, Nq, 32))
        for nm, t in (("dtheta", dth), ("dphi", dph)):
            err = t.double().abs().max().item()
            margins.record(nm + " (Nk = 1: zero)", err / d.abs().max().item(), 5e-5)
            assert math.isfinite(err) and err <= 5e-5 * d.abs().max().item(), (nm, err)
    else:
        close(dth, rth, tol=5e-5, name="dtheta")
        close(dph, rph, tol=5e-5, name="dphi")


def _attn_large(dev, B, Nq, Nk):
    gen = _gen()
    th, ph = rnd(gen, B, Nq, 8) * 6, rnd(gen, B, Nk, 8) * 6
    th[0] += 10.0            # a common component in every query of sample 0: its logits move by 10 * sum(phi_k), another running max per key tile
    th, ph, g, d = _f32(th), _f32(ph), _f32(rnd(gen, B, Nk, 32)), _f32(rnd(gen, B, Nq, 32))
    assert (th @ ph.transpose(1, 2)).abs().max().item() > 200          # exp() of these overflows fp32 without the running maximum
    (og, dth, dph, dg), (out, rth, rph, rg) = _attn_case(dev, th, ph, g, d, check_lse=True)
    close(dth, rth, tol=5e-5, name="dtheta")
    close(dph, rph, tol=5e-5, name="dphi")
    close(dg, rg, tol=5e-5, name="dg")


@pytest.mark.parametrize("B,Nq,Nk", [(2, 128, 96), (3, 200, 300)])
def test_attention_large_logits(dev, B, Nq, Nk):
    _attn_large(dev, B, Nq, Nk)


def test_attention_large_logits_deterministic(dev):
    from scrabble_gan_amd import ops
    ops.set_deterministic(True)
    try:
        _attn_large(dev, 3, 200, 300)
    finally:
        ops.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ 6. pools and elementwise
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 1023])
def test_elementwise_small_odd_counts(dev, n):
    from scrabble_gan_amd import ops
    gen = _gen()
    a, b = _f32(rnd(gen, n)), _f32(rnd(gen, n))
    ag, bg = g32(a, dev), g32(b, dev)
    close(ops.add(ag, bg), a + b, name="add")                  # n < 4: scalar tail only; 1023 = 255 float4 groups + 3
    close(ops.relu_mask(ag, bg), a * (b > 0), name="relu_mask")
    t = _f32(torch.tanh(a))
    close(ops.tanh_bwd(g32(t, dev), bg), b * (1 - t * t), name="tanh_bwd")


@pytest.mark.parametrize("n", [4, 8])
def test_float4_only_sweeps_at_one_and_two_groups(dev, n):
    from scrabble_gan_amd import ops
    gen = _gen()
    a, b, sig, s = _f32(rnd(gen, n)), _f32(rnd(gen, n)), _f32(torch.tensor([0.37], dtype=torch.float64)), _f32(rnd(gen, 2))
    ag, bg = g32(a, dev), g32(b, dev)
    close(ops.scale(ag, g32(sig, dev)), sig * a, name="scale")
    close(ops.scale_add(ag, bg, g32(sig, dev)), sig * a + b, name="scale_add")
    acc = torch.full((1,), 0.5, device=dev)
    ops.dot_accum(ag, bg, acc)
    close(acc, 0.5 + (a * b).sum().reshape(1), tol=1e-4, name="dot")
    close(ops.rowscale(g32(a.view(2, n // 2), dev), g32(s, dev)), a.view(2, n // 2) * s.view(2, 1), name="rowscale")


def test_float4_only_sweeps_refuse_a_ragged_count(dev):
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import ScrabbleHipError
    a, b, s = torch.ones(6, device=dev), torch.ones(6, device=dev), torch.ones(1, device=dev)
    with pytest.raises(ScrabbleHipError, match="SG_ERR_ARG"):
        ops.scale(a, s)
    with pytest.raises(ScrabbleHipError, match="SG_ERR_ARG"):
        ops.scale_add(a, b, s)
    acc = torch.zeros(1, device=dev)
    with pytest.raises(ScrabbleHipError, match="SG_ERR_ARG"):
        ops.dot_accum(a, b, acc)
    assert acc.item() == 0.0


def test_relu_mask_signed_zeros(dev):
    from scrabble_gan_amd import ops
    ref = torch.tensor([0.0, -0.0, 1.0, -1.0, 0.0, -0.0, 1e-30, -1e-30], device=dev)
    dy = torch.tensor([3.0, 5.0, 7.0, 9.0, -3.0, -5.0, -7.0, -9.0], device=dev)
    out = ops.relu_mask(dy, ref).cpu()
    assert out.tolist() == [0.0, 0.0, 7.0, 0.0, 0.0, 0.0, -7.0, 0.0]


def _windows(t, ph, pw):
    """[B, H, W, C] -> [B, H/ph, W/pw, C, ph*pw], window positions in row-major order (the kernel's index iy * pw + ix)."""
    B, H, W, C = t.shape
    return t.reshape(B, H // ph, ph, W // pw, pw, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // ph, W // pw, C, ph * pw)


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 2, 4), (2, 4, 6, 4), (3, 6, 5, 8)])
def test_maxpool_small_shapes_and_accumulate(dev, B, H, W, C):
    from scrabble_gan_amd import ops
    gen = _gen()
    ph, pw = 2, 1
    for name, a in (("randn", _f32(rnd(gen, B, H, W, C))), ("all negative", _f32(-1 - torch.rand(B, H, W, C, generator=gen, dtype=torch.float64)))):
        ar = a.clone().requires_grad_(True)
        y = O.max_pool(ar, ph, pw)
        dy = _f32(rnd(gen, *y.shape))
        y.backward(dy)
        yg, idx = ops.maxpool_fwd(g32(a, dev), ph, pw)
        close(yg, y, name="maxpool, " + name)
        if name == "all negative":
            assert (yg < 0).all()                             # the running maximum starts at -inf, not at 0
        dyg = g32(dy, dev)
        plain = ops.maxpool_bwd(dyg, idx, ph, pw)
        close(plain, ar.grad, name="maxpool_bwd, " + name)
        pre = _f32(rnd(gen, B, H, W, C))
        acc = ops.maxpool_bwd(dyg, idx, ph, pw, out=g32(pre, dev), accum=True)
        close(acc, pre + ar.grad, tol=1e-6, name="maxpool_bwd accum, " + name)
        over = ops.maxpool_bwd(dyg, idx, ph, pw, out=torch.full((B, H, W, C), math.nan, device=dev), accum=False)
        assert torch.isfinite(over).all() and torch.equal(over, plain)


@pytest.mark.parametrize("ph,pw", [(2, 1), (2, 2)])
def test_maxpool_windows_of_equal_values(dev, ph, pw):
    """Post-ReLU input: many windows are all zero (the recognizer's usual input).  Each dy goes to exactly ONE element of its
    window.  On a tie the kernel keeps the FIRST maximum in row-major window order (strict `>` from -inf: position 0 of an
    all-equal window); wherever the maximum is unique the oracle's autograd must agree."""
    from scrabble_gan_amd import ops
    gen = _gen()
    B, H, W, C = 2, 8, 12, 64
    a = _f32(torch.relu(rnd(gen, B, H, W, C)))
    ar = a.clone().requires_grad_(True)
    y = O.max_pool(ar, ph, pw)
    dy = _f32(rnd(gen, *y.shape))
    y.backward(dy)
    wa = _windows(a, ph, pw)
    ties = (wa == wa.max(-1, keepdim=True).values).sum(-1) > 1
    assert 0.02 < ties.double().mean().item() < 0.5 and (wa.max(-1).values == 0).any()
    yg, idx = ops.maxpool_fwd(g32(a, dev), ph, pw)
    close(yg, y, name="maxpool")
    dx = ops.maxpool_bwd(g32(dy, dev), idx, ph, pw).double().cpu()
    wd = _windows(dx, ph, pw)
    assert (wd.ne(0).sum(-1) <= 1).all()                       # one receiver per window ...
    assert torch.equal(wd.sum(-1), dy)                         # ... that gets dy itself
    unique = (~ties).unsqueeze(-1).expand_as(wd)
    assert torch.equal(wd[unique], _windows(ar.grad, ph, pw)[unique])
    assert torch.equal(idx.cpu().long()[ties], wa.argmax(-1)[ties])      # (torch.argmax: the index of the first maximum)


@pytest.mark.parametrize("B,H,W,C", [(2, 1, 1, 4), (2, 1, 3, 4), (2, 1, 1, 1024), (2, 3, 1, 1024)])
def test_gap_without_relu(dev, B, H, W, C):
    from scrabble_gan_amd import ops
    gen = _gen()
    x = _f32(rnd(gen, B, H, W, C)).requires_grad_(True)
    y = x.mean(dim=(1, 2))
    dy = _f32(rnd(gen, B, C))
    y.backward(dy)
    xg = g32(x, dev)
    assert (x < 0).any()
    close(ops.gap_fwd(xg, relu=False), y, name="gap, no relu")
    close(ops.gap_bwd(g32(dy, dev), xg, relu=False), x.grad, name="gap_bwd, no relu")
    x2 = x.detach().clone().requires_grad_(True)                # the ReLU form at the same shapes
    y2 = torch.relu(x2).mean(dim=(1, 2))
    y2.backward(dy)
    close(ops.gap_fwd(xg), y2, name="gap")
    close(ops.gap_bwd(g32(dy, dev), xg), x2.grad, name="gap_bwd")


def test_avgpool_small_shapes(dev):
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import ScrabbleHipError
    gen = _gen()
    for B, H, W, C in ((1, 2, 2, 4), (2, 6, 10, 12)):            # the smallest shape; C/4 = 3
        a, b = _f32(rnd(gen, B, H, W, C)), _f32(rnd(gen, B, H, W, C))
        close(ops.avgpool2_add_fwd(g32(a, dev), g32(b, dev)), O.avg_pool2(a) + O.avg_pool2(b), name="avgpool_add")
        close(ops.avgpool2_add_fwd(g32(a, dev)), O.avg_pool2(a), name="avgpool")
        ar = a.clone().requires_grad_(True)
        d = _f32(rnd(gen, B, H // 2, W // 2, C))
        O.avg_pool2(ar).backward(d)
        close(ops.avgpool2_bwd(g32(d, dev)), ar.grad, name="avgpool_bwd")
    a1 = _f32(rnd(gen, 1, 2, 2, 1)).requires_grad_(True)
    d1 = _f32(rnd(gen, 1, 1, 1, 1))
    O.avg_pool2(a1).backward(d1)
    close(ops.avgpool2_bwd(g32(d1, dev)), a1.grad, name="avgpool_bwd_c1")
    with pytest.raises(ScrabbleHipError, match="SG_ERR_ARG"):
        ops.avgpool2_add_fwd(torch.zeros(1, 3, 2, 4, device=dev))


@pytest.mark.parametrize("M,N", [(1, 1), (1, 53), (7, 3), (33, 4), (1000, 5)])
def test_bias_grad_small_shapes(dev, M, N):
    from scrabble_gan_amd import ops
    gen = _gen()
    dyb, db0 = _f32(rnd(gen, M, N)), _f32(rnd(gen, N))
    db = g32(db0, dev)                                          # db accumulates
    ops.bias_grad(g32(dyb, dev), db)
    close(db, db0 + dyb.sum(0), tol=5e-5, name="bias_grad %dx%d" % (M, N))


def test_bias_add_narrowest(dev):
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import ScrabbleHipError
    gen = _gen()
    y, b = _f32(rnd(gen, 1, 4)), _f32(rnd(gen, 4))
    close(ops.bias_add(g32(y, dev), g32(b, dev)), y + b, name="bias_add")
    with pytest.raises(ScrabbleHipError, match="SG_ERR_ARG"):
        ops.bias_add(torch.zeros(3, 2, device=dev), torch.zeros(2, device=dev))
