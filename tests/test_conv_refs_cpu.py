"""tests/conv_refs.py without a GPU: the flag composition of the references matches autograd through the oracle for mask / accum /
sample_scale at two tiny shapes, the generated ReLU masks of tests/test_conv_flags_gpu.py hold what the module promises for every seed it
uses, and the case tables cover what they claim."""
import math

import pytest
import torch

from oracle import scrabble_oracle as O
from tests import conv_refs as R

TINY = [(2, 3, 5, 4, 6, 3, True), (3, 4, 4, 8, 4, 2, False)]       # B, H, W, Cin, Cout, k, same


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= tol * (b.abs().max().item() + 1e-30)


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,same", TINY)
def test_flag_composition_matches_autograd(B, H, W, Cin, Cout, k, same):
    g = torch.Generator().manual_seed(B * 100 + k)
    pad = "same" if same else "valid"
    x, w = R.rnd(g, B, H, W, Cin), R.rnd(g, k, k, Cin, Cout) / math.sqrt(k * k * Cin)
    b1, b2 = R.rnd(g, Cout), R.rnd(g, Cout)
    # forward: relu_in, both biases, accumulate, ReLU after the accumulate
    y0 = O.conv2d(torch.relu(x), w, b1 + b2, padding=pad)
    prev = R.make_prev(g, y0.shape, y0.abs().max().item(), True)
    term, y = R.fwd(x, w, b1, b2, relu_in=True, relu_out=True, prev=prev, same=same)
    _close(term, y0)
    _close(y, torch.relu(y0 + prev))
    assert abs(prev.abs().max().item() / y0.abs().max().item() - 100.0) < 1e-3
    # data-grad of L = <conv(relu(m), w), dy>: autograd's ReLU backward is the mask rule (zero where m <= 0), then + prev
    dy = R.rnd(g, *y0.shape)
    m = R.make_mask(g, B, H, W, Cin).double().requires_grad_(True)
    O.conv2d(torch.relu(m), w, None, padding=pad).backward(dy)
    prevx = R.make_prev(g, x.shape, 1.0, False)
    term, keep, dx = R.dgrad(dy, w, (H, W), mask=m.detach(), prev=prevx, same=same)
    _close(dx, m.grad + prevx)
    assert torch.equal(dx[~keep], prevx[~keep])                      # masked elements: exactly the accumulate operand
    assert torch.equal(R.dgrad(dy, w, (H, W), mask=m.detach(), same=same)[2][~keep], torch.zeros(int((~keep).sum())).double())
    # weight-grad with per-sample factors: d/dw of sum_b s_b <conv(relu(x_b), w), dy_b>
    sc = R.f32(torch.rand(B, generator=g, dtype=torch.float64) * 2 - 0.5)
    wr, br = w.clone().requires_grad_(True), b1.clone().requires_grad_(True)
    (O.conv2d(torch.relu(x), wr, br, padding=pad) * dy * sc.view(B, 1, 1, 1)).sum().backward()
    dw, db = R.wgrad(x, dy, w.shape, relu_in=True, sample_scale=sc, same=same)
    _close(dw, wr.grad, 1e-6)        # (the reference rounds s_b * dy to fp32 once, as the kernels do)
    _close(db, br.grad, 1e-6)


@pytest.mark.parametrize("stride", [(2, 2), (2, 1), (1, 2)])
@pytest.mark.parametrize("k", [3, 1])
def test_transposed_composition_matches_autograd(stride, k):
    g = torch.Generator().manual_seed(17 + k)
    B, H, W, Cin, Cout = 2, 3, 4, 4, 6
    x = R.rnd(g, B, H, W, Cin).requires_grad_(True)
    w = (R.rnd(g, k, k, Cout, Cin) / math.sqrt(k * k * Cin)).requires_grad_(True)
    b1, b2 = R.rnd(g, Cout), R.rnd(g, Cout)
    y0 = O.conv2d_transpose(x, w, b1 + b2, stride)
    dy = R.rnd(g, *y0.shape)
    y0.backward(dy)
    prev = R.make_prev(g, y0.shape, 1.0, False)
    term, y = R.t_fwd(x.detach(), w.detach(), b1, b2, stride, prev)
    _close(term, y0.detach())
    _close(y, y0.detach() + prev)
    mask = R.make_mask(g, B, H, W, Cin).double()
    term, keep, dx = R.t_dgrad(dy, w.detach(), stride, mask)
    _close(term, x.grad)
    _close(dx, x.grad * (mask > 0))
    _close(R.t_wgrad(x.detach(), dy, w.shape, stride), w.grad)


def test_operand_roundings():
    g = torch.Generator().manual_seed(1)
    t = R.rnd(g, 64, 8)
    assert torch.equal(R.r16(t), t.to(torch.bfloat16).double())
    q = R.q8(t)
    assert abs(q.abs().max().item() / t.abs().max().item() - 1.0) < 1e-6      # the amax element maps to 448, an e4m3 value (the scale is fp32)
    assert (q - t).abs().max().item() <= 2.0 ** -4 * t.abs().max().item()
    assert (R.q8(t, relu=True) >= 0).all()
    assert (R.q5(t) - t).abs().max().item() <= 2.0 ** -3 * t.abs().max().item()


def test_masks_of_the_gpu_module_for_every_seed():
    from tests import test_conv_flags_gpu as T
    specs = T.mask_specs()
    assert len(specs) > 50
    for seed, shape in specs:
        R.check_mask(R.make_mask(torch.Generator().manual_seed(seed), *shape))


def test_tables_cover_what_the_module_promises():
    """Per route: every flag row at a straddling and an exact-multiple M, every M of its list with bias + bias2 + accum and
    mask + accum, every split state with both rows (direct families); the accumulate operand is 100 x the conv term on about half
    of the accumulate cases."""
    from tests import test_conv_flags_gpu as T
    for r, cfg in T.ROUTES.items():
        cs = [c for c in T.CASES if c[0] == r]
        for kind, rows in (("fwd", T.FWD_FLAGS), ("dgrad", T.DGRAD_FLAGS)):
            for f in rows:
                ms = {math.prod(c[2]) % 256 == 0 for c in cs if c[1] == kind and c[6] == f}
                assert ms == {True, False}, (r, kind, f)
        for kind, f in (("fwd", "bias+bias2+accum"), ("dgrad", "mask+accum")):
            assert {c[2] for c in cs if c[1] == kind and c[6] == f} >= set(cfg["shapes"]), (r, kind)
            if not r.startswith("wino"):
                assert {c[7] for c in cs if c[1] == kind and c[6] == f} == set(T.SPLITS), (r, kind)
        acc = [c[8] for c in cs if "accum" in c[6]]
        assert 0.35 <= sum(acc) / len(acc) <= 0.65, (r, sum(acc), len(acc))
    assert len({T._id(c) for c in T.CASES}) == len(T.CASES)
