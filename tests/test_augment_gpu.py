"""ops.augment / ops.augment_bwd (csrc/augment.hip) against the fp64 reference of tests/augment_refs.py.

Bounds (per sample, computed in augment_refs.bounds, nothing tuned on the kernels): the project's fp32 max-norm bound
2e-5 max(1, max|ref|); rows that are not pure integer translations add the coordinate term 2 eps (spread of the tap values) for y
and 2 eps 2 |c| max|dy| for dx with eps = 2^-22 (|a00| W + |a01| H + |a02|) (likewise sy).  Identity and integer translations
with c = 1, beta = 0 are bit-exact."""
import ctypes

import numpy as np
import pytest
import torch

from tests import augment_refs as AR
from tests import margins

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1, 1), (2, 3, 5, 1), (3, 32, 32, 1), (4, 7, 67, 3), (2, 32, 368, 1),
          (1, 33, 500, 1)]        # (the last: 16 500 floats, past what a workgroup stages in LDS -- the two-pass path)
PAD = 0.375
N_FIXED = 14


def _rows(H, W):
    """The rows of one shape: fixed cases (index: see EXACT / TRANSLATIONS below) + eight from the sampler, all four families."""
    from scrabble_gan_amd.augment import DiffAugment
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    about = lambda a00, a01, a11, tx=0.0, ty=0.0: (a00, a01, cx - a00 * cx - a01 * cy + tx, 0, a11, cy - a11 * cy + ty)
    fixed = [
        AR.row(),                                                           # 0 identity
        AR.row(c=1.3, beta=-0.2),                                           # 1 colour only
        AR.row(c=0.5, beta=0.5),                                            # 2 colour at its limits
        AR.row(m=(1, 0, 2, 0, 1, -1)),                                      # 3 integer translation
        AR.row(m=(1, 0, -1, 0, 1, 1)),                                      # 4 the other way
        AR.row(m=(1, 0, W, 0, 1, 0)),                                       # 5 a shift of the whole width: all pad
        AR.row(m=(1, 0, 0, 0, 1, -(H + 3))),                                # 6 ... and beyond the height
        AR.row(m=(1, 0, 0.5, 0, 1, -0.5)),                                  # 7 half-pixel translation
        AR.row(c=0.8, beta=0.1, m=(1, 0, -0.25, 0, 1, 0.75)),               # 8 quarter-pixel with colour
        AR.row(c=1.2, cut=(0, 0, W, H)),                                    # 9 cutout: everything
        AR.row(c=1.2, cut=(max(W - max(W // 4, 1), 0), 0, W, max(H // 2, 1))),      # 10 cutout clipped at the right / top border
        AR.row(m=(1, 0, 1, 0, 1, 0), cut=(0, H // 2, max(W // 2, 1), H)),   # 11 cutout at the left / bottom border, translated
        AR.row(m=about(1.1, -0.3, 0.9)),                                    # 12 shear + scale at the limits of the search window
        AR.row(c=0.7, beta=-0.3, m=about(0.9, 0.3, 1.1, tx=3, ty=-2), cut=(1, 0, 2, 1)),   # 13 the opposite limits, with everything else
    ]
    assert len(fixed) == N_FIXED
    drawn = DiffAugment("color,translation,cutout,affine", seed=1234 + H * 1000 + W).sample(8, H, W)
    p = np.concatenate([np.asarray(fixed, np.float32), drawn], 0)
    DiffAugment.check(p)                                                    # valid rows only reach the kernels
    return p


EXACT_Y = {0: (0, 0), 3: (2, -1), 4: (-1, 1), 5: None, 6: None}      # row -> (tx, ty) of a bit-exact shift (None: all pad)

_CASES = {}


def _case(shape):
    """x, dy, the rows and the fp64 reference (y, dx) of one shape -- computed once, shared, never modified."""
    if shape not in _CASES:
        B, H, W, C = shape
        rows = _rows(H, W)
        n = len(rows)
        g = torch.Generator().manual_seed(sum(shape))
        x1 = torch.rand(B, H, W, C, generator=g) * 2 - 1
        d1 = torch.randn(B, H, W, C, generator=g)
        reps = (n + B - 1) // B
        # launch k carries rows k*B .. k*B+B-1 (identity behind the last row); sample s of every launch is image s
        table = np.tile(np.asarray(AR.IDENTITY, np.float32), (reps * B, 1))
        table[:n] = rows
        x, dy = x1.repeat(reps, 1, 1, 1), d1.repeat(reps, 1, 1, 1)
        y_ref, dx_ref = AR.augment_ref_with_grad(x, table, dy, PAD)
        by, bdx = AR.bounds(x, table, dy, y_ref, dx_ref, PAD)
        _CASES[shape] = dict(x=x, dy=dy, table=table, n=n, reps=reps, y_ref=y_ref, dx_ref=dx_ref, by=by, bdx=bdx)
    return _CASES[shape]


def _run(dev, shape, case, pad=PAD):
    """Every launch of the shape (batch B each) -> (y, dx, mean) on the host, rows in table order."""
    from scrabble_gan_amd import ops
    B = shape[0]
    ys, dxs, means = [], [], []
    for k in range(case["reps"]):
        sl = slice(k * B, (k + 1) * B)
        p = torch.from_numpy(case["table"][sl]).to(dev)
        y, ctx = ops.augment(case["x"][sl].to(dev).contiguous(), p, pad)
        dx = ops.augment_bwd(case["dy"][sl].to(dev).contiguous(), ctx)
        ys.append(y.cpu()), dxs.append(dx.cpu()), means.append(ctx[2].cpu())
    return torch.cat(ys), torch.cat(dxs), torch.cat(means)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_augment_forward_and_backward_against_the_reference(dev, shape):
    B, H, W, C = shape
    case = _case(shape)
    y, dx, mean = _run(dev, shape, case)
    x, dy, n = case["x"], case["dy"], case["n"]
    mu = x.double().mean(dim=(1, 2, 3))
    assert ((mean.double() - mu).abs() <= 1e-6 * mu.abs() + 1e-7).all(), "mean_out"
    bad = []
    for r in range(len(case["table"])):
        ey = (y[r].double() - case["y_ref"][r]).abs().max().item()
        ed = (dx[r].double() - case["dx_ref"][r]).abs().max().item()
        print("row %2d  y %.3e / %.3e   dx %.3e / %.3e" % (r, ey, case["by"][r], ed, case["bdx"][r]))
        margins.record("augment y row %d" % r, ey / (case["by"][r] / 2e-5), 2e-5)
        margins.record("augment dx row %d" % r, ed / (case["bdx"][r] / 2e-5), 2e-5)
        if not ey <= case["by"][r]:
            bad.append("row %d %s: y off by %.3e > %.3e" % (r, case["table"][r].tolist(), ey, case["by"][r]))
        if not ed <= case["bdx"][r]:
            bad.append("row %d %s: dx off by %.3e > %.3e" % (r, case["table"][r].tolist(), ed, case["bdx"][r]))
    assert not bad, "\n".join(bad)
    # ---- bit-exact cases
    idn = [0] + list(range(n, len(case["table"])))                        # the identity row and the identity rows behind the last one
    for r in idn:
        assert torch.equal(y[r], x[r]) and torch.equal(dx[r], dy[r]), "identity row %d" % r
    for r, shift in EXACT_Y.items():
        want = torch.full((H, W, C), PAD)
        if shift is not None:
            tx, ty = shift                                                  # y[i, j] = x[i + ty, j + tx]
            i0, i1, j0, j1 = max(0, -ty), min(H, H - ty), max(0, -tx), min(W, W - tx)
            if i1 > i0 and j1 > j0:
                want[i0:i1, j0:j1] = x[r, i0 + ty:i1 + ty, j0 + tx:j1 + tx]
        assert torch.equal(y[r], want), "integer translation row %d is not the shifted image bit for bit" % r


@pytest.mark.parametrize("shape", [(4, 7, 67, 3), (2, 32, 368, 1)], ids=lambda s: "x".join(map(str, s)))
def test_adjoint_identity_of_the_linear_part(dev, shape):
    """<augment(x), dy> == <x, augment_bwd(dy)> with c = 1, beta = 0, pad = 0 (the map is then linear), for every row's geometry."""
    B, H, W, C = shape
    base = _case(shape)
    table = base["table"].copy()
    table[:, 0], table[:, 1] = 1.0, 0.0
    x, dy = base["x"], base["dy"]
    y_ref, dx_ref = AR.augment_ref_with_grad(x, table, dy, 0.0)
    by, bdx = AR.bounds(x, table, dy, y_ref, dx_ref, 0.0)
    y, dx, _ = _run(dev, shape, dict(base, table=table), pad=0.0)
    for r in range(len(table)):
        lhs, rhs = (y[r].double() * dy[r].double()).sum().item(), (x[r].double() * dx[r].double()).sum().item()
        # each element of y / dx is within its bound of the reference, for which the identity holds exactly
        slack = by[r] * dy[r].double().abs().sum().item() + bdx[r] * x[r].double().abs().sum().item()
        assert abs(lhs - rhs) <= slack, "row %d: <Ax, dy> = %.9e, <x, A'dy> = %.9e, allowed %.3e" % (r, lhs, rhs, slack)


def test_backward_is_bitwise_reproducible(dev):
    shape = (2, 32, 368, 1)
    case = _case(shape)
    _, dx_a, _ = _run(dev, shape, case)
    _, dx_b, _ = _run(dev, shape, case)
    assert torch.equal(dx_a, dx_b)


def test_more_samples_than_workgroups(dev):
    """B beyond the grid cap of the memory-bound kernels: workgroups loop over samples.  Colour rows have a closed form."""
    from scrabble_gan_amd import ops
    B, H, W, C = 4100, 1, 2, 1
    g = torch.Generator().manual_seed(5)
    x, dy = torch.rand(B, H, W, C, generator=g) * 2 - 1, torch.randn(B, H, W, C, generator=g)
    table = np.tile(np.asarray(AR.IDENTITY, np.float32), (B, 1))
    table[:, 0] = np.linspace(0.5, 1.5, B, dtype=np.float32)
    table[:, 1] = np.linspace(-0.5, 0.5, B, dtype=np.float32)
    c, beta = (torch.from_numpy(table[:, k]).double().view(B, 1, 1, 1) for k in (0, 1))
    y_ref = c * x.double() + (1 - c) * x.double().mean(dim=(1, 2, 3), keepdim=True) + beta
    dx_ref = c * dy.double() + (1 - c) * dy.double().mean(dim=(1, 2, 3), keepdim=True)
    y, ctx = ops.augment(x.to(dev), torch.from_numpy(table).to(dev))
    dx = ops.augment_bwd(dy.to(dev), ctx)
    assert (y.cpu().double() - y_ref).abs().max().item() <= 2e-5 * max(1.0, y_ref.abs().max().item())
    assert (dx.cpu().double() - dx_ref).abs().max().item() <= 2e-5 * max(1.0, dx_ref.abs().max().item())


def test_kernels_stay_inside_their_output_buffers(dev):
    """y and dx live in the middle of wider, sentinel-filled buffers: every sentinel survives (valid rows only)."""
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import call
    shape = (4, 7, 67, 3)
    B, H, W, C = shape
    case = _case(shape)
    n, guard, sentinel = B * H * W * C, 4096, -12345.5
    for k in range(case["reps"]):
        sl = slice(k * B, (k + 1) * B)
        p = torch.from_numpy(case["table"][sl]).to(dev)
        x, dy = case["x"][sl].to(dev).contiguous(), case["dy"][sl].to(dev).contiguous()
        ybuf = torch.full((n + 2 * guard,), sentinel, device=dev)
        dbuf = torch.full((n + 2 * guard,), sentinel, device=dev)
        mbuf = torch.full((B + 2 * 64,), sentinel, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        call("sg_augment_fwd", x.data_ptr(), p.data_ptr(), ybuf[guard:].data_ptr(), mbuf[64:].data_ptr(), B, H, W, C, PAD, st)
        call("sg_augment_bwd", dy.data_ptr(), p.data_ptr(), dbuf[guard:].data_ptr(), B, H, W, C, st)
        for buf, g, m in ((ybuf, guard, n), (dbuf, guard, n), (mbuf, 64, B)):
            assert (buf[:g] == sentinel).all() and (buf[g + m:] == sentinel).all()
            assert (buf[g:g + m] != sentinel).all()
        y, ctx = ops.augment(x, p, PAD)
        assert torch.equal(ybuf[guard:guard + n].view(shape), y) and torch.equal(dbuf[guard:guard + n].view(shape), ops.augment_bwd(dy, ctx))


def test_argument_errors(dev):
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import lib
    L = lib()
    x = torch.zeros(2, 3, 5, 1, device=dev)
    y, p, m = torch.empty_like(x), torch.from_numpy(np.asarray([AR.IDENTITY] * 2, np.float32)).to(dev), torch.empty(2, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    f = ctypes.c_float(0.0)
    ERR_ARG = -1
    assert L.sg_augment_fwd(x.data_ptr(), p.data_ptr(), y.data_ptr(), m.data_ptr(), 2, 3, 5, 1, f, st) == 0
    assert L.sg_augment_fwd(x.data_ptr(), p.data_ptr(), y.data_ptr(), m.data_ptr(), 2, 0, 5, 1, f, st) == ERR_ARG
    for B_, W_, C_ in ((0, 5, 1), (2, 0, 1), (2, 5, 0), (-1, 5, 1)):
        assert L.sg_augment_fwd(x.data_ptr(), p.data_ptr(), y.data_ptr(), m.data_ptr(), B_, 3, W_, C_, f, st) == ERR_ARG
        assert L.sg_augment_bwd(x.data_ptr(), p.data_ptr(), y.data_ptr(), B_, 3, W_, C_, st) == ERR_ARG
    assert L.sg_augment_fwd(None, p.data_ptr(), y.data_ptr(), m.data_ptr(), 2, 3, 5, 1, f, st) == ERR_ARG
    assert L.sg_augment_fwd(x.data_ptr(), None, y.data_ptr(), m.data_ptr(), 2, 3, 5, 1, f, st) == ERR_ARG
    assert L.sg_augment_fwd(x.data_ptr(), p.data_ptr(), None, m.data_ptr(), 2, 3, 5, 1, f, st) == ERR_ARG
    assert L.sg_augment_fwd(x.data_ptr(), p.data_ptr(), y.data_ptr(), None, 2, 3, 5, 1, f, st) == ERR_ARG
    assert L.sg_augment_fwd(x.data_ptr(), p.data_ptr(), x.data_ptr(), m.data_ptr(), 2, 3, 5, 1, f, st) == ERR_ARG      # in place
    assert L.sg_augment_bwd(None, p.data_ptr(), y.data_ptr(), 2, 3, 5, 1, st) == ERR_ARG
    assert L.sg_augment_bwd(x.data_ptr(), p.data_ptr(), None, 2, 3, 5, 1, st) == ERR_ARG
    assert L.sg_augment_fwd(x.data_ptr(), p.data_ptr(), y.data_ptr(), m.data_ptr(), 2, 1 << 16, 1 << 16, 1, f, st) == ERR_ARG   # past 32-bit indexing
    torch.cuda.synchronize()
    # the wrappers
    with pytest.raises(ValueError):
        ops.augment(x, p[:1].contiguous())
    with pytest.raises(ValueError):
        ops.augment(x, torch.zeros(2, 11, device=dev))
    with pytest.raises(ValueError):
        ops.augment(x.view(2, 15), p)
    _, ctx = ops.augment(x, p)
    with pytest.raises(ValueError):
        ops.augment_bwd(torch.zeros(2, 5, 3, 1, device=dev), ctx)
