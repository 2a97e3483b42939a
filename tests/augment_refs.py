"""fp64 torch reference of the augmentation kernels (csrc/augment.hip; definition in include/scrabble_hip.h), shared by
tests/test_augment_cpu.py, tests/test_augment_gpu.py and tests/test_augment_step_gpu.py.  Written with differentiable gathers,
so autograd yields the reference dx.  Nothing here touches the code under test."""
import numpy as np
import torch

IDENTITY = [1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0]


def row(c=1.0, beta=0.0, m=(1, 0, 0, 0, 1, 0), cut=(0, 0, 0, 0)):
    return [c, beta] + list(m) + list(cut)


def augment_ref(x, params, pad=0.0):
    """x [B,H,W,C] (any float dtype, may require grad), params [B,12] -> y in x's dtype.  Coordinates and weights are formed in
    fp64 from the fp32 parameter values; the pixel arithmetic runs in x's dtype (fp64 for the reference, fp32 for the yardstick of
    the step test)."""
    B, H, W, C = x.shape
    p = torch.as_tensor(np.asarray(params, np.float32)).double()
    ii = torch.arange(H, dtype=torch.float64).view(H, 1)
    jj = torch.arange(W, dtype=torch.float64).view(1, W)
    padv = torch.tensor(pad, dtype=x.dtype)
    outs = []
    for b in range(B):
        c, beta, a00, a01, a02, a10, a11, a12, x0, y0, x1, y1 = p[b].tolist()
        t = c * x[b] + (1.0 - c) * x[b].mean() + beta
        flat = t.reshape(H * W, C)
        sx, sy = a00 * jj + a01 * ii + a02, a10 * jj + a11 * ii + a12
        fx, fy = torch.floor(sx), torch.floor(sy)
        acc = torch.zeros(H, W, C, dtype=x.dtype)
        for oy, wy in ((0, 1.0 - (sy - fy)), (1, sy - fy)):
            for ox, wx in ((0, 1.0 - (sx - fx)), (1, sx - fx)):
                tx, ty = fx + ox, fy + oy
                inside = (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
                idx = (ty.clamp(0, H - 1) * W + tx.clamp(0, W - 1)).long().reshape(-1)
                v = torch.where(inside.unsqueeze(-1), flat[idx].reshape(H, W, C), padv)
                acc = acc + (wx * wy).to(x.dtype).unsqueeze(-1) * v
        cut = (jj >= x0) & (jj < x1) & (ii >= y0) & (ii < y1)
        outs.append(torch.where(cut.unsqueeze(-1), padv, acc))
    return torch.stack(outs, 0)


def augment_ref_with_grad(x, params, dy, pad=0.0):
    """-> (y, dx) in fp64: dx = d <augment(x), dy> / dx by autograd."""
    x64 = x.detach().double().clone().requires_grad_(True)
    y = augment_ref(x64, params, pad)
    (dx,) = torch.autograd.grad((y * dy.double()).sum(), x64)
    return y.detach(), dx


def exact_coordinates(r) -> bool:
    """A pure integer translation: its sample points are exact in fp32."""
    r = np.asarray(r, np.float64)
    return bool(r[2] == 1 and r[3] == 0 and r[5] == 0 and r[6] == 1 and r[4] == round(r[4]) and r[7] == round(r[7]))


def coordinate_eps(r, H, W) -> float:
    """fp32 rounding of a sample point: 2^-22 (|a00| W + |a01| H + |a02|) for sx, likewise for sy (three operations of relative
    error 2^-24 each on terms of at most that size); the larger of the two.  0 for exact coordinates."""
    if exact_coordinates(r):
        return 0.0
    r = np.abs(np.asarray(r, np.float64))
    return float(2.0 ** -22 * max(r[2] * W + r[3] * H + r[4], r[5] * W + r[6] * H + r[7]))


def bounds(x, params, dy, y_ref, dx_ref, pad=0.0):
    """Per-sample absolute bounds (by, bdx) for max|y - y_ref| and max|dx - dx_ref|: the fp32 max-norm bound 2e-5 max(1, max|ref|)
    plus the coordinate term -- a sample point off by eps moves y by at most eps times the spread of the tap values (the slope of
    the bilinear interpolant) per axis, and a tap weight by at most eps per axis, i.e. dx by 2 eps |c| max|dy| per axis."""
    B, H, W, C = x.shape
    p = np.asarray(params, np.float64)
    by, bdx = [], []
    for b in range(B):
        eps = coordinate_eps(p[b], H, W)
        c, beta = p[b, 0], p[b, 1]
        t = c * x[b].double() + (1 - c) * x[b].double().mean() + beta
        spread = max(t.max().item(), pad) - min(t.min().item(), pad)
        by.append(2e-5 * max(1.0, y_ref[b].abs().max().item()) + 2 * eps * spread)
        bdx.append(2e-5 * max(1.0, dx_ref[b].abs().max().item()) + 2 * eps * 2 * abs(c) * dy[b].abs().max().item())
    return by, bdx
