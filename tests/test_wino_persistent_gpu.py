"""The persistent tile loop of the grouped fp32 Winograd-domain products (sg_wino_persist_kernel in scrabble_gan_amd/csrc/conv_bf16v2.hip)
against the one-tile-per-workgroup kernel it replaces and against the fp64 oracle convolution.

The persistent kernel runs the same MFMAs in the same order on the same operands per tile, so its results must be BITWISE those of
`SG_WINO_PERSIST=0` (sg_debug_set_wino_persist(0, 0)); against the oracle both are held to the 2e-5 of max |ref| of tests/test_winograd_gpu.py.
Shapes: 16 tiles (one 128-row block per frequency plane), 144 tiles (Tp = 256: pad rows), an even shape that is no multiple of 4 for
F(2x2, 3x3); K = 32 / 64 / 96 (one, two, three k-tiles: both phantom parities; below the reduction-split threshold, so every tile is a
full tile); N = 64 (the 128 x 64 tiles, which stay on the one-tile kernel) / 128 / 256; grid caps 1, 5, 8 (several tiles per workgroup,
uneven last rounds, consecutive tiles in different frequency planes); four and eight waves per tile.

What "untouched" means here: the product writes all P * Tp rows of Mt (pad rows included, both kernels: they are never read back), so the
sentinels sit where nothing may be written -- the pad rows of V, the operands, and the memory behind the last row of Mt / of the workspace."""
import math

import pytest
import torch

from oracle import scrabble_oracle as O  # checker only

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 16, 4), (9, 8, 16, 4), (3, 6, 10, 2)]          # B, H, W, tile
KS, NS, CAPS = (32, 64, 96), (64, 128, 256), (1, 5, 8)
SENTINEL = 3.0
GUARD = 4096                                                      # floats behind a buffer's last row


@pytest.fixture(params=[0, 2], ids=["waves4", "waves8"])
def waves(request):
    """SG2_W8 = 0: four waves per 128 x 128 tile, 2: eight."""
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import lib
    old = ops.WINO_ROW_GAIN
    ops.WINO_ROW_GAIN = 0.0
    lib().sg_debug_set_w8(request.param)
    yield request.param
    lib().sg_debug_set_w8(1)
    lib().sg_debug_set_wino_persist(1, 0)
    ops.WINO_ROW_GAIN = old


def _geom(B, H, W, tile):
    P = (tile + 2) ** 2
    T = B * (H // tile) * (W // tile)
    return P, T, -(-T // 128) * 128


_REF = {}


def _case(dev, B, H, W, K, N):
    """inputs and fp64 oracle results of one (shape, K, N), computed once: forward K -> N and data-grad of an N -> K ... K -> N pair"""
    key = (B, H, W, K, N)
    if key not in _REF:
        g = torch.Generator(device=dev).manual_seed(B * 1000 + H * W + 7 * K + N)
        x = torch.randn(B, H, W, K, device=dev, generator=g)
        w = torch.randn(3, 3, K, N, device=dev, generator=g) / math.sqrt(9 * K)
        wb = torch.randn(3, 3, N, K, device=dev, generator=g) / math.sqrt(9 * K)       # data-grad: reduction over Cout = K, result Cin = N
        y_ref = O.conv2d(x.double().cpu(), w.double().cpu(), None)
        xr = torch.zeros(B, H, W, N, dtype=torch.float64, requires_grad=True)
        O.conv2d(xr, wb.double().cpu(), None).backward(x.double().cpu())
        _REF[key] = (x, w, wb, y_ref, xr.grad.detach())
    return _REF[key]


def _within(got, ref, name):
    err, scale = (got.double().cpu() - ref).abs().max().item(), ref.abs().max().item() + 1e-30
    print("%s: rel err %.3e" % (name, err / scale))
    assert err <= 2e-5 * scale, "%s: rel err %.3e > 2e-5" % (name, err / scale)


@pytest.mark.parametrize("B,H,W,tile", SHAPES)
def test_grouped_product_bitwise_and_sentinels(dev, waves, B, H, W, tile):
    """sg_wino_gemm: persistent == one-tile kernel bit for bit for every K, N and grid cap; V (pad rows included), u and the memory behind
    Mt's last row keep their contents."""
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import lib
    L = lib()
    P, T, Tp = _geom(B, H, W, tile)
    s = ops._stream()
    for K in KS:
        for N in NS:
            g = torch.Generator(device=dev).manual_seed(K + N + T)
            V = torch.randn(P, Tp, K, device=dev, generator=g)
            V[:, T:] = SENTINEL
            u = torch.randn(P, N, K, device=dev, generator=g)
            V0, u0 = V.clone(), u.clone()

            def run(mode, cap):
                Mt = torch.full((P * Tp * N + GUARD,), SENTINEL, device=dev)
                L.sg_debug_set_wino_persist(mode, cap)
                assert L.sg_wino_gemm(V.data_ptr(), u.data_ptr(), Mt.data_ptr(), B, H, W, K, N, tile, s) == 0
                assert torch.equal(Mt[P * Tp * N:], torch.full((GUARD,), SENTINEL, device=dev)), ("behind Mt", K, N, mode, cap)
                return Mt[:P * Tp * N].view(P, Tp, N)

            base = run(0, 0)
            ref = torch.einsum("ptk,pnk->ptn", V0[:, :T].double(), u0.double())
            scale = ref.abs().max().item()
            assert (base[:, :T].double() - ref).abs().max().item() <= 2e-5 * scale
            for cap in (0,) + CAPS:
                got = run(2, cap)
                assert torch.equal(got.view(torch.int32), base.view(torch.int32)), ("Mt", K, N, cap)
            assert torch.equal(V, V0) and torch.equal(u, u0)


@pytest.mark.parametrize("B,H,W,tile", SHAPES)
def test_conv_entry_points_vs_oracle_and_one_tile_kernel(dev, waves, B, H, W, tile):
    """sg_conv2d_fwd_wino / sg_conv2d_bwd_data_wino through the persistent product: bitwise the one-tile kernel's result, within 2e-5 of
    max |ref| of the fp64 oracle; V's pad rows in the workspace and the memory behind the workspace and behind the result are untouched."""
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import lib
    L = lib()
    P, T, Tp = _geom(B, H, W, tile)
    s = ops._stream()
    for K in KS:
        for N in NS:
            x, w, wb, y_ref, dx_ref = _case(dev, B, H, W, K, N)
            u = ops.packed_filter(w, "wino_fwd%d" % tile)
            ub = ops.packed_filter(wb, "wino_bwd%d" % tile)
            nbytes = 4 * P * Tp * (K + N)
            assert L.sg_wino_workspace_bytes(B, H, W, K, N, tile) == nbytes

            def run(mode, cap, fwd):
                ws = torch.full((nbytes // 4 + GUARD,), SENTINEL, device=dev)
                out = torch.full((B * H * W * N + GUARD,), SENTINEL, device=dev)
                L.sg_debug_set_wino_persist(mode, cap)
                if fwd:
                    rc = L.sg_conv2d_fwd_wino(x.data_ptr(), u.data_ptr(), None, None, out.data_ptr(), B, H, W, K, N, 0, tile, ws.data_ptr(), nbytes, s)
                else:
                    rc = L.sg_conv2d_bwd_data_wino(x.data_ptr(), ub.data_ptr(), None, out.data_ptr(), B, H, W, N, K, 0, tile, ws.data_ptr(), nbytes, s)
                assert rc == 0
                fill = torch.full((GUARD,), SENTINEL, device=dev)
                assert torch.equal(ws[nbytes // 4:], fill) and torch.equal(out[B * H * W * N:], fill), ("guards", K, N, mode, cap, fwd)
                if Tp > T:
                    pad = ws[:P * Tp * K].view(P, Tp, K)[:, T:]
                    assert torch.equal(pad, torch.full_like(pad, SENTINEL)), ("V pad rows", K, N, mode, cap, fwd)
                return out[:B * H * W * N].view(B, H, W, N)

            for fwd, ref, name in ((True, y_ref, "y"), (False, dx_ref, "dx")):
                base = run(0, 0, fwd)
                _within(base, ref, "%s one-tile K=%d N=%d" % (name, K, N))
                for cap in CAPS:
                    got = run(2, cap, fwd)
                    assert torch.equal(got.view(torch.int32), base.view(torch.int32)), (name, K, N, cap)
                _within(got, ref, "%s persistent K=%d N=%d" % (name, K, N))


def test_deterministic_mode_is_bitwise_repeatable(dev, waves):
    """Deterministic mode switches the reduction split off, so longer reductions (K = 256: eight k-tiles) reach the persistent kernel too:
    two runs agree bit for bit, with each other and with the one-tile kernel, and with the oracle to 2e-5."""
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import lib
    L = lib()
    B, H, W, K, N = 9, 8, 16, 256, 128
    x, w, _, y_ref, _ = _case(dev, B, H, W, K, N)
    ops.set_deterministic(True)
    try:
        L.sg_debug_set_wino_persist(2, 5)
        a = ops.conv2d_fwd(x, w)
        b = ops.conv2d_fwd(x, w)
        L.sg_debug_set_wino_persist(0, 0)
        c = ops.conv2d_fwd(x, w)
    finally:
        ops.set_deterministic(False)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    _within(a, y_ref, "y deterministic")
