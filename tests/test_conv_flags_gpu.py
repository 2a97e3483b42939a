"""Flag-by-route parity of the convolutions at tile-edge shapes (stride-1 and transposed) against the fp64 oracle.

Every stride-1 entry point of scrabble_gan_amd/ops.py picks one of six kernel families, and every family implements the epilogue
contract of include/scrabble_hip.h on its own -- the direct kernels twice (plain stores, and float atomics for reduction-split
tiles).  Here each family is pinned (`route`), asserted to be the one the op's own predicates select, and run through the flag
matrix at the smallest shapes at which the tiling can go wrong: pixel counts around the tile heights (128 / 256), a sample
boundary inside a tile, H = 1, channel counts on and off the tile grids, never-split / heuristic / three-way-split launches.

What each case checks (tests/conv_refs.py holds the references):
  * max |got - ref| <= tol * max |conv term| + 2^-24 * max |prev|.  The conv term is the fp64 convolution + biases BEFORE the
    accumulate, so a dropped or doubled partial sum cannot hide under a large accumulate operand (max |prev| = 100 x the conv term on
    half of the accumulate cases); the second summand is the rounding of the single fp32 addition prev + conv, which no kernel
    can avoid.  tol is the project's own: 2e-5 fp32 forward / data-grad and 5e-5 weight-grad (test_ops_gpu.py), 2e-5 / 1e-4 Winograd
    (test_winograd_gpu.py), 5e-5 (1e-4 weight-grad) against the oracle on bf16-rounded operands and 1e-2 against the exact one
    (test_bf16_gpu.py), 5e-5 against the oracle on operands quantised like the fp8 kernels' and 6e-2 / 0.15 against the exact one
    (test_fp8_gpu.py).
  * masked elements are exact: bitwise prev with SG_ACCUM, +0.0 without (the mask holds +0.0, -0.0, negatives and positives).
  * the output lies between two guard blocks of one 256-row tile each, bitwise unchanged by the launch (so are the bytes of the
    Winograd workspace beyond sg_wino_workspace_bytes).
"""
import contextlib
import functools
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import conv_refs as R  # noqa: E402
from tests import margins  # noqa: E402

# ================================================================================================================================
# tables
# ================================================================================================================================
# (B, H, W): M = B H W around the tile heights -- 128 (first generation), 256 (second generation)
M_DIRECT = [(1, 8, 16),      # 128
            (1, 3, 43),      # 129
            (3, 5, 17),      # 255
            (1, 8, 32),      # 256
            (1, 1, 257),     # 257; H = 1: every vertical tap of a SAME 3x3 lies outside the image
            (3, 4, 22)]      # 264: a sample boundary inside a tile, a ragged last tile
M_WINO = [(1, 2, 64), (3, 2, 44), (1, 4, 64), (2, 4, 36), (5, 2, 26)]       # the even counterparts
STRADDLE, EXACT = (3, 4, 22), (1, 8, 32)
W_STRADDLE, W_EXACT = (3, 2, 44), (1, 4, 64)

FWD_FLAGS = ["none", "bias", "bias+bias2", "relu_in", "relu_out", "accum", "bias+bias2+accum", "accum+relu_out"]
DGRAD_FLAGS = ["none", "mask", "accum", "mask+accum"]
SPLITS = [1, -1, 3]          # sg_debug_set_splitk / _v2: never split, the heuristic, every tile cut three ways

# route -> conv dtype, operand rounding of its oracle, tolerances (forward / data-grad, weight-grad, against the exact oracle),
# (K, N) = (reduction channels, output channels), kernel sizes, pixel shapes
ROUTES = {
    "f32-gen1": dict(mode="f32", rounding="f32", tol=2e-5, wtol=5e-5, exact=None, chans=[(48, 96)], kernels=[3, 1], shapes=M_DIRECT),
    "f32-v2": dict(mode="f32", rounding="f32", tol=2e-5, wtol=5e-5, exact=None, chans=[(32, 64), (96, 192), (32, 256)], kernels=[3, 1], shapes=M_DIRECT),
    "wino2": dict(mode="f32", rounding="f32", tol=2e-5, wtol=1e-4, exact=None, chans=[(32, 64), (96, 192), (32, 256)], kernels=[3], shapes=M_WINO),
    "wino4": dict(mode="f32", rounding="f32", tol=2e-5, wtol=1e-4, exact=None, chans=[(32, 64), (96, 192), (32, 256)], kernels=[3], shapes=[(1, 4, 64), (2, 4, 36)]),
    "bf16-gen1": dict(mode="bf16", rounding="bf16", tol=5e-5, wtol=1e-4, exact=1e-2, chans=[(40, 192), (72, 64), (72, 256)], kernels=[3, 1], shapes=M_DIRECT),
    "bf16-v2": dict(mode="bf16", rounding="bf16", tol=5e-5, wtol=1e-4, exact=1e-2, chans=[(64, 64), (192, 192), (64, 256)], kernels=[3, 1], shapes=M_DIRECT),
    "fp8": dict(mode="fp8", rounding="fp8", tol=5e-5, wtol=5e-5, exact=6e-2, chans=[(128, 256)], kernels=[3, 1], shapes=M_DIRECT),
}
DIRECT = ("f32-gen1", "f32-v2", "bf16-gen1", "bf16-v2", "fp8")


def _matrix(route):
    """-> [(direction, (B, H, W), (K, N), k, same, flags, split, big)] for one route:
    A  every flag row at one straddling M and one exact-multiple M;
    B  every M of the route's list with bias + bias2 + accum (forward) and mask + accum (data-grad), cycling channels and kernels;
    C  every split state with those two rows at both M (direct families).
    big = the accumulate operand is 100 x the conv term (every other accumulate case)."""
    cfg = ROUTES[route]
    wino = route.startswith("wino")
    pair = (W_STRADDLE, W_EXACT) if route == "wino2" else ((2, 4, 36), (1, 4, 64)) if route == "wino4" else (STRADDLE, EXACT)
    out, n_acc = [], 0

    def add(d, shp, ch, k, same, flags, split):
        nonlocal n_acc
        big = False
        if "accum" in flags:
            big = n_acc % 2 == 1
            n_acc += 1
        out.append((d, shp, ch, k, same, flags, split, big))

    for shp in pair:                                                    # A
        for f in FWD_FLAGS:
            add("fwd", shp, cfg["chans"][0], 3, True, f, -1)
        for f in DGRAD_FLAGS:
            add("dgrad", shp, cfg["chans"][0], 3, True, f, -1)
    for i, shp in enumerate(cfg["shapes"]):                              # B
        ch, k = cfg["chans"][(i + 1) % len(cfg["chans"])], cfg["kernels"][i % len(cfg["kernels"])]
        add("fwd", shp, ch, k, True, "bias+bias2+accum", -1)
        add("dgrad", shp, ch, k, True, "mask+accum", -1)
    if not wino:                                                        # C
        for shp in pair:
            for sp in SPLITS:
                add("fwd", shp, cfg["chans"][-1], 3, True, "bias+bias2+accum", sp)
                add("dgrad", shp, cfg["chans"][-1], 3, True, "mask+accum", sp)
    return out


# what only the first-generation kernels take: 2x2 VALID, channel counts off every grid (N = 66 is off the float4 grid: the [K,N]
# filter loader of the forward launch wants N % 4 == 0, the data-grad's transposing loader does not), the one-channel (thin) kernels
EXTRA = {
    "f32-gen1": [("fwd", STRADDLE, (48, 96), 2, False, "bias+bias2+accum", 3, True), ("dgrad", STRADDLE, (48, 96), 2, False, "mask+accum", 3, False),
                 ("fwd", EXACT, (48, 96), 2, False, "relu_in", -1, False), ("dgrad", EXACT, (48, 96), 2, False, "mask", -1, False),
                 ("dgrad", STRADDLE, (48, 66), 3, True, "mask+accum", -1, True), ("dgrad", (1, 3, 43), (48, 66), 3, True, "mask", 3, False),
                 ("dgrad", EXACT, (48, 66), 1, True, "accum", -1, False),
                 ("fwd", STRADDLE, (48, 1), 3, True, "bias+tanh_out", -1, False), ("fwd", (1, 1, 257), (48, 1), 3, True, "bias+tanh_out", -1, False),
                 ("fwd", (1, 3, 43), (48, 1), 3, True, "bias+accum", -1, True), ("fwd", STRADDLE, (48, 1), 3, True, "relu_out", -1, False),
                 ("dgrad", STRADDLE, (48, 1), 3, True, "mask+accum", -1, False),
                 ("fwd", STRADDLE, (1, 64), 3, True, "bias", -1, False), ("fwd", (1, 3, 43), (1, 64), 3, True, "bias+accum+relu_out", -1, False),
                 ("fwd", (1, 1, 257), (1, 64), 1, True, "relu_in", -1, False), ("dgrad", STRADDLE, (1, 64), 3, True, "mask+accum", -1, True)],
    "bf16-gen1": [("fwd", STRADDLE, (40, 192), 2, False, "bias+bias2+accum", 3, True), ("dgrad", STRADDLE, (40, 192), 2, False, "mask+accum", 3, False),
                  ("fwd", EXACT, (72, 64), 2, False, "relu_in", -1, False), ("dgrad", EXACT, (72, 64), 2, False, "mask", -1, False)],
}


def _all_cases():
    """The matrix of every route plus its extras; a case that two of the rules A / B / C produce is kept once."""
    seen, out = set(), []
    for r in ROUTES:
        for c in _matrix(r) + EXTRA.get(r, []):
            if (r,) + c[:-1] not in seen:
                seen.add((r,) + c[:-1])
                out.append((r,) + c)
    return out


CASES = _all_cases()


def _id(c):
    r, d, (B, H, W), (K, N), k, same, flags, split, big = c
    return "%s-%s-%dx%dx%d-%dto%d-k%d%s-%s-split%d%s" % (r, d, B, H, W, K, N, k, "" if same else "v", flags, split, "-big" if big else "")


# weight gradient: (route, (B, H, W), (Cin, Cout), k)
WGRAD_CASES = [("f32-gen1", STRADDLE, (48, 96), 3), ("f32-gen1", EXACT, (48, 96), 1), ("f32-gen1", (1, 3, 43), (48, 96), 3),
               ("wino2", W_STRADDLE, (32, 64), 3), ("wino2", W_EXACT, (96, 192), 3), ("wino4", (2, 4, 36), (32, 64), 3), ("wino4", (1, 4, 64), (96, 192), 3),
               ("bf16-gen1", (3, 4, 24), (40, 72), 3), ("bf16-gen1", (3, 4, 24), (72, 96), 3), ("bf16-gen1", EXACT, (72, 192), 1),
               ("bf16-v2", (3, 4, 24), (64, 256), 3), ("bf16-v2", EXACT, (64, 64), 3), ("bf16-v2", EXACT, (192, 256), 1),
               ("fp8", (3, 4, 24), (256, 256), 3), ("fp8", EXACT, (256, 256), 1)]

# transposed convolutions: (B, H, W, Cin, Cout)
T_SHAPES = [(2, 4, 8, 64, 32), (1, 3, 43, 64, 96), (2, 4, 16, 128, 64)]
T_STRIDES = [(2, 2), (2, 1), (1, 2)]
T_KERNELS = [3, 1]


def seed_of(*key):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31 - 1)


def mask_specs():
    """(seed, shape) of every ReLU mask the module generates (tests/test_conv_refs_cpu.py checks them without a GPU)."""
    specs = set()
    for r, d, (B, H, W), (K, N), k, same, flags, split, big in CASES:
        specs.add((seed_of(B, H, W, K, N, k, int(same)), (B, H, W, N)))
    for (B, H, W, Cin, Cout) in T_SHAPES + [T_BIG]:
        for st in T_STRIDES:
            for k in T_KERNELS:
                specs.add((seed_of(B, H, W, Cin, Cout, k, st[0], st[1]), (B, H, W, Cin)))
    return sorted(specs)


T_BIG = (4, 64, 128, 64, 32)          # 256 tiles of 128 pixels per parity class: the far side of sg_conv2d_transpose_fwd's pre-zero condition


# ================================================================================================================================
# routes
# ================================================================================================================================
_KNOBS = ("USE_WINOGRAD", "F32_V2_MIN_TILES", "WINO_MIN_C", "WINO_MIN_KN", "WINO_TILE", "WINO4_WGRAD_MIN_TILES", "WINO_ROW_GAIN",
          "OPERAND_ONLY_MIN_TILES")


def set_split(n):
    from scrabble_gan_amd._lib import lib
    lib().sg_debug_set_splitk(int(n))
    lib().sg_debug_set_splitk_v2(int(n))


@contextlib.contextmanager
def route(name, split=-1, deterministic=False):
    """Pin the stride-1 convs to one kernel family with the knobs the existing tests use; everything is restored on the way out."""
    from scrabble_gan_amd import ops
    saved = {k: getattr(ops, k) for k in _KNOBS}
    try:
        ops.set_conv_dtype(ROUTES[name]["mode"] if name in ROUTES else name)
        if name == "f32-gen1":
            ops.USE_WINOGRAD, ops.F32_V2_MIN_TILES = False, 1 << 30
        elif name == "f32-v2":
            ops.USE_WINOGRAD, ops.F32_V2_MIN_TILES = False, 0
        elif name in ("wino2", "wino4"):
            ops.USE_WINOGRAD, ops.WINO_TILE, ops.F32_V2_MIN_TILES = True, int(name[-1]), 1 << 30
            ops.WINO_MIN_C, ops.WINO_MIN_KN, ops.WINO4_WGRAD_MIN_TILES, ops.WINO_ROW_GAIN = {2: 32, 4: 32}, {2: 0, 4: 0}, 0, 0.0
        if deterministic:
            ops.set_deterministic(True)
        else:
            set_split(split)
        yield ops
    finally:
        if deterministic:
            ops.set_deterministic(False)
        set_split(-1)
        for k, v in saved.items():
            setattr(ops, k, v)
        ops.set_conv_dtype("f32")
        ops.new_step()
        ops.end_step()


def family(ops, K, N, k, same, H, W, B, tanh_out=False):
    """The family ops.conv2d_fwd / conv2d_bwd_data launch for reduction channels K, output channels N on B x H x W output pixels:
    the op's own predicates in the op's own order."""
    if ops._wino_ok(K, N, k, k, same, H, W, B) and not tanh_out:
        return "wino%d" % ops._wino_tile(H, W)
    if ops._fp8_ok(K, N, k, k, same) and not tanh_out:
        return "fp8"
    if ops._v2_ok(K, N, k, k, same) and not tanh_out:
        return "bf16-v2"
    if ops._f32v2_ok(K, N, k, k, same, B * H * W) and not tanh_out:
        return "f32-v2"
    if ops._bf16_ok(K, N) and not tanh_out:
        return "bf16-gen1"
    return "f32-gen1"


def wgrad_family(ops, Cin, Cout, k, same, H, W):
    if ops._wino_wgrad_ok(Cin, Cout, k, k, same, H, W):
        t = ops._wino_tile(H, W)
        return "wino%d" % t
    if ops._fp8_wgrad_ok(Cin, Cout, k, k, same):
        return "fp8"
    if ops.USE_V2 and ops._low() and (same or k == 1) and ((Cin % 64 == 0 and Cout % 256 == 0) or (Cin == 64 and Cout == 64 and not ops.DETERMINISTIC)):
        return "bf16-v2"
    return "bf16-gen1" if ops._low() else "f32-gen1"


# ================================================================================================================================
# data and references (computed once per shape, shared by the cases)
# ================================================================================================================================
@functools.lru_cache(maxsize=None)
def case_data(B, H, W, K, N, k, same):
    """Forward: x [B,Hi,Wi,K] * w [k,k,K,N] -> [B,H,W,N].  Data-grad: dy [B,Hd,Wd,K] with the filter wd [k,k,N,K] (Cin = N, Cout = K)
    -> dx [B,H,W,N].  Both launches have reduction channels K, output channels N and B H W output pixels."""
    g = torch.Generator().manual_seed(seed_of(B, H, W, K, N, k, int(same)))
    d = SimpleNamespace()
    d.mask = R.make_mask(g, B, H, W, N)
    Hi, Wi = (H, W) if same else (H + k - 1, W + k - 1)
    Hd, Wd = (H, W) if same else (H - k + 1, W - k + 1)
    d.x, d.w = R.rnd(g, B, Hi, Wi, K), R.f32(R.rnd(g, k, k, K, N) / math.sqrt(k * k * K))
    d.b1, d.b2 = R.rnd(g, N), R.rnd(g, N)
    d.dy, d.wd = R.rnd(g, B, Hd, Wd, K), R.f32(R.rnd(g, k, k, N, K) / math.sqrt(k * k * K))
    return d


@functools.lru_cache(maxsize=None)
def fwd_conv(key, rounding, relu_in):
    d = case_data(*key)
    return R.fwd(d.x, d.w, relu_in=relu_in, same=key[6], rounding=rounding)[0]


@functools.lru_cache(maxsize=None)
def dgrad_conv(key, rounding):
    d = case_data(*key)
    return R.dgrad(d.dy, d.wd, (key[1], key[2]), same=key[6], rounding=rounding)[0]


def g32(t, dev):
    return None if t is None else t.float().to(dev).contiguous()


def check(got, term, full, tol, name, prev=None, keep=None):
    """max |got - full| <= tol * max |term| + 2^-24 * max |prev|; the masked elements (keep == False) bitwise prev / +0.0."""
    g = got.detach().cpu()
    assert g.shape == full.shape, (name, g.shape, full.shape)
    assert torch.isfinite(g).all(), name
    err = (g.double() - full).abs().max().item()
    bnd = R.bound(tol, term, prev)
    print("%s: err %.3e, bound %.3e (%.1f %%)" % (name, err, bnd, 100.0 * err / bnd))
    margins.record(name, tol * err / bnd, tol)
    assert err <= bnd, "%s: max err %.3e > %.3e = %.1e * max|conv term| %.3e + 2^-24 * max|prev| %.3e" % (
        name, err, bnd, tol, term.abs().max().item(), 0.0 if prev is None else prev.abs().max().item())
    if keep is not None and not bool(keep.all()):
        gi = g.contiguous().view(torch.int32)[~keep]
        want = prev.float().contiguous().view(torch.int32)[~keep] if prev is not None else torch.zeros_like(gi)
        assert torch.equal(gi, want), "%s: a masked element is not bitwise %s" % (name, "prev" if prev is not None else "+0.0")


class WinoGuard:
    """The stream's Winograd scratch, oversized and sentinel-filled: the bytes beyond sg_wino_workspace_bytes stay what they were."""

    def __init__(self, ops, dev, B, H, W, K, N, tile):
        from scrabble_gan_amd._lib import lib
        self.ops, self.n = ops, int(lib().sg_wino_workspace_bytes(B, H, W, K, N, tile))
        assert self.n > 0
        self.extra = 4 * 128 * max(K, N)
        self.buf = torch.full((self.n + self.extra,), 0x5a, device=dev, dtype=torch.uint8)
        ops._WINO_WS[ops._stream()] = self.buf

    def check(self, name):
        assert self.ops._WINO_WS[self.ops._stream()] is self.buf, "%s: the workspace was reallocated (sg_wino_workspace_bytes too small?)" % name
        tail = self.buf[self.n:].cpu()
        assert bool((tail == 0x5a).all()), "%s: the launch wrote behind sg_wino_workspace_bytes" % name
        self.ops._WINO_WS.pop(self.ops._stream(), None)


# ================================================================================================================================
# 2. the flag matrix, stride-1 forward and data-grad
# ================================================================================================================================
def run_case(dev, ops, r, d_, B, H, W, K, N, k, same, flags, big, out=None, want16=False, amax_scale=None):
    """One launch of the case on the current route -> (result tensor, term, full, prev, keep).  `out`: a caller-provided result
    tensor (accumulate operand already inside) instead of a guarded one."""
    cfg = ROUTES[r]
    fl = set(flags.split("+")) - {"none"}
    key = (B, H, W, K, N, k, same)
    d = case_data(*key)
    assert family(ops, K, N, k, same, H, W, B, "tanh_out" in fl) == r, "the routing predicates no longer send this case to %s" % r
    gp = torch.Generator().manual_seed(seed_of(*key[:6]) + 1)
    res = SimpleNamespace(exact=None)
    if d_ == "fwd":
        conv = fwd_conv(key, cfg["rounding"], "relu_in" in fl)
        prev = R.make_prev(gp, conv.shape, conv.abs().max().item(), big) if "accum" in fl else None
        b1, b2 = (d.b1 if "bias" in fl else None), (d.b2 if "bias2" in fl else None)
        term = conv + (0 if b1 is None else b1) + (0 if b2 is None else b2)
        full = term if prev is None else term + prev
        full = torch.relu(full) if "relu_out" in fl else torch.tanh(full) if "tanh_out" in fl else full
        keep = None
        if cfg["exact"] is not None:
            te = fwd_conv(key, "f32", "relu_in" in fl) + (0 if b1 is None else b1) + (0 if b2 is None else b2)
            fe = te if prev is None else te + prev
            res.exact = (te, torch.relu(fe) if "relu_out" in fl else fe)
        guard = None if out is not None else R.Guarded(conv.shape, dev, prev)
        o = out if out is not None else guard.t
        got = ops.conv2d_fwd(g32(d.x, dev), g32(d.w, dev), g32(b1, dev), g32(b2, dev), same=same, relu_in="relu_in" in fl, relu_out="relu_out" in fl,
                             tanh_out="tanh_out" in fl, out=o, accum="accum" in fl, want16=want16)
    else:
        conv = dgrad_conv(key, cfg["rounding"])
        prev = R.make_prev(gp, conv.shape, conv.abs().max().item(), big) if "accum" in fl else None
        mask = d.mask.double() if "mask" in fl else None
        if mask is not None:
            R.check_mask(d.mask)
        keep = None if mask is None else mask > 0
        term = conv
        full = (term if keep is None else term * keep) + (0 if prev is None else prev)
        if cfg["exact"] is not None:
            te = dgrad_conv(key, "f32")
            res.exact = (te, (te if keep is None else te * keep) + (0 if prev is None else prev))
        guard = None if out is not None else R.Guarded(conv.shape, dev, prev)
        o = out if out is not None else guard.t
        got = ops.conv2d_bwd_data(g32(d.dy, dev), g32(d.wd, dev), (H, W), mask=None if mask is None else d.mask.to(dev), same=same, out=o,
                                  accum="accum" in fl, want16=want16, amax_scale=amax_scale)
    torch.cuda.synchronize()
    res.got, res.term, res.full, res.prev, res.keep, res.guard = got, term, full, prev, keep, guard
    return res


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_flag_matrix(dev, case):
    r, d_, (B, H, W), (K, N), k, same, flags, split, big = case
    cfg = ROUTES[r]
    with route(r, split) as ops:
        wg = WinoGuard(ops, dev, B, H, W, K, N, int(r[-1])) if r.startswith("wino") else None
        res = run_case(dev, ops, r, d_, B, H, W, K, N, k, same, flags, big)
        name = _id(case)
        res.guard.check(name)
        if wg is not None:
            wg.check(name)
        check(res.got, res.term, res.full, cfg["tol"], name, res.prev, res.keep)
        if res.exact is not None and "tanh_out" not in flags:
            check(res.got, res.exact[0], res.exact[1], cfg["exact"], name + " vs exact oracle", res.prev)


# ================================================================================================================================
# 2. weight gradient: relu_in x db x sample_scale, += on a non-zero dw / db
# ================================================================================================================================
@pytest.mark.parametrize("r,shp,ch,k", WGRAD_CASES, ids=["%s-%dx%dx%d-%dto%d-k%d" % ((r,) + s + c + (k,)) for r, s, c, k in WGRAD_CASES])
def test_weight_grad_flags(dev, r, shp, ch, k):
    """dw += and db += on non-zero contents for every combination of SG_RELU_IN, a bias gradient and per-sample factors.  The bias
    gradient sums fp32 values on every route (5e-5; 1e-4 in the Winograd domain)."""
    (B, H, W), (Cin, Cout) = shp, ch
    cfg = ROUTES[r]
    g = torch.Generator().manual_seed(seed_of(B, H, W, Cin, Cout, k, 77))
    x, dy = R.rnd(g, B, H, W, Cin), R.rnd(g, B, H, W, Cout)
    sc = R.f32(torch.rand(B, generator=g, dtype=torch.float64) * 2 - 0.5)
    dw0, db0 = R.rnd(g, k, k, Cin, Cout), R.rnd(g, Cout)
    rounding, wtol = cfg["rounding"], cfg["wtol"]
    if r == "bf16-gen1" and not (Cin >= 64 and Cout >= 64 and W % 4 == 0):
        rounding, wtol = "f32", 5e-5          # sg_conv2d_bwd_weight(SG_MMA_BF16) keeps fp32 operands below 64 channels: the exact oracle, the fp32 bar
    with route(r) as ops:
        assert wgrad_family(ops, Cin, Cout, k, True, H, W) == r
        xg, dyg, scg = g32(x, dev), g32(dy, dev), g32(sc, dev)
        for relu_in in (False, True):
            for scaled in (False, True):
                ref_w, ref_b = R.wgrad(x, dy, (k, k, Cin, Cout), relu_in, sc if scaled else None, rounding=rounding)
                for with_db in (False, True):
                    name = "%s relu_in=%d scale=%d db=%d" % (r, relu_in, scaled, with_db)
                    gw, gb = R.Guarded(dw0.shape, dev, dw0), R.Guarded(db0.shape, dev, db0)
                    ops.new_step()
                    ops.conv2d_bwd_weight(xg, dyg, gw.t, relu_in=relu_in, db=gb.t if with_db else None, sample_scale=scg if scaled else None)
                    torch.cuda.synchronize()
                    gw.check(name + " dw")
                    gb.check(name + " db")
                    check(gw.t, ref_w, ref_w + dw0, wtol, name + " dW", dw0)
                    if with_db:
                        check(gb.t, ref_b, ref_b + db0, 1e-4 if r.startswith("wino") else 5e-5, name + " db", db0)
                    else:
                        assert torch.equal(gb.t.cpu(), db0.float()), name + ": db written although none was passed"


# ================================================================================================================================
# 2. low-precision extras: bf16 twins, amax slots, operand-only results
# ================================================================================================================================
LOWP = [("bf16-v2", "bf16", (64, 64)), ("bf16-v2", "fp8", (192, 192)), ("fp8", "fp8", (128, 256))]      # (family, conv dtype, (K, N))


@pytest.mark.parametrize("fam,mode,ch", LOWP, ids=["%s-in-%s-mode" % (f, m) for f, m, _ in LOWP])
@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("shp", [STRADDLE, EXACT])
def test_twin_and_amax(dev, fam, mode, ch, split, shp):
    """want16=True: the twin equals result.to(bfloat16) bitwise on every row, reduction-split rows included; in fp8 mode the recorded
    amax pair is exactly (max |result|, max |scale[b] result|)."""
    (B, H, W), (K, N) = shp, ch
    with route(fam, split) as ops:
        ops.set_conv_dtype(mode)
        for d_, flags in (("fwd", "bias+bias2"), ("fwd", "bias+accum"), ("dgrad", "mask"), ("dgrad", "mask+accum")):
            name = "%s %s %s split %d" % (fam, d_, flags, split)
            conv_shape = (B, H, W, N)
            gp = torch.Generator().manual_seed(5)
            out = torch.randn(*conv_shape, generator=gp).to(dev) if "accum" in flags else torch.empty(*conv_shape, device=dev)
            prev = out.clone()
            sc = g32(torch.rand(B, generator=gp, dtype=torch.float64) * 2 - 0.5, dev) if d_ == "dgrad" else None
            ops.new_step()
            d = case_data(B, H, W, K, N, 3, True)
            if d_ == "fwd":
                got = ops.conv2d_fwd(g32(d.x, dev), g32(d.w, dev), g32(d.b1, dev), g32(d.b2, dev) if "bias2" in flags else None, out=out,
                                     accum="accum" in flags, want16=True)
                assert family(ops, K, N, 3, True, H, W, B) == fam
            else:
                got = ops.conv2d_bwd_data(g32(d.dy, dev), g32(d.wd, dev), (H, W), mask=d.mask.to(dev), out=out, accum="accum" in flags, want16=True,
                                          amax_scale=sc)
            torch.cuda.synchronize()
            assert got is out and torch.isfinite(got).all(), name
            if "accum" in flags:
                assert not torch.equal(got, prev), name
            t16 = ops._twin_get(got)
            assert t16 is not None, name + ": no twin registered"
            assert torch.equal(t16.view(torch.int16), got.to(torch.bfloat16).view(torch.int16)), name + ": twin != bf16(result)"
            rec = ops._amax_get(got, sc, need_scaled=sc is not None)
            if mode == "fp8":
                assert rec is not None, name + ": no amax recorded"
                assert rec[0].item() == got.abs().max().item(), name + ": amax[0]"
                want1 = got.abs().max().item() if sc is None else (got.abs() * sc.abs().view(B, 1, 1, 1)).max().item()
                assert rec[1].item() == want1, name + ": amax[1]"
            else:
                assert rec is None


@pytest.mark.parametrize("fam,mode,ch", [("bf16-v2", "bf16", (64, 64)), ("fp8", "fp8", (128, 256))], ids=["bf16", "fp8"])
@pytest.mark.parametrize("shp", [STRADDLE, EXACT])
def test_operand_only_result(dev, fam, mode, ch, shp):
    """want16="only" under the NaN poison of tests/conftest.py: the fp32 handle stays all-NaN, the bf16 copy is bitwise the twin of the
    never-split ordinary launch (an operand-only launch has no reduction split: the partial tiles would meet in the fp32 result)."""
    (B, H, W), (K, N) = shp, ch
    d = case_data(B, H, W, K, N, 3, True)
    with route(fam, 1) as ops:
        assert ops.GHOST_NAN
        ops.OPERAND_ONLY_MIN_TILES = 0
        assert ops.operand_only_ok(B, H, W, N) and family(ops, K, N, 3, True, H, W, B) == fam
        xg, wg, bg = g32(d.x, dev), g32(d.w, dev), g32(d.b1, dev)
        ref = ops.conv2d_fwd(xg, wg, bg, relu_in=True, want16=True)
        t_ref = ops._twin_get(ref).clone()
        ops.new_step()
        set_split(-1)
        ghost = ops.conv2d_fwd(xg, wg, bg, relu_in=True, want16="only")
        torch.cuda.synchronize()
        assert torch.isnan(ghost).all(), "the fp32 handle of an operand-only result was written"
        assert torch.equal(ops._twin_get(ghost).view(torch.int16), t_ref.view(torch.int16))
        with pytest.raises(RuntimeError):
            ops._p(ghost)


# ================================================================================================================================
# 4. transposed convolutions
# ================================================================================================================================
@functools.lru_cache(maxsize=None)
def t_data(B, H, W, Cin, Cout, k, sh, sw):
    g = torch.Generator().manual_seed(seed_of(B, H, W, Cin, Cout, k, sh, sw))
    d = SimpleNamespace()
    d.mask = R.make_mask(g, B, H, W, Cin)
    d.x, d.w = R.rnd(g, B, H, W, Cin), R.f32(R.rnd(g, k, k, Cout, Cin) / math.sqrt(k * k * Cin))
    d.b1, d.b2, d.dy = R.rnd(g, Cout), R.rnd(g, Cout), R.rnd(g, B, sh * H, sw * W, Cout)
    d.dw0 = R.rnd(g, k, k, Cout, Cin)
    return d


def run_transposed(dev, ops, mode, B, H, W, Cin, Cout, k, st, fwd_rows, dgrad_rows, wgrad=True):
    sh, sw = st
    d = t_data(B, H, W, Cin, Cout, k, sh, sw)
    R.check_mask(d.mask)
    xg, wg, dyg = g32(d.x, dev), g32(d.w, dev), g32(d.dy, dev)
    low = mode == "bf16"
    f_round = "bf16" if low and ops._bf16_ok(Cin, Cout) and k >= sh and k >= sw else "f32"
    d_round = "bf16" if low and ops._bf16_ok(Cout, Cin) else "f32"
    w_round = "bf16" if low and Cin % 64 == 0 and Cout % 64 == 0 and H * W >= 64 else "f32"
    tol = lambda rd: 5e-5 if rd == "bf16" else 2e-5
    gp = torch.Generator().manual_seed(3)
    for i, flags in enumerate(fwd_rows):
        fl = set(flags.split("+"))
        conv = R.t_fwd(d.x, d.w, stride=st, rounding=f_round)[0]
        b1, b2 = (d.b1 if "bias" in fl else None), (d.b2 if "bias2" in fl else None)
        prev = R.make_prev(gp, conv.shape, conv.abs().max().item(), i % 2 == 1) if "accum" in fl else None
        term, full = R.t_fwd(d.x, d.w, b1, b2, st, prev, f_round)
        name = "convT fwd %s %s" % (mode, flags)
        gd = R.Guarded(conv.shape, dev, prev)
        ops.conv2d_transpose_fwd(xg, wg, g32(b1, dev), g32(b2, dev), stride=st, out=gd.t, accum="accum" in fl)
        torch.cuda.synchronize()
        gd.check(name)
        check(gd.t, term, full, tol(f_round), name, prev)
        if k == 1 and sh * sw > 1:          # parity classes without a tap hold exactly bias (+ bias2) (+ prev): fp32 sums of fp32 values
            tapless = torch.ones(sh * H, sw * W, dtype=torch.bool)
            tapless[::sh, ::sw] = False
            want = torch.zeros(*conv.shape, dtype=torch.float32)
            for b in (b1, b2):
                if b is not None:
                    want = want + b.float()
            if prev is not None:
                want = want + prev.float()
            assert torch.equal(gd.t.cpu()[:, tapless], want[:, tapless]), name + ": a tap-less parity class is not exactly bias (+ bias2) (+ prev)"
    for i, flags in enumerate(dgrad_rows):
        fl = set(flags.split("+"))
        mask = d.mask.double() if "mask" in fl else None
        conv = R.t_dgrad(d.dy, d.w, st, rounding=d_round)[0]
        prev = R.make_prev(gp, conv.shape, conv.abs().max().item(), i % 2 == 0) if "accum" in fl else None
        term, keep, full = R.t_dgrad(d.dy, d.w, st, mask, prev, d_round)
        name = "convT dgrad %s %s" % (mode, flags)
        gd = R.Guarded(conv.shape, dev, prev)
        ops.conv2d_transpose_bwd_data(dyg, wg, stride=st, mask=None if mask is None else d.mask.to(dev), out=gd.t, accum="accum" in fl)
        torch.cuda.synchronize()
        gd.check(name)
        check(gd.t, term, full, tol(d_round), name, prev, keep if mask is not None else None)
    if wgrad:
        ref = R.t_wgrad(d.x, d.dy, d.dw0.shape, st, w_round)
        gd = R.Guarded(d.dw0.shape, dev, d.dw0)
        ops.new_step()
        ops.conv2d_transpose_bwd_weight(xg, dyg, gd.t, stride=st)
        torch.cuda.synchronize()
        gd.check("convT dW")
        check(gd.t, ref, ref + d.dw0, 1e-4 if w_round == "bf16" else 5e-5, "convT dW %s (+= on non-zero dw)" % mode, d.dw0)


T_FWD_ROWS = ["bias", "bias+bias2", "accum", "bias+accum"]
T_DGRAD_ROWS = ["none", "mask", "accum", "mask+accum"]


@pytest.mark.parametrize("mode", ["f32", "bf16"])
@pytest.mark.parametrize("k", T_KERNELS)
@pytest.mark.parametrize("st", T_STRIDES, ids=lambda s: "s%dx%d" % s)
@pytest.mark.parametrize("shp", T_SHAPES, ids=lambda s: "%dx%dx%d-%dto%d" % s)
def test_transposed_flags(dev, mode, k, st, shp):
    """conv2d_transpose_fwd / _bwd_data / _bwd_weight: the generator's ResBlockUp uses bias2, accum (the shortcut add) and the
    accumulating data-grad.  All of these shapes are on the pre-zeroing side of sg_conv2d_transpose_fwd (few tiles per class)."""
    with route(mode) as ops:
        run_transposed(dev, ops, mode, *shp, k, st, T_FWD_ROWS, T_DGRAD_ROWS)


@pytest.mark.parametrize("split", [-1, 3])
@pytest.mark.parametrize("shp", [T_SHAPES[0], T_SHAPES[2]], ids=lambda s: "%dx%dx%d-%dto%d" % s)
def test_transposed_forced_split(dev, split, shp):
    """Pre-zeroed output: the parity-class launches split onto the zeros (bias on split 0 only); with accum they split onto prev."""
    with route("f32", split) as ops:
        run_transposed(dev, ops, "f32", *shp, 3, (2, 2), T_FWD_ROWS, ["mask+accum"], wgrad=False)


@pytest.mark.parametrize("split", [-1, 3])
def test_transposed_no_prezero_branch(dev, split):
    """256 tiles per parity class: sg_conv2d_transpose_fwd neither zeroes y nor sets SG_PREZEROED; the strided classes then only split
    when they accumulate."""
    B, H, W, Cin, Cout = T_BIG
    assert -(-(B * H * W) // 128) * -(-Cout // 128) >= 256
    with route("f32", split) as ops:
        run_transposed(dev, ops, "f32", B, H, W, Cin, Cout, 3, (2, 2), ["bias+bias2", "bias+accum"], [], wgrad=False)


@pytest.mark.parametrize("hw,v2", [((4, 16), True), ((4, 15), False)], ids=["HW64-bf16v2", "HW60-fp32"])
def test_transposed_weight_grad_bf16v2_gate(dev, hw, v2):
    """bf16 mode: Cin, Cout % 64 == 0 and H W >= 64 -> the DMA-fed bf16 weight-grad; H W = 60 -> the fp32 kernel (exact operands)."""
    B, Cin, Cout = 2, 128, 64
    with route("bf16") as ops:
        assert (ops.USE_V2 and Cin % 64 == 0 and Cout % 64 == 0 and hw[0] * hw[1] >= 64) == v2
        run_transposed(dev, ops, "bf16", B, hw[0], hw[1], Cin, Cout, 3, (2, 2), [], [], wgrad=True)


# ================================================================================================================================
# 5. contract edges of the C ABI: argument checks that return before any launch
# ================================================================================================================================
SG_ERR_ARG, SG_ERR_UNSUPPORTED, SG_ACCUM = -1, -3, 2


def test_abi_rejects_off_grid_shapes_untouched(dev):
    from scrabble_gan_amd._lib import lib
    L = lib()
    n = 1 << 20
    a = torch.zeros(n, device=dev)                      # every operand: valid, zero-filled, larger than any shape below
    b = torch.zeros(n, device=dev)
    am = torch.ones(2, device=dev)
    out = torch.full((n,), R.SENTINEL, device=dev)
    out16 = torch.full((n,), R.SENTINEL, device=dev)
    A, Bp, AM, O_, O16 = a.data_ptr(), b.data_ptr(), am.data_ptr(), out.data_ptr(), out16.data_ptr()
    Bn, H, W = 2, 4, 8
    U = SG_ERR_UNSUPPORTED
    calls = [
        ("sg_conv2d_fwd_v2 K=48", U, lambda: L.sg_conv2d_fwd_v2(A, Bp, None, None, O_, Bn, H, W, 48, 64, 3, 3, 1, 0, None)),
        ("sg_conv2d_fwd_v2 N=96", U, lambda: L.sg_conv2d_fwd_v2(A, Bp, None, None, O_, Bn, H, W, 64, 96, 3, 3, 1, 0, None)),
        ("sg_conv2d_bwd_data_v2 K=48", U, lambda: L.sg_conv2d_bwd_data_v2(A, Bp, None, O_, Bn, H, W, 64, 48, 3, 3, 1, 0, None)),
        ("sg_conv2d_fwd_bf16v2 K=96", U, lambda: L.sg_conv2d_fwd_bf16v2(A, Bp, None, None, O_, O16, Bn, H, W, 96, 64, 3, 3, 1, 0, None, None)),
        ("sg_conv2d_fwd_bf16v2 N=96", U, lambda: L.sg_conv2d_fwd_bf16v2(A, Bp, None, None, O_, O16, Bn, H, W, 64, 96, 3, 3, 1, 0, None, None)),
        ("sg_conv2d_bwd_data_bf16v2 K=96", U, lambda: L.sg_conv2d_bwd_data_bf16v2(A, Bp, None, None, O_, O16, Bn, H, W, 64, 96, 3, 3, 1, 0, None, None, None)),
        ("sg_conv2d_bwd_weight_bf16v2 Cin=96", U, lambda: L.sg_conv2d_bwd_weight_bf16v2(A, Bp, O_, Bn, H, W, 96, 256, 3, 3, 1, 0, None)),
        ("sg_conv2d_bwd_weight_bf16v2 Cout=128", U, lambda: L.sg_conv2d_bwd_weight_bf16v2(A, Bp, O_, Bn, H, W, 128, 128, 3, 3, 1, 0, None)),
        ("sg_conv2d_bwd_weight_bf16v2 VALID 3x3", U, lambda: L.sg_conv2d_bwd_weight_bf16v2(A, Bp, O_, Bn, H, W, 64, 256, 3, 3, 0, 0, None)),
        ("sg_conv2d_fwd_fp8 N=128", U, lambda: L.sg_conv2d_fwd_fp8(A, AM, Bp, AM, None, None, O_, O16, Bn, H, W, 128, 128, 3, 3, 1, 0, None, None)),
        ("sg_conv2d_fwd_fp8 K=64", U, lambda: L.sg_conv2d_fwd_fp8(A, AM, Bp, AM, None, None, O_, O16, Bn, H, W, 64, 256, 3, 3, 1, 0, None, None)),
        ("sg_conv2d_fwd_fp8 SG_RELU_IN", U, lambda: L.sg_conv2d_fwd_fp8(A, AM, Bp, AM, None, None, O_, O16, Bn, H, W, 128, 256, 3, 3, 1, 1, None, None)),
        ("sg_conv2d_bwd_weight_fp8 Cin=128", U, lambda: L.sg_conv2d_bwd_weight_fp8(A, AM, Bp, AM, O_, Bn, H, W, 128, 256, 3, 3, 1, None)),
        ("sg_conv2d_bwd_weight_fp8 Cout=128", U, lambda: L.sg_conv2d_bwd_weight_fp8(A, AM, Bp, AM, O_, Bn, H, W, 256, 128, 3, 3, 1, None)),
        ("sg_conv2d_transpose_fwd_bf16 1x1 s2", U, lambda: L.sg_conv2d_transpose_fwd_bf16(A, Bp, None, None, O_, Bn, H, W, 64, 64, 1, 1, 2, 2, 0, None)),
        ("sg_conv2d_transpose_fwd_bf16 1x1 s(1,2)", U, lambda: L.sg_conv2d_transpose_fwd_bf16(A, Bp, None, None, O_, Bn, H, W, 64, 64, 1, 1, 1, 2, 0, None)),
        ("sg_conv2d_transpose_fwd_bf16 N=32", U, lambda: L.sg_conv2d_transpose_fwd_bf16(A, Bp, None, None, O_, Bn, H, W, 64, 32, 3, 3, 2, 2, 0, None)),
        ("sg_conv2d_transpose_fwd_bf16 K=44", U, lambda: L.sg_conv2d_transpose_fwd_bf16(A, Bp, None, None, O_, Bn, H, W, 44, 64, 3, 3, 2, 2, 0, None)),
        ("sg_conv2d_transpose_bwd_weight_bf16v2 HW=60", U, lambda: L.sg_conv2d_transpose_bwd_weight_bf16v2(A, Bp, O_, Bn, 4, 15, 128, 64, 3, 3, 2, 2, None)),
        ("sg_conv2d_transpose_bwd_weight_bf16v2 Cin=96", U, lambda: L.sg_conv2d_transpose_bwd_weight_bf16v2(A, Bp, O_, Bn, 4, 16, 96, 64, 3, 3, 2, 2, None)),
        ("sg_conv2d_fwd_bf16v2 y NULL + SG_ACCUM", SG_ERR_ARG, lambda: L.sg_conv2d_fwd_bf16v2(A, Bp, None, None, None, O16, Bn, H, W, 64, 64, 3, 3, 1, SG_ACCUM, None, None)),
        ("sg_conv2d_fwd_fp8 y NULL + SG_ACCUM", SG_ERR_ARG, lambda: L.sg_conv2d_fwd_fp8(A, AM, Bp, AM, None, None, None, O16, Bn, H, W, 128, 256, 3, 3, 1, SG_ACCUM, None, None)),
    ]
    want = torch.full((n,), R.SENTINEL).view(torch.int32)
    for name, rc_want, fn in calls:
        rc = fn()
        torch.cuda.synchronize()
        assert rc == rc_want, "%s returned %d, expected %d" % (name, rc, rc_want)
        assert torch.equal(out.cpu().view(torch.int32), want) and torch.equal(out16.cpu().view(torch.int32), want), name + " wrote to its output"


# ================================================================================================================================
# 6. deterministic mode
# ================================================================================================================================
DET = [(r, ROUTES[r]["chans"][-1]) for r in ROUTES]


@pytest.mark.parametrize("r,ch", DET, ids=[r for r, _ in DET])
def test_deterministic_mode(dev, r, ch):
    """ops.set_deterministic(True): two launches are bitwise equal, and sample 0 of a B = 3 launch is bitwise the same sample launched
    alone -- at the shape whose tiles straddle samples.  (The per-tensor scale of an fp8 operand is the amax of the WHOLE tensor: the
    largest |element| of each activation operand is put into sample 0, so that the operand bytes of sample 0 do not depend on the
    batch.)"""
    (K, N), (B, H, W) = ch, ((2, 4, 36) if r == "wino4" else W_STRADDLE if r == "wino2" else STRADDLE)
    if r == "wino4":
        B = 3
    d = case_data(B, H, W, K, N, 3, True)
    x, dy = d.x.clone(), d.dy.clone()
    x[0, 0, 0, 0], dy[0, 0, 0, 0] = 8.0, -8.0
    gp = torch.Generator().manual_seed(9)
    prev = torch.randn(B, H, W, N, generator=gp)
    with route(r, deterministic=True) as ops:
        assert family(ops, K, N, 3, True, H, W, B) == r and family(ops, K, N, 3, True, H, W, 1) == r
        wg, wdg, b1 = g32(d.w, dev), g32(d.wd, dev), g32(d.b1, dev)

        def fwd(n):
            ops.new_step()
            return ops.conv2d_fwd(g32(x[:n], dev), wg, b1, relu_in=True, out=prev[:n].to(dev), accum=True).cpu()

        def dgr(n):
            ops.new_step()
            return ops.conv2d_bwd_data(g32(dy[:n], dev), wdg, (H, W), mask=d.mask[:n].to(dev), out=prev[:n].to(dev), accum=True).cpu()

        for name, f in (("forward bias+accum", fwd), ("data-grad mask+accum", dgr)):
            a, b, one = f(B), f(B), f(1)
            assert torch.isfinite(a).all() and not torch.equal(a, prev)
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s %s: two launches differ" % (r, name)
            assert torch.equal(a[:1].view(torch.int32), one.view(torch.int32)), "%s %s: sample 0 depends on the batch it is launched in" % (r, name)
