"""Op-level GPU parity of the BiLSTM recognizer path and of the entry points no other test calls directly: one BiLSTM layer through
nn.bilstm_fwd / nn.bilstm_bwd, the LSTM cell kernels alone, ops.gemm addressing (column blocks of wider matrices, offsets, beta = 0),
the dense wrappers, the elementwise ops of make_my_recognizer, the loss terms, and spectral norm forward + backward at the shapes
where its kernels change path.

The references are the fp64 CPU oracle (or plain fp64 formulas written here) on seeded inputs; the bounds are the project's fp32 op
bounds, 2e-5 on forward results and 5e-5 on gradients / accumulate forms, relative to max|ref| of the tensor (`close()`, as in
test_ops_gpu.py).  The oracle's own fp32-vs-fp64 gap on O.bilstm is <= 7e-7 at these sizes, under 4 % of the bounds.

A `+=` result is compared with prefill + reference where the prefill is drawn at the scale of the reference gradient of that tensor
(a prefill far larger than the gradient would hide the gradient's error inside the bound on the sum)."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import margins  # noqa: E402

from oracle import scrabble_oracle as O  # noqa: E402  (checker only)

SENTINEL = -777.25       # exactly representable; nothing computed below comes near it


def close(got, ref, tol=2e-5, name=""):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    err = (got - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-12
    margins.record(name, err / scale, tol)
    assert err <= tol * scale, "%s: max err %.3e vs scale %.3e (rel %.3e > %.1e)" % (name, err, scale, err / scale, tol)


def close_abs(got, ref, atol, name=""):
    """max|got - ref| <= atol (recorded as error / 1 against the bound `atol`)."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert torch.isfinite(got).all(), name
    err = (got - ref).abs().max().item()
    margins.record(name, err, atol)
    assert err <= atol, "%s: max abs err %.3e > %.1e" % (name, err, atol)


def rnd(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64)


def g32(t, dev):
    return t.float().to(dev).contiguous()


def untouched_outside(after, before, block, name=""):
    """`after` (device) is bit-identical to `before` (host copy taken before the launch) outside the boolean mask `block`."""
    a, b = after.detach().cpu().clone(), before.clone()
    assert a.shape == b.shape == block.shape, (name, a.shape, b.shape, block.shape)
    a[block], b[block] = 0.0, 0.0
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: wrote outside its block" % name


def prefill_like(gen, ref):
    """Random prefill of a `+=` target at the scale of its reference gradient (unit scale where that gradient is zero)."""
    s = ref.abs().max().item()
    return rnd(gen, *ref.shape) * (s if s > 0 else 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# 1. one BiLSTM layer against O.bilstm
# ------------------------------------------------------------------------------------------------------------------------------
BILSTM_CASES = [
    (3, 1, 20, 10),       # no recurrence: only the first-step branches (c_prev = None, h_copy = None) of both directions
    (3, 2, 20, 10),       # one recurrent step; 4H = 40: a ragged 32-wide GEMM tile, gate quarters at offsets that are no multiple of 4 floats
    (1, 5, 24, 72),       # B = 1
    (33, 5, 144, 72),     # two ragged M tiles in the recurrent GEMM, I = 144 as in layer 1, 4H = 288
    (3, 3, 512, 256),     # the model's own H, I = 2H as in layers 2-5
]
_DIRS = ("fw", "bw")
_BILSTM_REF = {}


def _bilstm_reference(B, T, I, H, masked):
    """Inputs (fp64, seeded) and the autograd reference of one case, computed once and shared; nothing mutates it."""
    key = (B, T, I, H, masked)
    if key in _BILSTM_REF:
        return _BILSTM_REF[key]
    gen = torch.Generator().manual_seed(4321 + 7 * B + 31 * T + I + 3 * H + (1 if masked else 0))
    p = {}
    for d in _DIRS:
        p["l.%s.W" % d] = O.glorot_uniform((I, 4 * H), gen)
        p["l.%s.U" % d] = O.orthogonal((H, 4 * H), gen)
        p["l.%s.b" % d] = rnd(gen, 4 * H) * 0.3           # random: the default forget-bias pattern would hide a gate-order slip
    x = rnd(gen, B, T, I)
    masks = None
    if masked:                                            # two independent per-direction input-dropout masks of {0, 2}
        masks = tuple(torch.randint(0, 2, (B, I), generator=gen).double() * 2.0 for _ in _DIRS)
    dout = rnd(gen, B, T, 2 * H)
    leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xr = x.clone().requires_grad_(True)
    out = O.bilstm(xr, leaves, "l", masks)
    out.backward(dout)
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach() for k, v in leaves.items()}
    prefill = {k: prefill_like(gen, grads[k]) for k in sorted(grads)}
    ref = {"p": p, "x": x, "masks": masks, "dout": dout, "out": out.detach(), "dx": xr.grad.detach(), "grads": grads, "prefill": prefill}
    _BILSTM_REF[key] = ref
    return ref


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "masks"])
@pytest.mark.parametrize("B,T,I,H", BILSTM_CASES)
def test_bilstm_layer(dev, B, T, I, H, masked):
    from scrabble_gan_amd import nn
    R = _bilstm_reference(B, T, I, H, masked)
    S = nn.ParamStore(nn.bilstm_specs("l", I, H), dev, torch.Generator().manual_seed(0))
    S.load(R["p"])
    xg, doutg = g32(R["x"], dev), g32(R["dout"], dev)
    gmasks = None if R["masks"] is None else tuple(g32(m, dev) for m in R["masks"])
    names = sorted(R["grads"])

    # gradients into a zeroed store
    out, ctx = nn.bilstm_fwd(xg, S, "l", gmasks)
    close(out, R["out"], 2e-5, "out")
    S.zero_grad()
    dx = nn.bilstm_bwd(ctx, doutg, S, "l", want_dw=True)
    close(dx, R["dx"], 5e-5, "dx")
    for k in names:
        if T == 1 and k.endswith(".U"):                   # no recurrent step: h_{t-1} = 0 for the only step, so gU's scale is 0
            assert R["grads"][k].abs().max().item() == 0.0
            assert S.g[k].abs().max().item() == 0.0, "%s must be exactly zero at T = 1" % k
        else:
            close(S.g[k], R["grads"][k], 5e-5, "g" + k[1:])

    # += semantics: the same gradients on top of a non-zero store (the backward pass consumed the gates: forward again)
    out, ctx = nn.bilstm_fwd(xg, S, "l", gmasks)
    close(out, R["out"], 2e-5, "out (second pass)")
    for k in names:
        S.g[k].copy_(g32(R["prefill"][k], dev))
    pre32 = {k: S.g[k].detach().cpu().clone() for k in names}
    dx = nn.bilstm_bwd(ctx, doutg, S, "l", want_dw=True)
    close(dx, R["dx"], 5e-5, "dx (prefilled store)")
    for k in names:
        if T == 1 and k.endswith(".U"):
            assert torch.equal(S.g[k].cpu(), pre32[k]), "%s: prefill + 0 must stay the prefill" % k
        else:
            close(S.g[k], pre32[k].double() + R["grads"][k], 5e-5, "prefill + g" + k[1:])

    # want_dw=False: dx unchanged, the gradient store bit-identical to its prefill
    out, ctx = nn.bilstm_fwd(xg, S, "l", gmasks)
    flat_before = S.grad.detach().cpu().clone()
    dx = nn.bilstm_bwd(ctx, doutg, S, "l", want_dw=False)
    close(dx, R["dx"], 5e-5, "dx (want_dw=False)")
    assert torch.equal(S.grad.cpu().view(torch.int32), flat_before.view(torch.int32)), "want_dw=False wrote into the gradient store"


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the LSTM cell kernels alone, operands embedded in wider buffers at a non-zero offset
# ------------------------------------------------------------------------------------------------------------------------------
def _embed(block, ld, off, dev):
    """-> (device buffer [B, ld] of SENTINEL holding `block` [B, w] in columns off..off+w, host copy, boolean mask of those columns).
    The kernel's `offset` argument is `off`, its row stride `ld`."""
    Bn, w = block.shape
    buf = torch.full((Bn, ld), SENTINEL, dtype=torch.float32)
    buf[:, off:off + w] = block.float()
    mask = torch.zeros(Bn, ld, dtype=torch.bool)
    mask[:, off:off + w] = True
    return buf.to(dev), buf.clone(), mask


def _cell_fwd_ref(z, cp):
    H = z.shape[1] // 4
    i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
    c = f * cp + i * g
    return (i, f, g, o), c, o * torch.tanh(c)


def _run_cell_fwd(dev, z, cp, with_cprev, with_hcopy):
    """Launch ops.lstm_cell_fwd on embedded operands; -> gate quarters, c, h, h_copy block (or None), after checking that nothing
    outside the addressed blocks changed."""
    from scrabble_gan_amd import ops
    B, H4 = z.shape
    H = H4 // 4
    ldz, z_off = 3 * H4, H4
    ldh, h_off = 2 * H + 7, 3
    ldc, hc_off = H + 5, 2
    zb, z0, zm = _embed(z, ldz, z_off, dev)
    hb, h0, hm = _embed(torch.full((B, H), SENTINEL, dtype=torch.float64), ldh, h_off, dev)
    cb, c0, cm = _embed(torch.full((B, H), SENTINEL, dtype=torch.float64), ldc, hc_off, dev)
    c_out = torch.full((B, H), SENTINEL, device=dev)
    ops.lstm_cell_fwd(zb, z_off, ldz, g32(cp, dev) if with_cprev else None, c_out, hb, h_off, ldh, cb if with_hcopy else None,
                      hc_off if with_hcopy else 0, ldc, B, H)
    torch.cuda.synchronize()
    untouched_outside(zb, z0, zm, "z")
    untouched_outside(hb, h0, hm, "h_out")
    if with_hcopy:
        untouched_outside(cb, c0, cm, "h_copy")
    else:
        assert torch.equal(cb.cpu(), c0), "h_copy=None must not be written"
    gates = zb[:, z_off:z_off + H4]
    return [gates[:, q * H:(q + 1) * H] for q in range(4)], c_out, hb[:, h_off:h_off + H], (cb[:, hc_off:hc_off + H] if with_hcopy else None)


@pytest.mark.parametrize("with_hcopy", [False, True], ids=["nocopy", "hcopy"])
@pytest.mark.parametrize("with_cprev", [False, True], ids=["c0", "cprev"])
@pytest.mark.parametrize("H", [10, 256])
def test_lstm_cell_fwd(dev, H, with_cprev, with_hcopy):
    B = 5
    gen = torch.Generator().manual_seed(77 + H)
    z, cp = rnd(gen, B, 4 * H) * 1.5, rnd(gen, B, H)
    (ri, rf, rg, ro), rc, rh = _cell_fwd_ref(z, cp if with_cprev else torch.zeros_like(cp))
    gates, c, h, hc = _run_cell_fwd(dev, z, cp, with_cprev, with_hcopy)
    for got, ref, nm in zip(gates, (ri, rf, rg, ro), "ifgo"):
        close(got, ref, 2e-5, "gate " + nm)
    close(c, rc, 2e-5, "c_out")
    close(h, rh, 2e-5, "h")
    if with_hcopy:
        close(hc, rh, 2e-5, "h_copy")
        assert torch.equal(hc.cpu(), h.cpu()), "h_copy differs from h"


def test_lstm_cell_fwd_saturating(dev):
    """Pre-activations of +-30 and +-100 among ordinary ones: sigm_ goes through expf(-x), which overflows to inf at x = -100; every
    result must be finite and within 2e-5 absolute of the fp64 value (all results are bounded by 1 resp. |c_prev| + 1)."""
    B, H = 5, 10
    gen = torch.Generator().manual_seed(99)
    z, cp = rnd(gen, B, 4 * H) * 1.5, rnd(gen, B, H)
    sat = torch.tensor([30.0, -30.0, 100.0, -100.0], dtype=torch.float64)
    for q in range(4):                                    # every gate quarter sees all four values, against varying neighbours
        for s in range(4):
            z[(q + s) % B, q * H + (3 * s + q) % H] = sat[s]
    z[4, 0:H], z[4, H:2 * H], z[4, 2 * H:3 * H], z[4, 3 * H:] = 100.0, 100.0, -100.0, 100.0       # a whole row saturated: c = cp - 1
    z[3, 0:H], z[3, H:2 * H], z[3, 3 * H:] = -100.0, -100.0, -100.0                               # ... and one shut: c = h = 0
    (ri, rf, rg, ro), rc, rh = _cell_fwd_ref(z, cp)
    gates, c, h, hc = _run_cell_fwd(dev, z, cp, True, True)
    for got, ref, nm in zip(gates, (ri, rf, rg, ro), "ifgo"):
        close_abs(got, ref, 2e-5, "saturating gate " + nm)
    close_abs(c, rc, 2e-5, "saturating c_out")
    close_abs(h, rh, 2e-5, "saturating h")
    close_abs(hc, rh, 2e-5, "saturating h_copy")


@pytest.mark.parametrize("with_cprev,with_dhb,with_dcnext", list(itertools.product([False, True], repeat=3)),
                         ids=lambda v: "y" if v else "n")
@pytest.mark.parametrize("H", [10, 256])
def test_lstm_cell_bwd(dev, H, with_cprev, with_dhb, with_dcnext):
    """d(pre-activations) and dc_prev against autograd through the fp64 cell formula."""
    from scrabble_gan_amd import ops
    B = 5
    gen = torch.Generator().manual_seed(177 + H)
    z = (rnd(gen, B, 4 * H) * 1.5).requires_grad_(True)
    cp = (rnd(gen, B, H) if with_cprev else torch.zeros(B, H, dtype=torch.float64)).requires_grad_(True)
    dh_a, dh_b, dc_next = rnd(gen, B, H), rnd(gen, B, H), rnd(gen, B, H)
    (ri, rf, rg, ro), rc, rh = _cell_fwd_ref(z, cp)
    dh = dh_a + (dh_b if with_dhb else 0.0)
    loss = (rh * dh).sum() + ((rc * dc_next).sum() if with_dcnext else 0.0)
    dz, dcp = torch.autograd.grad(loss, [z, cp])

    H4 = 4 * H
    ldz, g_off = 3 * H4, H4
    lda, a_off = 2 * H + 7, 3
    gb, g0, gm = _embed(torch.cat([ri, rf, rg, ro], dim=1).detach(), ldz, g_off, dev)
    ab, a0, am = _embed(dh_a, lda, a_off, dev)
    dc_prev = torch.full((B, H), SENTINEL, device=dev)
    c_t = g32(rc.detach(), dev)
    c_t0 = c_t.cpu().clone()
    ops.lstm_cell_bwd(gb, g_off, ldz, g32(cp.detach(), dev) if with_cprev else None, c_t, ab, a_off, lda,
                      g32(dh_b, dev) if with_dhb else None, g32(dc_next, dev) if with_dcnext else None, dc_prev, B, H)
    torch.cuda.synchronize()
    untouched_outside(gb, g0, gm, "gates")
    assert torch.equal(ab.cpu(), a0), "dh_a is an input"
    assert torch.equal(c_t.cpu(), c_t0), "c_t is an input"
    got = gb[:, g_off:g_off + H4]
    for q, nm in enumerate("ifgo"):
        ref = dz[:, q * H:(q + 1) * H]
        if nm == "f" and not with_cprev:                  # df = dc * c_prev * f (1 - f) with c_prev = 0: the scale is 0
            assert ref.abs().max().item() == 0.0 and got[:, q * H:(q + 1) * H].abs().max().item() == 0.0
        else:
            close(got[:, q * H:(q + 1) * H], ref, 5e-5, "dz " + nm)
    close(dc_prev, dcp, 5e-5, "dc_prev")


# ------------------------------------------------------------------------------------------------------------------------------
# 3. ops.gemm addressing, every transpose combination; the dense wrappers
# ------------------------------------------------------------------------------------------------------------------------------
TRANS = [(False, False), (True, False), (False, True), (True, True)]
_TRANS_IDS = ["nn", "tn", "nt", "tt"]


def _operands(gen, M, N, K, tA, tB):
    """-> A, B as stored (A [K,M] when transposed, B [N,K] when transposed) and op(A) @ op(B) in fp64."""
    A = rnd(gen, K, M) if tA else rnd(gen, M, K)
    B = rnd(gen, N, K) if tB else rnd(gen, K, N)
    return A, B, (A.t() if tA else A) @ (B.t() if tB else B)


@pytest.mark.parametrize("tA,tB", TRANS, ids=_TRANS_IDS)
@pytest.mark.parametrize("M,N,K,lda,A_off,ldc,out_off", [
    (5, 40, 10, 30, 10, 120, 40),         # the recurrent step's shape class: z_t += h_{t-1} U on strided rows
    (7, 32, 53, None, 0, 128, 64),        # the CBN dz scatter: dense A, a 32-column block of a 128-wide matrix
], ids=["recurrent", "cbn-scatter"])
def test_gemm_column_blocks(dev, tA, tB, M, N, K, lda, A_off, ldc, out_off):
    """A and out as column blocks of wider row-major matrices, beta = 1.  Outside A's block the buffer holds NaN (a read there poisons
    the result), outside out's block a sentinel that must stay bit-identical."""
    from scrabble_gan_amd import ops
    gen = torch.Generator().manual_seed(31 + M)
    A, Bm, prod = _operands(gen, M, N, K, tA, tB)
    C0 = rnd(gen, M, N)
    if lda is None:
        lda, Abuf = A.shape[1], g32(A, dev)
    else:
        host = torch.full((A.shape[0], lda), float("nan"), dtype=torch.float32)
        host[:, A_off:A_off + A.shape[1]] = A.float()
        Abuf = host.to(dev)
    out, out0, om = _embed(C0, ldc, out_off, dev)
    ret = ops.gemm(Abuf, g32(Bm, dev), M, N, K, lda, Bm.shape[1], transA=tA, transB=tB, out=out, ldc=ldc, beta=1.0, A_off=A_off,
                   out_off=out_off)
    assert ret is out
    torch.cuda.synchronize()
    untouched_outside(out, out0, om, "out")
    close(out[:, out_off:out_off + N], prod + C0.float().double(), 5e-5, "gemm block += ")


@pytest.mark.parametrize("tA,tB", TRANS, ids=_TRANS_IDS)
@pytest.mark.parametrize("M,N,K", [
    (37, 53, 70),         # ragged tiles in M, N and K
    (24, 1, 1024),        # N = 1, K = 1024: the logit head
    (1, 53, 512),         # M = 1
    (37, 53, 7),          # K below one 32-wide k-tile
])
def test_gemm_beta0_ignores_out(dev, tA, tB, M, N, K):
    """beta = 0 into an `out` full of NaN: the kernel must not read C.  With a bias."""
    from scrabble_gan_amd import ops
    gen = torch.Generator().manual_seed(57 + K)
    A, Bm, prod = _operands(gen, M, N, K, tA, tB)
    bias = rnd(gen, N)
    out = torch.full((M, N), float("nan"), device=dev)
    ops.gemm(g32(A, dev), g32(Bm, dev), M, N, K, A.shape[1], Bm.shape[1], transA=tA, transB=tB, bias=g32(bias, dev), out=out, beta=0.0)
    close(out, prod + bias, 2e-5, "gemm beta=0")
    fresh = ops.gemm(g32(A, dev), g32(Bm, dev), M, N, K, A.shape[1], Bm.shape[1], transA=tA, transB=tB, alpha=-0.75)
    assert fresh.shape == (M, N)
    close(fresh, -0.75 * prod, 2e-5, "gemm alpha, fresh out")


def test_dense_wrappers(dev):
    from scrabble_gan_amd import ops
    M, K, N = 24, 512, 53
    gen = torch.Generator().manual_seed(91)
    x, w, b, dy = rnd(gen, M, K), rnd(gen, K, N) / 16, rnd(gen, N), rnd(gen, M, N)
    xg, wg, dyg = g32(x, dev), g32(w, dev), g32(dy, dev)
    close(ops.dense_fwd(xg, wg, g32(b, dev)), x @ w + b, 2e-5, "dense_fwd bias")
    close(ops.dense_fwd(xg, wg), x @ w, 2e-5, "dense_fwd")
    close(ops.dense_bwd_input(dyg, wg), dy @ w.t(), 2e-5, "dense_bwd_input")
    ref = x.t() @ dy
    dw = g32(prefill_like(gen, ref), dev)
    dw0 = dw.cpu().double()
    ops.dense_bwd_weight(xg, dyg, dw)
    close(dw, dw0 + ref, 5e-5, "dense_bwd_weight +=")
    ops.dense_bwd_weight(xg, dyg, dw)
    close(dw, dw0 + 2 * ref, 5e-5, "dense_bwd_weight += twice")


# ------------------------------------------------------------------------------------------------------------------------------
# 4. elementwise entry points
# ------------------------------------------------------------------------------------------------------------------------------
ABOVE_GRID_CAP = 4096 * 256 + 777        # one element per thread, 4 096 workgroups of 256 at most: the grid-stride loop runs a second pass


@pytest.mark.parametrize("n", [1, 1000, ABOVE_GRID_CAP])
@pytest.mark.parametrize("alpha", [0.01, 0.3])
def test_leaky_relu(dev, alpha, n):
    from scrabble_gan_amd import ops
    gen = torch.Generator().manual_seed(5 + n % 1000)
    x = torch.randn(n, generator=gen)
    dy = torch.randn(n, generator=gen)
    zeros = torch.arange(0, n, 7)                         # exact zeros among the inputs (n = 1: the only element)
    x[zeros] = 0.0
    if n > 1:
        x[-1], x[n // 2 + 1] = -1.25, 2.5                 # the tail of the second pass holds a known pair
    xg, dyg = x.to(dev), dy.to(dev)
    y = ops.leaky_relu_fwd(xg, alpha)
    dx = ops.leaky_relu_bwd(dyg, xg, alpha)
    x64, dy64 = x.double(), dy.double()
    close(y, torch.where(x64 > 0, x64, alpha * x64), 2e-5, "leaky fwd")
    close(dx, torch.where(x64 > 0, dy64, alpha * dy64), 5e-5, "leaky bwd")
    yc, dxc = y.cpu(), dx.cpu()
    assert (yc[zeros] == 0).all(), "x = 0 -> y = 0"
    assert torch.equal(dxc[zeros], torch.tensor(alpha, dtype=torch.float32) * dy[zeros]), "x = 0 -> dx = alpha * dy"
    assert torch.equal(yc[x > 0], x[x > 0]) and torch.equal(dxc[x > 0], dy[x > 0]), "positive side is the identity"


@pytest.mark.parametrize("B,T,cols,per_sample", [
    (3, 5, 144, False), (3, 5, 144, True), (3, 5, 7, False), (3, 5, 7, True),
    (1461, 5, 144, True),                                 # 1 051 920 elements: above the grid cap, one mask row per sample
    (1461, 5, 144, False),
])
def test_mul_mask(dev, B, T, cols, per_sample):
    from scrabble_gan_amd import ops
    assert B < 100 or B * T * cols > 4096 * 256
    gen = torch.Generator().manual_seed(11 + cols)
    x = torch.randn(B, T, cols, generator=gen)
    if per_sample:                                        # rows_per_mask = T: mask [B, cols] shared by a sample's T rows
        mask = torch.randint(0, 2, (B, cols), generator=gen).float() * 2.0 + torch.randn(B, cols, generator=gen) * 0.125
        want = x * mask.unsqueeze(1)
        got = ops.mul_mask(x.to(dev), mask.to(dev), rows_per_mask=T)
    else:
        mask = torch.randn(B, T, cols, generator=gen)
        want = x * mask
        got = ops.mul_mask(x.to(dev), mask.to(dev))
    assert got.shape == x.shape
    assert torch.equal(got.cpu(), want), "mul_mask is one fp32 product per element"


def test_mul_mask_rejects_a_mask_of_the_wrong_size(dev):
    """Host-side check, nothing is launched."""
    from scrabble_gan_amd import ops
    x = torch.zeros(3, 5, 8, device=dev)
    for mask_shape, rpm in (((3, 8), 1), ((3, 5, 8), 5), ((2, 8), 5), ((3, 7), 5), ((15, 8), 4), ((3, 8), 0)):
        with pytest.raises(ValueError):
            ops.mul_mask(x, torch.ones(*mask_shape, device=dev), rows_per_mask=rpm)
    assert ops.mul_mask(x, torch.ones(3, 8, device=dev), rows_per_mask=5).shape == x.shape


@pytest.mark.parametrize("C", [4, 128])
def test_bias_add(dev, C):
    from scrabble_gan_amd import ops
    gen = torch.Generator().manual_seed(13 + C)
    y, b = rnd(gen, 3, 5, 7, C), rnd(gen, C)
    yg = g32(y, dev)
    ptr = yg.data_ptr()
    ret = ops.bias_add(yg, g32(b, dev))
    assert ret is yg and yg.data_ptr() == ptr, "bias_add works in place and returns its argument"
    close(yg, y + b, 2e-5, "bias_add")
    assert torch.equal(yg.cpu(), y.float() + b.float()), "one fp32 add per element"


def test_bias_add_rejects_channels_not_a_multiple_of_4(dev):
    """The C entry point returns SG_ERR_ARG before any launch."""
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import ScrabbleHipError
    y = torch.full((5, 6), 1.5, device=dev)
    with pytest.raises(ScrabbleHipError):
        ops.bias_add(y, torch.ones(6, device=dev))
    assert (y == 1.5).all()


def test_normalize_u8(dev):
    from scrabble_gan_amd import ops
    u8 = torch.arange(256, dtype=torch.uint8).repeat(3).view(3, 16, 16)
    assert u8.numel() % 16 == 0
    got = ops.normalize_u8(u8.to(dev))
    assert got.shape == u8.shape and got.dtype == torch.float32
    close_abs(got, (u8.double() - 127.5) / 127.5, 1e-6, "normalize_u8")


@pytest.mark.parametrize("mode", [0, 1], ids=["hinge", "not_saturating"])
def test_loss_terms(dev, mode):
    from scrabble_gan_amd import ops
    B = 37
    gen = torch.Generator().manual_seed(17 + mode)
    v = [rnd(gen, B, 1) * 1.5 for _ in range(5)]
    ref = (O.hinge if mode == 0 else O.not_saturating)(*v)
    got = ops.loss_terms(*[g32(t.reshape(-1), dev) for t in v], mode)
    assert got.shape == (7, B)
    for i, nm in enumerate(("d_loss", "d_loss_real", "d_loss_fake", "g_loss", "s_loss", "s_a", "s_b")):
        close(got[i], ref[i].reshape(-1), 1e-5, nm)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. spectral norm, forward and backward
# ------------------------------------------------------------------------------------------------------------------------------
SN_SHAPES = [
    (1024, 1),            # the discriminator's dense weight: N = 1
    (1, 1, 3, 5),         # K = 3 < the 4 rows of a workgroup
    (3, 3, 16, 40),       # K = 144, N = 40 (the shape of test_adam_rmsprop_spectral)
    (3, 3, 7, 300),       # K = 63, N > 256: the column kernels loop
    (1, 1, 64, 8),        # K = exactly one 64-row slab
    (130, 53),            # K one past a multiple of 64 plus ragged rows
]


def _sn_inputs(shape):
    gen = torch.Generator().manual_seed(23 + len(shape) + shape[-1])
    return gen, rnd(gen, *shape), rnd(gen, 1, shape[-1])


@pytest.mark.parametrize("power_iteration", [1, 3])
@pytest.mark.parametrize("shape", SN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spectral_norm_fwd(dev, shape, power_iteration):
    from scrabble_gan_amd import ops
    _, w, u = _sn_inputs(shape)
    wg = g32(w, dev)
    got = ops.spectral_norm(wg, g32(u.reshape(-1), dev), power_iteration)
    assert got.shape == w.shape
    close(got, O.spectral_norm(w, u, power_iteration), 2e-5, "spectral_norm")
    assert torch.equal(wg.cpu(), w.float()), "w is an input"


@pytest.mark.parametrize("shape", SN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_spectral_norm_bwd(dev, shape):
    """dw += d/dw <g, spectral_norm(w, u, 1)>: full autograd through the oracle (the reference applies no stop-gradient)."""
    from scrabble_gan_amd import ops
    gen, w, u = _sn_inputs(shape)
    g = rnd(gen, *shape)
    wr = w.clone().requires_grad_(True)
    (O.spectral_norm(wr, u, 1) * g).sum().backward()
    assert torch.isfinite(wr.grad).all()
    dw = g32(prefill_like(gen, wr.grad), dev)
    dw0 = dw.cpu().double()
    ops.spectral_norm_bwd(g32(w, dev), g32(u.reshape(-1), dev), g32(g, dev), dw)
    close(dw, dw0 + wr.grad, 5e-5, "prefill + spectral_norm_bwd")
