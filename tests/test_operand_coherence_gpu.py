"""Coherence of the low-precision operand copies (scrabble_gan_amd/operands.py) and of the filter cache (ops._PACK_CACHE) on the GPU.

Which bytes a convolution reads is decided by host bookkeeping: the bf16 twin, the e4m3 / e5m2 copies with their amax scalars, the
gradient bundles with their column sums, the kept Winograd transform of an activation, and the packed copies of a filter.  A
mistake there gives a finite result of the right size, computed from what the tensor held BEFORE its last write.  Every test
here makes a copy through a real consumer, changes the tensor (or the filter, or the scale) outright, runs the consumer again and
compares with the fp64 reference (tests/conv_refs.py) of the NEW values under the bound tests/test_conv_flags_gpu.py applies to
that route and direction.  Before anything runs on the GPU each case asserts on the CPU that the reference of the OLD values misses
the reference of the new ones by at least 100 bounds (`apart`): a stale copy cannot pass.

Writers of ops.py into a tensor the caller passed in (whole-file scan):
  * activation side, tested here (section 1): conv2d_fwd / conv2d_bwd_data / conv2d_transpose_fwd / conv2d_transpose_bwd_data (out=,
    with and without accum), add(out=), bias_add, relu_mask(out=), maxpool_bwd(out=, with and without accum), scale_add(out=),
    gemm(out=, beta 0 and 1; dense_bwd_weight goes through it), resample_u8(out=) with an fp32 kind;
  * parameter gradients and statistics -- conv2d_bwd_weight / conv2d_transpose_bwd_weight (dw, db), bias_grad, dot_accum,
    bn_bwd_reduce (dgamma_c, dbeta_c), bn_update_moving, filterbank_bwd (dtable, dz), spectral_norm_bwd, feature_moments,
    legibility_sums: accumulators that no convolution reads as an operand;
  * raw-pointer writers outside the contract, by their docstrings: adam_update / rmsprop_update (call weights_changed themselves),
    ema_update / swap_buffers (the caller does, section 2), lstm_cell_fwd / lstm_cell_bwd (GEMM-only tensors).

Where a reference needs the values a launch left behind (the writers' results, a chained conv's intermediate) they are read back
and the reference is evaluated on them, after the read-back itself was checked against its own fp64 reference: one bf16 ulp of an
intermediate that rounds the other way in fp64 is 2^-8 of one product, as large as the whole 5e-5 bound of the second conv."""
import functools
import gc
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import scrabble_oracle as O  # noqa: E402
from tests import conv_refs as R  # noqa: E402
from tests import lowp_refs as L  # noqa: E402
from tests.test_conv_flags_gpu import (EXACT, ROUTES, STRADDLE, W_STRADDLE, W_EXACT, T_SHAPES, case_data, check, family, g32, route, seed_of,  # noqa: E402
                                       t_data, wgrad_family)

WG_SHAPE = (3, 4, 24)           # the weight-grad shape of test_conv_flags_gpu.WGRAD_CASES with more than one sample (288 pixels: two tiles)
DB_TOL = 5e-5                   # the bias gradient sums fp32 values on every route (1e-4 in the Winograd domain)


def apart(name, old, new, tol):
    """The 100 x condition: max |ref(old) - ref(new)| >= 100 bounds of the check the new reference is used in."""
    gap, bnd = (old - new).abs().max().item(), R.bound(tol, new)
    assert gap >= 100.0 * bnd, "%s: the old and the new reference are only %.1f bounds apart -- the data is too tame" % (name, gap / bnd)


def rng(*key):
    return torch.Generator().manual_seed(seed_of(*key))


def copies_of(ops, t):
    """{id: tensor} of every copy the registry holds for t's storage (+ its kept transform); holding the tensors keeps the ids unique."""
    rec, out = ops._OPERANDS.find(t), []
    if rec is not None:
        out += [rec.bf16] if rec.bf16 is not None else []
        out += [rec.amax.pair] if rec.amax is not None else []
        out += [e.data for e in rec.fp8.values()] + [e.data for e in rec.grad_bf16.values()]
        out += [e.amax2 for e in rec.grad_fp8.values()] + list(rec.amax2.values())
    kept = ops._OPERANDS._kept.get(t.untyped_storage().data_ptr())
    if kept is not None:
        out.append(kept.V)
    return {id(c): c for c in out}


def n_copies(ops, t):
    rec = ops._OPERANDS.find(t)
    return (0 if rec is None else rec.count()) + (t.untyped_storage().data_ptr() in ops._OPERANDS._kept)


# ================================================================================================================================
# 1. every in-place writer invalidates every kind of copy
# ================================================================================================================================
class Kind:
    """One kind of copy: the tensor `old` [B,H,W,C] that acquires it, the consumer that makes and reads it, its fp64 reference."""
    route, split = None, 1
    ungated = ()                # results that do not depend on t (checked, but no stale copy could change them)

    def data(self):
        raise NotImplementedError

    @functools.lru_cache(maxsize=None)
    def d(self):
        return self.data()

    def ref(self, t):
        """{name: (conv term, tol)} for the tensor values t (fp64, CPU); cached by contents."""
        key = (type(self).__name__, hash(t.float().numpy().tobytes()))
        if key not in _REFS:
            _REFS[key] = self._ref(t)
        return _REFS[key]


_REFS = {}


class Twin(Kind):
    """a bf16 twin: a bf16-v2 forward reading t"""
    route, rounding, chans, relu = "bf16-v2", "bf16", (64, 64), False

    def data(self):
        (B, H, W), (K, N) = EXACT, self.chans
        cd = case_data(B, H, W, K, N, 3, True)
        return SimpleNamespace(old=cd.x, w=cd.w)

    def check_route(self, ops):
        (B, H, W), (K, N) = EXACT, self.chans
        assert family(ops, K, N, 3, True, H, W, B) == self.route

    def consume(self, ops, tg, dev, first):
        return {"y": ops.conv2d_fwd(tg, g32(self.d().w, dev), relu_in=self.relu)}

    def present(self, ops, tg):
        assert ops._twin_get(tg) is not None

    def _ref(self, t):
        return {"y": (R.fwd(t, self.d().w, relu_in=self.relu, rounding=self.rounding)[0], ROUTES[self.route]["tol"])}


class Fp8(Twin):
    """an e4m3 copy plus its amax: an fp8 forward reading t"""
    route, rounding, chans = "fp8", "fp8", (128, 256)

    def present(self, ops, tg):
        e = ops._OPERANDS.get_fp8(tg, self.relu)
        assert e is not None and e.amax.numel() == 1


class Fp8Relu(Fp8):
    relu = True


class Grad16(Kind):
    """the scaled and the unscaled gradient bundle with column sums: a bf16-v2 weight-grad with db and sample_scale, t as dy"""
    route, rounding, chans, k = "bf16-v2", "bf16", (64, 256), 3

    def data(self):
        (B, H, W), (Cin, Cout) = WG_SHAPE, self.chans
        g = rng(B, H, W, Cin, Cout, self.k, 41)
        return SimpleNamespace(x=R.rnd(g, B, H, W, Cin), old=R.rnd(g, B, H, W, Cout), sc=R.f32(torch.rand(B, generator=g, dtype=torch.float64) * 2 - 0.5))

    def check_route(self, ops):
        (B, H, W), (Cin, Cout) = WG_SHAPE, self.chans
        assert wgrad_family(ops, Cin, Cout, self.k, True, H, W) == self.route

    def consume(self, ops, tg, dev, first):
        d, out = self.d(), {}
        xg = g32(d.x, dev)
        for tag, sc in (("-scaled", self.scg), ("", None)):
            dw, db = torch.zeros(self.k, self.k, *self.chans, device=dev), torch.zeros(self.chans[1], device=dev)
            ops.conv2d_bwd_weight(xg, tg, dw, relu_in=True, db=db, sample_scale=sc)
            out["dw" + tag], out["db" + tag] = dw, db
        return out

    def present(self, ops, tg):
        for sc in (self.scg, None):
            e = ops._OPERANDS.get_grad_bf16(tg, sc)
            assert e is not None and e.colsum is not None

    def _ref(self, t):
        d, out = self.d(), {}
        for tag, sc in (("-scaled", d.sc), ("", None)):
            dw, db = R.wgrad(d.x, t, (self.k, self.k) + self.chans, True, sc, rounding=self.rounding)
            out["dw" + tag], out["db" + tag] = (dw, ROUTES[self.route]["wtol"]), (db, DB_TOL)
        return out


class Grad8(Grad16):
    """the same for the fp8 weight-grad (e5m2 bundle with its amax pair)"""
    route, rounding, chans, k = "fp8", "fp8", (256, 256), 1

    def present(self, ops, tg):
        for sc in (self.scg, None):
            e = ops._OPERANDS.get_grad_fp8(tg, sc)
            assert e is not None and e.colsum is not None and e.amax2.numel() == 2


class Amax2(Kind):
    """a stand-alone amax2 pair: avgpool2_bwd_operands in fp8 mode on t as dout, its handle feeding conv2's data-grad and weight-grad"""
    route, C = "fp8", 256

    def data(self):
        (B, H, W), C = WG_SHAPE, self.C
        g = rng(B, H, W, C, 43)
        return SimpleNamespace(old=R.rnd(g, B, H // 2, W // 2, C), x=R.rnd(g, B, H, W, C), sc=R.f32(torch.rand(B, generator=g, dtype=torch.float64) * 2 - 0.5),
                               w=R.f32(R.rnd(g, 1, 1, C, C) / math.sqrt(C)))

    def check_route(self, ops):
        (B, H, W), C = WG_SHAPE, self.C
        assert family(ops, C, C, 1, True, H, W, B) == "fp8" and wgrad_family(ops, C, C, 1, True, H, W) == "fp8"

    def consume(self, ops, tg, dev, first):
        d, (B, H, W), C = self.d(), WG_SHAPE, self.C
        h = ops.avgpool2_bwd_operands(tg, self.scg, True)
        assert ops.GHOST_NAN and ops._is_ghost(h) and torch.isnan(h).all()
        dw, db = torch.zeros(1, 1, C, C, device=dev), torch.zeros(C, device=dev)
        ops.conv2d_bwd_weight(g32(d.x, dev), h, dw, relu_in=True, db=db, sample_scale=self.scg)
        dx = ops.conv2d_bwd_data(h, g32(d.w, dev), (H, W))
        assert torch.isnan(h).all()
        return {"dx": dx, "dw": dw, "db": db}

    def present(self, ops, tg):
        assert ops._OPERANDS.get_amax2(tg, self.scg) is not None

    def _ref(self, t):
        d, (B, H, W), C = self.d(), WG_SHAPE, self.C
        dc = pool_bwd(t)
        dw, db = R.wgrad(d.x, dc, (1, 1, C, C), True, d.sc, rounding="fp8")
        return {"dx": (R.dgrad(dc, d.w, (H, W), rounding="fp8")[0], 5e-5), "dw": (dw, 5e-5), "db": (db, DB_TOL)}


def pool_bwd(dout):
    """avgpool2_bwd in fp64: 0.25 * dout replicated 2 x 2 (exact in fp32)."""
    return (0.25 * dout).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


class Kept(Kind):
    """a kept Winograd input transform: an f32 Winograd forward inside a step, then the Winograd weight-grad"""
    route, chans, split, ungated = "wino2", ROUTES["wino2"]["chans"][0], -1, ("db",)     # (t is the activation: db sums the gradient alone)

    def data(self):
        (B, H, W), (K, N) = W_STRADDLE, self.chans
        cd = case_data(B, H, W, K, N, 3, True)
        return SimpleNamespace(old=cd.x, w=cd.w, dy=R.rnd(rng(B, H, W, K, N, 47), B, H, W, N))

    def check_route(self, ops):
        (B, H, W), (K, N) = W_STRADDLE, self.chans
        assert ops.WINO_KEEP_V and ops._OPERANDS.keeping
        assert family(ops, K, N, 3, True, H, W, B) == "wino2" and wgrad_family(ops, K, N, 3, True, H, W) == "wino2"

    def consume(self, ops, tg, dev, first):
        d = self.d()
        if first:                           # (the second time the weight-grad alone: a forward launch would keep a fresh transform)
            ops.conv2d_fwd(tg, g32(d.w, dev), relu_in=True)
        dw, db = torch.zeros(3, 3, *self.chans, device=dev), torch.zeros(self.chans[1], device=dev)
        ops.conv2d_bwd_weight(tg, g32(d.dy, dev), dw, relu_in=True, db=db)
        return {"dw": dw, "db": db}

    def present(self, ops, tg):
        assert ops._OPERANDS.kept(tg, True, 2) is not None

    def _ref(self, t):
        d = self.d()
        dw, db = R.wgrad(t, d.dy, (3, 3) + self.chans, True, None, rounding="f32")
        return {"dw": (dw, ROUTES["wino2"]["wtol"]), "db": (db, 1e-4)}


KINDS = {"twin": Twin(), "fp8": Fp8(), "fp8-relu": Fp8Relu(), "grad-bf16": Grad16(), "grad-fp8": Grad8(), "amax2": Amax2(), "kept-wino": Kept()}


# ---- the writers: run(ops, tg, old, dev) stores into tg; predict(old) -> what it stores, in fp64 on the CPU (the low-precision conv
# writers round their source: within SLACK x max |old| of the prediction, checked on the read-back)
SLACK = 0.13            # 2 x 2^-4: an e4m3 source (relative half-ulp 2^-4) taken twice by the accumulating fp8 writer


def _eye(C, v, dev):
    return (v * torch.eye(C)).view(1, 1, C, C).to(dev).contiguous()


def _neg(old):
    return -old


def w_conv_fwd(accum):
    def run(ops, tg, old, dev):
        ops.conv2d_fwd(g32(old, dev), _eye(old.shape[3], -2.0 if accum else -1.0, dev), out=tg, accum=accum)
    return run, _neg


def w_dgrad(accum):
    def run(ops, tg, old, dev):
        ops.conv2d_bwd_data(g32(old, dev), _eye(old.shape[3], -2.0 if accum else -1.0, dev), tuple(old.shape[1:3]), out=tg, accum=accum)
    return run, _neg


def _even(old, v, accum):
    p = torch.zeros_like(old)
    p[:, ::2, ::2] = v * old[:, ::2, ::2]
    return old + p if accum else p


def w_t_fwd(accum):
    """1x1, stride 2: the even pixels get v x old, the tap-less parity classes 0 (+ old)."""
    v = -2.0 if accum else -1.0

    def run(ops, tg, old, dev):
        ops.conv2d_transpose_fwd(g32(old[:, ::2, ::2], dev), _eye(old.shape[3], v, dev), stride=(2, 2), out=tg, accum=accum)
    return run, lambda old: _even(old, v, accum)


def w_t_dgrad(accum):
    def run(ops, tg, old, dev):
        B, H, W, C = old.shape
        dy = torch.zeros(B, 2 * H, 2 * W, C, dtype=torch.float64)
        dy[:, ::2, ::2] = old
        ops.conv2d_transpose_bwd_data(g32(dy, dev), _eye(C, -2.0 if accum else -1.0, dev), stride=(2, 2), out=tg, accum=accum)
    return run, _neg


def w_add():
    def run(ops, tg, old, dev):
        ops.add(g32(-2.0 * old, dev), g32(old, dev), out=tg)
    return run, _neg


def _bias(old):
    C = old.shape[3]
    return R.f32(8.0 * old.abs().max() * (1.0 - 2.0 * (torch.arange(C, dtype=torch.float64) % 2)))


def w_bias_add():
    def run(ops, tg, old, dev):
        ops.bias_add(tg, g32(_bias(old), dev))
    return run, lambda old: R.f32(old + _bias(old))


def w_relu_mask():
    def run(ops, tg, old, dev):
        ops.relu_mask(g32(-old, dev), torch.ones(old.shape, device=dev), out=tg)
    return run, _neg


def _pool_src(old, accum):
    """-> (the pooled tensor xh whose 2 x 2 argmax positions the gradient goes to, its indices, the pooled gradient: -old (-2 old when
    accumulating) at those positions, so that they end up negated like the other writers' targets)."""
    B, H, W, C = old.shape
    xh = R.rnd(rng(*old.shape, 53), B, H, W, C)
    _, idx = F.max_pool2d(xh.permute(0, 3, 1, 2), 2, return_indices=True)
    at = old.permute(0, 3, 1, 2).flatten(2).gather(2, idx.flatten(2)).view(idx.shape)
    return xh, idx, ((-2.0 if accum else -1.0) * at).permute(0, 2, 3, 1).contiguous()


def w_maxpool_bwd(accum):
    def run(ops, tg, old, dev):
        xh, _, dyp = _pool_src(old, accum)
        _, idx = ops.maxpool_fwd(g32(xh, dev), 2, 2)
        ops.maxpool_bwd(g32(dyp, dev), idx, 2, 2, out=tg, accum=accum)

    def predict(old):
        xh, idx, dyp = _pool_src(old, accum)
        up = F.max_unpool2d(dyp.permute(0, 3, 1, 2).contiguous(), idx, 2).permute(0, 2, 3, 1)
        return R.f32(old + up) if accum else up
    return run, predict


def w_scale_add():
    def run(ops, tg, old, dev):
        ops.scale_add(g32(old, dev), g32(old, dev), torch.full((1,), -2.0, device=dev), out=tg)         # out = sigma o + x
    return run, _neg


def w_gemm(beta):
    def run(ops, tg, old, dev):
        C = old.shape[3]
        M = old.numel() // C
        ops.gemm(g32(old, dev).view(M, C), (-1.0 - beta) * torch.eye(C, device=dev), M, C, C, C, C, out=tg.view(M, C), beta=beta)
    return run, _neg


def _image(old):
    return np.random.default_rng(old.numel()).integers(0, 256, (old.numel() // 256, 256), dtype=np.uint8)


def w_resample():
    """An identity-sized linear resample (exact: tests/test_resample_gpu.py) of a random grey image over the whole of t."""
    def run(ops, tg, old, dev):
        img = _image(old)
        buf, offs, strides = ops.pack_gray_images([img])
        desc = ops.resample_desc(offs, strides, [img.shape], [0], img.shape[0], 256, 256)
        ops.resample_u8(buf.to(dev), desc, ops.RESAMPLE_LINEAR, ops.RESAMPLE_OUT_F32, out=tg.view(-1))
    return run, lambda old: ((torch.from_numpy(_image(old).astype(np.float64)) - 127.5) / 127.5).view(old.shape)


WRITERS = {"conv_fwd": w_conv_fwd(False), "conv_fwd+accum": w_conv_fwd(True), "conv_dgrad": w_dgrad(False), "conv_dgrad+accum": w_dgrad(True),
           "convT_fwd": w_t_fwd(False), "convT_fwd+accum": w_t_fwd(True), "convT_dgrad": w_t_dgrad(False), "convT_dgrad+accum": w_t_dgrad(True),
           "add": w_add(), "bias_add": w_bias_add(), "relu_mask": w_relu_mask(), "maxpool_bwd": w_maxpool_bwd(False),
           "maxpool_bwd+accum": w_maxpool_bwd(True), "scale_add": w_scale_add(), "gemm": w_gemm(0.0), "gemm+beta": w_gemm(1.0),
           "resample_u8": w_resample()}
REGISTERING = ("conv_fwd", "conv_dgrad")            # in fp8 mode their own epilogue records the amax of what they wrote


def gate(kind, old, new, label):
    K = KINDS[kind]
    r_old, r_new = K.ref(old), K.ref(new)
    for name, (term, tol) in r_new.items():
        if name not in K.ungated:
            apart("%s %s" % (label, name), r_old[name][0], term, tol)


def written(tg, pred, old, label):
    """The read-back of what the writer stored, checked against its prediction."""
    torch.cuda.synchronize()
    new = tg.detach().cpu().double()
    assert torch.isfinite(new).all(), label
    err = (new - pred).abs().max().item()
    assert err <= SLACK * old.abs().max().item(), "%s: the writer stored something else than predicted (max diff %.3e)" % (label, err)
    return new


@pytest.mark.parametrize("writer", list(WRITERS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_writer_invalidates_copy(dev, kind, writer):
    K, (run, predict) = KINDS[kind], WRITERS[writer]
    label = "%s after %s" % (kind, writer)
    old = K.d().old
    pred = predict(old)
    gate(kind, old, pred, label)
    with route(K.route, K.split) as ops:
        ops.new_step()
        K.check_route(ops)
        tg, plain, guarded = g32(old, dev), g32(old, dev), R.Guarded(old.shape, dev, old)
        K.scg = g32(getattr(K.d(), "sc", None), dev)           # ONE scale tensor for the case: the bundles are keyed by its address
        for sib in (plain, guarded.t):
            K.consume(ops, sib, dev, True)
        K.consume(ops, tg, dev, True)
        K.present(ops, tg)
        K.present(ops, plain)
        before, sib_before = copies_of(ops, tg), (n_copies(ops, plain), n_copies(ops, guarded.t))
        assert before and sib_before[0] == n_copies(ops, tg)
        run(ops, tg, old, dev)
        white = []                          # the white-box half, reported after the numeric half
        if ops._OPERANDS.find(tg) is not None and not (ops.CONV_DTYPE == "fp8" and writer.split("+")[0] in REGISTERING):
            white.append("the writer left a record behind")
        if set(copies_of(ops, tg)) & set(before):
            white.append("a copy of the old contents survived the write")
        if tg.untyped_storage().data_ptr() in ops._OPERANDS._kept:
            white.append("the kept transform survived the write")
        if (n_copies(ops, plain), n_copies(ops, guarded.t)) != sib_before:
            white.append("the write dropped a sibling's copies")
        new = written(tg, pred, old, label)
        got = K.consume(ops, tg, dev, False)
        torch.cuda.synchronize()
        guarded.check(label)
        if not torch.equal(new, pred):
            gate(kind, old, new, label)
        for name, (term, tol) in K.ref(new).items():
            check(got[name], term, term, tol, "%s %s" % (label, name))
        assert not white, "%s: %s" % (label, "; ".join(white))


@pytest.mark.parametrize("writer", ["add", "bias_add", "conv_fwd", "gemm+beta"])
def test_writer_into_a_batch_slice_drops_the_whole_twin(dev, writer):
    """The twin belongs to the whole storage; a writer that targets t[1:2] must drop it (and the next consumer convert t anew)."""
    (B, H, W), (K, N) = STRADDLE, (64, 64)
    cd = case_data(B, H, W, K, N, 3, True)
    run, predict = WRITERS[writer]
    old = cd.x
    pred = old.clone()
    pred[1:2] = predict(old[1:2])
    ref = lambda t: R.fwd(t, cd.w, rounding="bf16")[0]          # noqa: E731
    apart(writer, ref(old), ref(pred), 5e-5)
    with route("bf16-v2", 1) as ops:
        ops.new_step()
        assert family(ops, K, N, 3, True, H, W, B) == "bf16-v2"
        tg, wg = g32(old, dev), g32(cd.w, dev)
        ops.conv2d_fwd(tg, wg)
        twin = ops._twin_get(tg)
        assert twin is not None and ops._twin_get(tg[1:2]).data_ptr() == twin.data_ptr() + 2 * H * W * K
        run(ops, tg[1:2], old[1:2], dev)
        gone = ops._OPERANDS.find(tg) is None and ops._twin_get(tg[1:2]) is None
        new = written(tg, pred, old, writer)
        got = ops.conv2d_fwd(tg, wg)
        term = ref(new)
        apart(writer, ref(old), term, 5e-5)
        check(got, term, term, 5e-5, "whole tensor after %s into t[1:2]" % writer)
        assert gone, "%s into t[1:2] left the whole tensor's record behind" % writer


# ================================================================================================================================
# 2. the filter cache follows the weights
# ================================================================================================================================
def _f(route_, shp, ch, run, ref, tol, wshape, knob=False, t=False):
    return SimpleNamespace(route=route_, shp=shp, ch=ch, run=run, ref=ref, tol=tol, wshape=wshape, knob=knob, t=t)


def _fwd_kind(r, shp, ch):
    B, H, W = shp
    cd = lambda: case_data(B, H, W, ch[0], ch[1], 3, True)       # noqa: E731
    return _f(r, shp, ch, lambda ops, w, dev: ops.conv2d_fwd(g32(cd().x, dev), w), lambda w: R.fwd(cd().x, w, rounding=ROUTES[r]["rounding"])[0],
              ROUTES[r]["tol"], lambda: cd().w)


def _bwd_kind(r, shp, ch, knob=False):
    B, H, W = shp
    cd = lambda: case_data(B, H, W, ch[0], ch[1], 3, True)       # noqa: E731
    return _f(r, shp, ch, lambda ops, w, dev: ops.conv2d_bwd_data(g32(cd().dy, dev), w, (H, W)),
              lambda w: R.dgrad(cd().dy, w, (H, W), rounding=ROUTES[r]["rounding"])[0], ROUTES[r]["tol"], lambda: cd().wd, knob)


_T = T_SHAPES[2] + (3, 2, 2)             # (2, 4, 16, 128 -> 64), 3x3, stride 2: both directions on the bf16 kernels
FILTER_KINDS = {
    "fwd": _fwd_kind("bf16-v2", EXACT, (64, 64)),
    "bwd": _bwd_kind("bf16-v2", EXACT, (64, 64)),
    "fwd_f32t": _fwd_kind("f32-v2", EXACT, (32, 64)),
    "bwd_f32": _bwd_kind("f32-gen1", EXACT, (256, 128), knob=True),
    "wino_fwd2": _fwd_kind("wino2", W_EXACT, (32, 64)),
    "wino_bwd2": _bwd_kind("wino2", W_EXACT, (32, 64)),
    "wino_fwd4": _fwd_kind("wino4", (1, 4, 64), (32, 64)),
    "wino_bwd4": _bwd_kind("wino4", (1, 4, 64), (32, 64)),
    "t_fwd": _f("bf16", None, None, lambda ops, w, dev: ops.conv2d_transpose_fwd(g32(t_data(*_T).x, dev), w, stride=(2, 2)),
                lambda w: R.t_fwd(t_data(*_T).x, w, stride=(2, 2), rounding="bf16")[0], 5e-5, lambda: t_data(*_T).w, t=True),
    "t_bwd": _f("bf16", None, None, lambda ops, w, dev: ops.conv2d_transpose_bwd_data(g32(t_data(*_T).dy, dev), w, stride=(2, 2)),
                lambda w: R.t_dgrad(t_data(*_T).dy, w, (2, 2), rounding="bf16")[0], 5e-5, lambda: t_data(*_T).w, t=True),
    "fwd8": _fwd_kind("fp8", EXACT, (128, 256)),
    "bwd8": _bwd_kind("fp8", EXACT, (128, 256)),
}
PAD = 64                # floats in front of the filter inside its flat parameter buffer (nn.ParamStore: every filter is a view of one)


def _store(w, dev):
    flat = torch.zeros(PAD + w.numel(), device=dev)
    flat[PAD:].copy_(w.float().view(-1))
    return flat, flat[PAD:].view(w.shape)


def _like_oracle(wg, want, w, decay, what):
    """The optimizer kernels against the oracle's fp64 update: 1e-6 of max |w| (tests/test_ops_gpu.py) + what the fp32 value of the
    decay does to a step of this size -- 1 - decay carries a relative error of up to 2^-24 / (1 - decay), its root (the step's
    denominator from a fresh state) half of that; at the learning rates of test_ops_gpu.py this is far below its 1e-6."""
    torch.cuda.synchronize()
    got = wg.detach().cpu().double()
    bnd = 1e-6 * want.abs().max().item() + 2.0 ** -25 / (1.0 - decay) * (want - w).abs().max().item()
    assert (got - want).abs().max().item() <= bnd, what
    return got


def c_adam(ops, flat, wg, w, dev):
    g = R.rnd(rng(w.numel(), 61), *w.shape)
    P = {"w": w.clone()}
    O.adam_update(P, {"w": g}, {}, 1.0, 0.5, 0.999)             # one step of size ~1 per weight from a fresh state
    yield P["w"]
    ops.adam_update(wg, g32(g, dev), torch.zeros_like(wg), torch.zeros_like(wg), 1.0 * math.sqrt(1 - 0.999) / (1 - 0.5), 0.5, 0.999)
    yield _like_oracle(wg, P["w"], w, 0.999, "adam_update")


def c_rmsprop(ops, flat, wg, w, dev):
    g = R.rnd(rng(w.numel(), 67), *w.shape)
    P = {"w": w.clone()}
    O.rmsprop_update(P, {"w": g}, {}, 1.0)
    yield P["w"]
    ops.rmsprop_update(wg, g32(g, dev), torch.zeros_like(wg), 1.0)
    yield _like_oracle(wg, P["w"], w, 0.9, "rmsprop_update")


def c_inplace(ops, flat, wg, w, dev):
    yield -w
    wg.neg_()
    yield -w


def c_flat_copy(ops, flat, wg, w, dev):
    """nn.ParamStore loads a checkpoint into the FLAT buffer: the filter views share its version counter."""
    new = R.f32(8.0 * w.flip(0, 1))
    yield new
    v = wg._version
    flat.copy_(torch.cat([torch.zeros(PAD, dtype=torch.float64), new.reshape(-1)]).float())
    assert wg._version != v, "a view no longer shares the version counter of its base"
    yield new


def c_swap(ops, flat, wg, w, dev):
    """averaging.py: swap_buffers, then weights_changed()."""
    new = R.f32(-8.0 * w)
    yield new
    other = torch.cat([torch.zeros(PAD, dtype=torch.float64), new.reshape(-1)]).float().to(dev)
    ops.swap_buffers(flat, other)
    ops.weights_changed()
    yield new


def c_dtype(ops, flat, wg, w, dev):
    """set_conv_dtype to another mode and back, the filter rewritten through a raw pointer in between (ema_update with 1 - decay = 1
    makes it bitwise the source, and leaves the cache to its caller)."""
    new = R.f32(-8.0 * w)
    yield new
    mode = ops.CONV_DTYPE
    ops.set_conv_dtype("f32" if mode != "f32" else "bf16")
    assert not ops._PACK_CACHE and ops._OPERANDS.count() == 0
    ops.ema_update(flat, torch.cat([torch.zeros(PAD, dtype=torch.float64), new.reshape(-1)]).float().to(dev), 1.0)
    ops.set_conv_dtype(mode)
    assert not ops._PACK_CACHE and ops._OPERANDS.count() == 0
    yield new


CHANGES = {"adam_update": c_adam, "rmsprop_update": c_rmsprop, "torch-inplace": c_inplace, "flat-copy_": c_flat_copy,
           "swap_buffers+weights_changed": c_swap, "set_conv_dtype-roundtrip": c_dtype}


def _cache_kinds(ops):
    return {k[2] for k in ops._PACK_CACHE}


@pytest.mark.parametrize("change", list(CHANGES))
@pytest.mark.parametrize("kind", list(FILTER_KINDS))
def test_filter_cache_follows_the_weights(dev, kind, change):
    fk = FILTER_KINDS[kind]
    w = fk.wshape()
    label = "%s after %s" % (kind, change)
    with route(fk.route, 1) as ops:
        saved = ops.TRANSPOSED_DGRAD_FILTERS
        try:
            ops.TRANSPOSED_DGRAD_FILTERS = fk.knob
            ops.new_step()
            if not fk.t:
                B, H, W = fk.shp
                assert family(ops, fk.ch[0], fk.ch[1], 3, True, H, W, B) == fk.route
            flat, wg = _store(w, dev)
            steps = CHANGES[change](ops, flat, wg, w, dev)
            ref_old, ref_pred = fk.ref(w), fk.ref(next(steps))
            apart(label, ref_old, ref_pred, fk.tol)
            first = fk.run(ops, wg, dev)
            check(first, ref_old, ref_old, fk.tol, label + " (before)")
            assert kind in _cache_kinds(ops), "%s: the conv did not read the %s copy (%s)" % (label, kind, sorted(_cache_kinds(ops)))
            new = next(steps)
            ops.new_step()                  # (the activation's copies are not under test here)
            got = fk.run(ops, wg, dev)
            term = fk.ref(new)
            apart(label, ref_old, term, fk.tol)
            check(got, term, term, fk.tol, label)
        finally:
            ops.TRANSPOSED_DGRAD_FILTERS = saved
            ops.weights_changed()


@pytest.mark.parametrize("r", ["wino2", "wino4"])
def test_wino_filter_is_rebuilt_from_a_rebuilt_transpose(dev, r):
    """wino_fwd* is derived from the fwd_f32t entry of the same cache: after weights_changed() both are new tensors of the new filter."""
    fk = FILTER_KINDS["wino_fwd" + r[-1]]
    w = fk.wshape()
    new = R.f32(-8.0 * w.flip(3))
    apart(r, fk.ref(w), fk.ref(new), fk.tol)
    with route(r, 1) as ops:
        flat, wg = _store(w, dev)
        fk.run(ops, wg, dev)
        old = {k[2]: e[1] for k, e in ops._PACK_CACHE.items()}
        assert set(old) == {"fwd_f32t", "wino_fwd" + r[-1]}
        ops.swap_buffers(wg, g32(new, dev))
        ops.weights_changed()
        assert not ops._PACK_CACHE
        got = fk.run(ops, wg, dev)
        now = {k[2]: e[1] for k, e in ops._PACK_CACHE.items()}
        assert set(now) == set(old) and all(now[k] is not old[k] for k in now)
        assert torch.equal(now["fwd_f32t"].cpu(), new.float().permute(0, 1, 3, 2).contiguous())
        term = fk.ref(new)
        check(got, term, term, fk.tol, r + " forward after swap_buffers + weights_changed")


# ================================================================================================================================
# 3. chains: what one launch leaves for the next
# ================================================================================================================================
CHAIN = {"bf16": ("bf16-v2", (64, 64)), "fp8": ("fp8", (128, 256))}             # mode -> (route, conv1 channels); conv2 is N -> N


def _chain_data(mode, shp):
    r, (K, N) = CHAIN[mode]
    B, H, W = shp
    cd = case_data(B, H, W, K, N, 3, True)
    g = rng(B, H, W, N, N, 71)
    return r, cd, R.f32(R.rnd(g, 3, 3, N, N) / math.sqrt(9 * N)), R.rnd(g, B, H, W, N)


def _rd(t):
    torch.cuda.synchronize()
    return t.detach().cpu().double()


def _bits(a, b):
    return torch.equal(a.detach().cpu().view(torch.int32), b.detach().cpu().view(torch.int32))


@pytest.mark.parametrize("shp", [EXACT, STRADDLE], ids=["exact", "straddle"])
@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_two_conv_chain_warm_equals_cold(dev, mode, shp):
    """conv2d_fwd(want16=True) -> conv reading the result: the epilogue's twin / amax (warm) against a conversion sweep (cold)."""
    r, cd, w2, _ = _chain_data(mode, shp)
    B, H, W = shp
    cfg = ROUTES[r]
    y_ref = R.fwd(cd.x, cd.w, cd.b1, rounding=cfg["rounding"])[1]
    z_composed = R.fwd(R.f32(y_ref), w2, relu_in=True, rounding=cfg["rounding"])[0]
    with route(r, 1) as ops:
        N = cd.w.shape[3]
        assert family(ops, cd.w.shape[2], N, 3, True, H, W, B) == r and family(ops, N, N, 3, True, H, W, B) == r
        xg, w1g, b1g, w2g = g32(cd.x, dev), g32(cd.w, dev), g32(cd.b1, dev), g32(w2, dev)
        ops.new_step()
        y = ops.conv2d_fwd(xg, w1g, b1g, want16=True)
        assert ops._twin_get(y) is not None and (mode == "bf16" or ops._amax_get(y) is not None)
        z_warm = ops.conv2d_fwd(y, w2g, relu_in=True)
        if mode == "fp8":
            assert ops._OPERANDS.get_fp8(y, True).amax.data_ptr() == ops._amax_get(y).data_ptr(), "the epilogue's amax was not reused"
        ops.new_step()
        y2 = ops.conv2d_fwd(xg, w1g, b1g, want16=True)
        ops.new_step()
        assert ops._OPERANDS.find(y2) is None
        z_cold = ops.conv2d_fwd(y2, w2g, relu_in=True)
        assert _bits(y, y2) and _bits(z_warm, z_cold), "warm and cold differ"
        check(y, y_ref, y_ref, cfg["tol"], "%s chain conv1" % mode)
        term = R.fwd(_rd(y), w2, relu_in=True, rounding=cfg["rounding"])[0]
        check(z_warm, term, term, cfg["tol"], "%s chain conv2 on conv1's checked result" % mode)
        check(z_warm, z_composed, z_composed, cfg["exact"], "%s chain conv2 vs the composed reference" % mode)


def test_dgrad_to_wgrad_chain_fp8_warm_equals_cold(dev):
    """conv2d_bwd_data(want16=True, amax_scale=s) -> conv2d_bwd_weight(sample_scale=s): the epilogue's amax pair against sg_amax2_f32."""
    (B, H, W), (K, N) = WG_SHAPE, (128, 256)
    cd = case_data(B, H, W, K, N, 3, True)
    g = rng(B, H, W, N, 73)
    x2, s = R.rnd(g, B, H, W, N), R.f32(torch.rand(B, generator=g, dtype=torch.float64) * 2 - 0.5)
    dx_ref = R.dgrad(cd.dy, cd.wd, (H, W), rounding="fp8")[0]
    with route("fp8", 1) as ops:
        assert family(ops, K, N, 3, True, H, W, B) == "fp8" and wgrad_family(ops, N, N, 1, True, H, W) == "fp8"
        dyg, wdg, x2g, sg = g32(cd.dy, dev), g32(cd.wd, dev), g32(x2, dev), g32(s, dev)
        res = []
        for cold in (False, True):
            ops.new_step()
            dx = ops.conv2d_bwd_data(dyg, wdg, (H, W), want16=True, amax_scale=sg)
            assert ops._amax_get(dx, sg, need_scaled=True) is not None
            if cold:
                ops.new_step()
            dw = torch.zeros(1, 1, N, N, device=dev)
            ops.conv2d_bwd_weight(x2g, dx, dw, relu_in=True, sample_scale=sg)
            res.append((dx, dw))
        assert _bits(res[0][0], res[1][0]) and _bits(res[0][1], res[1][1]), "warm and cold differ"
        check(res[0][0], dx_ref, dx_ref, 5e-5, "dgrad -> wgrad chain dx")
        term = R.wgrad(x2, _rd(res[0][0]), (1, 1, N, N), True, s, rounding="fp8")[0]
        check(res[0][1], term, term, 5e-5, "dgrad -> wgrad chain dW")


@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_batch_slices_read_their_part(dev, mode):
    """The chunked backward of net_architecture: y[:B1] and y[B1:] of a registered tensor; in fp8 mode each slice takes its own amax."""
    r, cd, w2, _ = _chain_data(mode, STRADDLE)
    B, H, W = STRADDLE
    cfg = ROUTES[r]
    with route(r, 1) as ops:
        N = cd.w.shape[3]
        ops.new_step()
        y = ops.conv2d_fwd(g32(cd.x, dev), g32(cd.w, dev), g32(cd.b1, dev), want16=True)
        twin, w2g = ops._twin_get(y), g32(w2, dev)
        y64 = _rd(y)
        y_ref = R.fwd(cd.x, cd.w, cd.b1, rounding=cfg["rounding"])[1]
        check(y, y_ref, y_ref, cfg["tol"], "%s slices conv1" % mode)
        lo = R.fwd(y64[:2], w2, relu_in=True, rounding=cfg["rounding"])[0]
        hi = R.fwd(y64[2:], w2, relu_in=True, rounding=cfg["rounding"])[0]
        whole = R.fwd(y64, w2, relu_in=True, rounding=cfg["rounding"])[0]
        if mode == "fp8":                   # the slices' own scales matter: the slice references differ from the whole tensor's
            assert y64[:2].abs().max() != y64[2:].abs().max()
        for name, sl, term in (("y[:2]", y[:2], lo), ("y[2:]", y[2:], hi)):
            got = ops.conv2d_fwd(sl, w2g, relu_in=True)
            if mode == "bf16":
                assert ops._twin_get(sl).data_ptr() == twin.data_ptr() + 2 * sl.storage_offset()
            else:
                e = ops._OPERANDS.get_fp8(sl, True)
                assert e is not None and e.amax.item() == sl.abs().max().item(), name + ": a non-ghost slice takes its own amax"
            check(got, term, term, cfg["tol"], "%s %s" % (mode, name))
        got = ops.conv2d_fwd(y, w2g, relu_in=True)
        check(got, whole, whole, cfg["tol"], "%s whole tensor beside its slices" % mode)


@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_operand_only_result_feeds_its_consumers(dev, mode):
    """want16="only": conv2's forward, its weight-grad (the result as activation operand) and a batch slice of it read the bf16 copy
    (fp8 mode: e4m3 cut from the bf16 values with the whole tensor's recorded amax); the fp32 handle stays NaN."""
    r, cd, w2, dz = _chain_data(mode, STRADDLE)
    B, H, W = STRADDLE
    cfg = ROUTES[r]
    y_ref = R.fwd(cd.x, cd.w, cd.b1, rounding=cfg["rounding"])[1]
    with route(r, 1) as ops:
        N = cd.w.shape[3]
        assert ops.GHOST_NAN
        ops.OPERAND_ONLY_MIN_TILES = 0
        assert ops.operand_only_ok(B, H, W, N) and wgrad_family(ops, N, N, 3, True, H, W) == r
        ops.new_step()
        h = ops.conv2d_fwd(g32(cd.x, dev), g32(cd.w, dev), g32(cd.b1, dev), want16="only")
        assert ops._is_ghost(h)
        t16 = ops._twin_get(h)
        y16 = _rd(t16.float())
        bnd = R.bound(cfg["tol"], y_ref) + 2.0 ** -8 * y_ref.abs().max().item()         # the fp32 result's bound + half a bf16 ulp (8-bit significand)
        assert (y16 - y_ref).abs().max().item() <= bnd, "the bf16 copy of the operand-only result"
        bits16 = t16.view(torch.int16).cpu().numpy().view(np.uint16)

        def operand(sl):
            """relu(y) as the consumers of the slice `sl` of the batch read it, dequantised."""
            if mode == "bf16":
                return torch.relu(y16[sl])
            amax = ops._OPERANDS.storage_amax(h)[0].item()
            assert abs(amax - y_ref.abs().max().item()) <= bnd
            codes = L.cvt_fp8_bf16(bits16[sl.start or 0:sl.stop], np.float32(amax), relu=True)
            e = ops._OPERANDS.get_fp8(h[sl], True)
            assert e is not None and np.array_equal(e.data.cpu().numpy().ravel(), codes.ravel()), "the e4m3 copy cut from the bf16 values"
            return torch.from_numpy(L.e4m3fn_bits_to_f64(codes)).view(y16[sl].shape) * (float(np.float32(amax)) / 448.0)

        w2q = R.r16(w2) if mode == "bf16" else R.q8(w2)
        z = ops.conv2d_fwd(h, g32(w2, dev), relu_in=True)
        term = O.conv2d(operand(slice(None)), w2q, None, padding="same")
        check(z, term, term, cfg["tol"], "%s operand-only -> forward" % mode)
        for name, sl in (("whole", slice(None)), ("slice", slice(1, B))):
            dw = torch.zeros(3, 3, N, N, device=dev)
            ops.conv2d_bwd_weight(h[sl], g32(dz[sl], dev), dw, relu_in=True)
            a = operand(sl)
            wz = torch.zeros(3, 3, N, N, dtype=torch.float64, requires_grad=True)
            O.conv2d(a, wz, None, padding="same").backward(R.r16(dz[sl]) if mode == "bf16" else R.q5(dz[sl]))
            check(dw, wz.grad, wz.grad, cfg["wtol"], "%s operand-only -> weight-grad (%s)" % (mode, name))
        for f in (lambda: ops.add(h, h), lambda: ops.relu_mask(h, h), lambda: ops.bn_stats_sums(h)):
            with pytest.raises(RuntimeError, match="operand-only"):
                f()
        torch.cuda.synchronize()
        assert torch.isnan(h).all(), "the fp32 handle of an operand-only result was written"


@pytest.mark.parametrize("want_dw", [True, False], ids=["dw", "nodw"])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "wscale"])
@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_pooled_gradient_handle(dev, mode, scaled, want_dw):
    """avgpool2_bwd_operands feeds conv2's weight-grad (with db) and data-grad and the shortcut's weight-grad: bitwise what
    avgpool2_bwd + the fp32-tensor path give (the same kernels on the same operand bytes), and within the route's bounds of fp64."""
    r, C = ("bf16-v2", 64) if mode == "bf16" else ("fp8", 256)
    B, H, W = STRADDLE[0], 2 * STRADDLE[1], 2 * STRADDLE[2]          # the pooled gradient (the shortcut's weight-grad operand) has the STRADDLE shape
    cfg = ROUTES[r]
    g = rng(B, H, W, C, 79)
    dout, x, xs = R.rnd(g, B, H // 2, W // 2, C), R.rnd(g, B, H, W, C), R.rnd(g, B, H // 2, W // 2, C)
    w2, sc = R.f32(R.rnd(g, 3, 3, C, C) / math.sqrt(9 * C)), R.f32(torch.rand(B, generator=g, dtype=torch.float64) * 2 - 0.5) if scaled else None
    dc = pool_bwd(dout)
    with route(r, 1) as ops:
        assert ops.GHOST_NAN and family(ops, C, C, 3, True, H, W, B) == r and wgrad_family(ops, C, C, 3, True, H, W) == r
        doutg, xg, xsg, w2g, scg = g32(dout, dev), g32(x, dev), g32(xs, dev), g32(w2, dev), g32(sc, dev)
        res = []
        for handle in (True, False):
            ops.new_step()
            d = ops.avgpool2_bwd_operands(doutg, scg, want_dw) if handle else ops.avgpool2_bwd(doutg)
            assert ops._is_ghost(d) == handle and bool(torch.isnan(d).all()) == handle
            out = {}
            if want_dw:
                out["dw"], out["db"] = torch.zeros(3, 3, C, C, device=dev), torch.zeros(C, device=dev)
                ops.conv2d_bwd_weight(xg, d, out["dw"], relu_in=True, db=out["db"], sample_scale=scg)
                out["dws"], out["dbs"] = torch.zeros(1, 1, C, C, device=dev), torch.zeros(C, device=dev)
                ops.conv2d_bwd_weight(xsg, doutg, out["dws"], db=out["dbs"], sample_scale=scg)
            out["dx"] = ops.conv2d_bwd_data(d, w2g, (H, W), mask=xg)
            torch.cuda.synchronize()
            assert bool(torch.isnan(d).all()) == handle
            if mode == "bf16":              # the operand bytes both launches read
                out["bytes"] = [ops._twin_get(d)] + ([ops._OPERANDS.get_grad_bf16(d, scg).data] if want_dw else [])
            else:
                e4, e5 = ops._OPERANDS.get_fp8(d, False), ops._OPERANDS.get_grad_fp8(d, scg) if want_dw else None
                out["bytes"] = [e4.data, e4.amax] + ([e5.data, e5.amax] if want_dw else [])
            res.append(out)
        for a, b in zip(res[0]["bytes"], res[1]["bytes"]):
            assert a.dtype == b.dtype and torch.equal(a.view(-1).view(torch.uint8), b.view(-1).view(torch.uint8)), \
                "an operand copy made through the handle differs from the fp32-tensor path's"
        assert _bits(res[0]["dx"], res[1]["dx"]), "dx through the handle differs from the fp32-tensor path"      # (one adder per address at split 1;
        # the weight-grads cut these 1056 pixels into chunks that meet in float atomics: the same operand bytes, compared with fp64 below)
        name = "pooled gradient %s %s" % (mode, "wscale" if scaled else "plain")
        keep = x > 0
        term = R.dgrad(dc, w2, (H, W), rounding=cfg["rounding"])[0]
        check(res[0]["dx"], term, term * keep, cfg["tol"], name + " dx", keep=keep)
        if want_dw:
            dw, db = R.wgrad(x, dc, (3, 3, C, C), True, sc, rounding=cfg["rounding"])
            dws, dbs = R.wgrad(xs, dout, (1, 1, C, C), False, sc, rounding=cfg["rounding"])
            for k, term, tol in (("dw", dw, cfg["wtol"]), ("db", db, DB_TOL), ("dws", dws, cfg["wtol"]), ("dbs", dbs, DB_TOL)):
                check(res[0][k], term, term, tol, "%s %s" % (name, k))
            torch.testing.assert_close(db, dbs, rtol=1e-12, atol=1e-12)         # (conv2 and the shortcut share dout's column sums)


@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_two_scales_on_one_gradient(dev, mode):
    r, (Cin, Cout), k = ("bf16-v2", (64, 256), 3) if mode == "bf16" else ("fp8", (256, 256), 1)
    B, H, W = WG_SHAPE
    cfg = ROUTES[r]
    g = rng(B, H, W, Cin, Cout, 83)
    x, dy = R.rnd(g, B, H, W, Cin), R.rnd(g, B, H, W, Cout)
    s1 = R.f32(torch.rand(B, generator=g, dtype=torch.float64) + 0.5)
    s2 = R.f32(-8.0 * s1.flip(0))
    wd = R.f32(R.rnd(g, k, k, Cin, Cout) / math.sqrt(k * k * Cout))
    refs = [R.wgrad(x, dy, (k, k, Cin, Cout), True, s, rounding=cfg["rounding"]) for s in (s1, s2, None)]
    for i in range(3):
        for j in range(3):
            if i != j:
                apart("scale %d vs %d dW" % (i, j), refs[i][0], refs[j][0], cfg["wtol"])
                apart("scale %d vs %d db" % (i, j), refs[i][1], refs[j][1], DB_TOL)
    with route(r, 1) as ops:
        assert wgrad_family(ops, Cin, Cout, k, True, H, W) == r and family(ops, Cout, Cin, k, True, H, W, B) == r
        ops.new_step()
        xg, dyg = g32(x, dev), g32(dy, dev)
        for i, s in enumerate((s1, s2, None)):
            dw, db = torch.zeros(k, k, Cin, Cout, device=dev), torch.zeros(Cout, device=dev)
            ops.conv2d_bwd_weight(xg, dyg, dw, relu_in=True, db=db, sample_scale=g32(s, dev))
            check(dw, refs[i][0], refs[i][0], cfg["wtol"], "%s two scales: dW of call %d" % (mode, i))
            check(db, refs[i][1], refs[i][1], DB_TOL, "%s two scales: db of call %d" % (mode, i))
        plain = ops._twin_get(dyg) if mode == "bf16" else ops._OPERANDS.get_fp8(dyg, False)
        assert plain is not None, "the first call left no unscaled copy for the data-grad"
        n = ops._OPERANDS.find(dyg).count()
        dx = ops.conv2d_bwd_data(dyg, g32(wd, dev), (H, W))
        assert ops._OPERANDS.find(dyg).count() == n, "the data-grad converted the gradient again"
        term = R.dgrad(dy, wd, (H, W), rounding=cfg["rounding"])[0]
        check(dx, term, term, cfg["tol"], "%s two scales: the later data-grad" % mode)


def test_recycled_scale_address_fp8(dev):
    """The amax pair of a data-grad result is matched by the address of its scale.  If that scale is freed and the allocator hands its
    address to a new [B] tensor with 8 x larger factors, the weight-grad must still quantise with ITS amax (the e5m2 operand would
    clamp at 57344 otherwise).  The registry keeps the scale alive, so the address is not handed out again and the case skips; the
    registry-level twin of it (tests/test_operands_cpu.py::test_amax_entry_keeps_its_scale_alive) always runs."""
    (B, H, W), (K, N) = WG_SHAPE, (128, 256)
    cd = case_data(B, H, W, K, N, 3, True)
    g = rng(B, H, W, N, 89)
    x2, s = R.rnd(g, B, H, W, N), R.f32(torch.rand(B, generator=g, dtype=torch.float64) + 0.5)
    dx_ref = R.dgrad(cd.dy, cd.wd, (H, W), rounding="fp8")[0]
    refs = [R.wgrad(x2, R.f32(dx_ref), (1, 1, N, N), True, f * s, rounding="fp8")[0] for f in (1.0, 8.0)]
    apart("s1 vs s2", refs[0], refs[1], 5e-5)
    with route("fp8", 1) as ops:
        ops.new_step()
        s1 = g32(s, dev)
        addr = s1.data_ptr()
        dx = ops.conv2d_bwd_data(g32(cd.dy, dev), g32(cd.wd, dev), (H, W), want16=True, amax_scale=s1)
        torch.cuda.synchronize()
        del s1
        gc.collect()
        s2 = (8.0 * s).float().to(dev)
        if s2.data_ptr() != addr:
            pytest.skip("the allocator did not hand the freed scale's address out again (the amax entry keeps its scale alive)")
        dw = torch.zeros(1, 1, N, N, device=dev)
        ops.conv2d_bwd_weight(g32(x2, dev), dx, dw, relu_in=True, sample_scale=s2)
        term = R.wgrad(x2, _rd(dx), (1, 1, N, N), True, 8.0 * s, rounding="fp8")[0]
        check(dw, term, term, 5e-5, "weight-grad with a scale at a recycled address")


@pytest.mark.parametrize("change", ["deterministic", "f32"])
def test_mode_change_between_forward_and_backward(dev, change):
    """A ghost made in bf16 mode whose consumer runs after the mode flags changed: the ghost error, not a read of the poison."""
    r, cd, w2, dz = _chain_data("bf16", STRADDLE)
    B, H, W = STRADDLE
    with route(r, 1) as ops:
        assert ops.GHOST_NAN
        ops.OPERAND_ONLY_MIN_TILES = 0
        ops.new_step()
        h = ops.conv2d_fwd(g32(cd.x, dev), g32(cd.w, dev), g32(cd.b1, dev), want16="only")
        assert ops._is_ghost(h) and ops._PACK_CACHE
        dw = torch.zeros(3, 3, 64, 64, device=dev)
        try:
            if change == "deterministic":
                ops.set_deterministic(True)
            else:
                ops.set_conv_dtype("f32")
                assert not ops._PACK_CACHE, "set_conv_dtype left packed filters behind"
                assert ops._OPERANDS.count() == 1 and ops._is_ghost(h) and ops._twin_get(h) is None, "only the ghost mark outlives set_conv_dtype"
            with pytest.raises(RuntimeError, match="operand-only"):
                ops.conv2d_bwd_weight(h, g32(dz, dev), dw, relu_in=True)
            if change == "f32":             # (in deterministic bf16 mode the forward conv still reads the bf16 copy)
                with pytest.raises(RuntimeError, match="operand-only"):
                    ops.conv2d_fwd(h, g32(w2, dev), relu_in=True)
        finally:
            ops.set_deterministic(False)
        torch.cuda.synchronize()
        assert not dw.any() and torch.isnan(h).all()
        ops.new_step()
        assert ops._OPERANDS.count() == 0 and not ops._is_ghost(h)
