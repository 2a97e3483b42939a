"""The averaged generator on the GPU: the three sweeps of csrc/averaging.hip against numpy, WeightAverage / applied() /
standing_statistics against the fp64 oracle, and the train loop with averaging, sample sheets and resume switched on.

Bounds.  ema_update: ema + a (p - ema) is three fp32 operations (difference, product, sum; two with an FMA), each with a
relative rounding error of at most 2^-24 of a quantity no larger than |p| + |ema| (a <= 1), so 3 x 2^-24 (|p| + |ema|), and
one more 2^-24 of slack: 4 x 2^-24 (|p| + |ema|) per element.  Iterated towards a fixed p with a = 0.1 the error obeys
e_{t+1} <= 0.9 e_t + b, i.e. e <= 10 b.  Everything else is bitwise, or the tolerance of the test it cites."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import scrabble_oracle as O  # noqa: E402  (checker only)
from tests.test_nets_gpu import close, nl_pair, perturb  # noqa: E402

SIZES = [4, 5, 1023, 1024, 1025, 2 ** 22 + 5]      # vector body alone, a tail, a partial last workgroup, more than one grid pass
EPS = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _values(n, gen, dev):
    """fp32 values of both signs over six orders of magnitude."""
    mag = 10.0 ** (torch.rand(n, generator=gen) * 6 - 3)
    return (torch.randn(n, generator=gen) * mag).float().to(dev)


def _ema_ref(ema, p, a32):
    e, q = ema.double().cpu().numpy(), p.double().cpu().numpy()
    return e + float(a32) * (q - e)


# --------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("n", SIZES)
def test_ema_update_against_float64(dev, n):
    from scrabble_gan_amd import ops
    gen = torch.Generator().manual_seed(n)
    p = _values(n, gen, dev)
    p0 = p.clone()
    for coef in (1 - 0.9999, 0.5, 0.1):
        a32 = np.float32(coef)                              # the one rounding of the coefficient (ctypes does the same)
        ema = _values(n, gen, dev)
        ref = _ema_ref(ema, p, a32)
        bound = 4 * EPS * (p.abs() + ema.abs()).double().cpu().numpy()
        ops.ema_update(ema, p, coef)
        err = np.abs(ema.double().cpu().numpy() - ref)
        worst = float((err / np.maximum(bound, 1e-300)).max())
        print("ema_update n=%d coef=%g: worst error %.3f of the bound" % (n, coef, worst))
        assert (err <= bound).all(), (n, coef, worst)
    ema = _values(n, gen, dev)
    before = ema.clone()
    ops.ema_update(ema, p, 0.0)
    assert torch.equal(ema, before)                         # coefficient 0: bitwise unchanged
    ops.ema_update(ema, p, 1.0)
    assert torch.equal(ema, p)                              # coefficient 1: bitwise p (ema + (p - ema) would not be)
    assert torch.equal(p, p0)                               # p is never written


def test_ema_recursion_stays_within_ten_step_bounds(dev):
    from scrabble_gan_amd import ops
    gen = torch.Generator().manual_seed(11)
    n = 1025
    p, ema = _values(n, gen, dev), _values(n, gen, dev)
    a32 = np.float32(0.1)
    ref = ema.double().cpu().numpy()
    q = p.double().cpu().numpy()
    # |ema_t| <= max(|ema_0|, |p|) (a convex combination), so every step's bound is at most this one
    step_bound = 4 * EPS * (np.abs(q) + np.maximum(np.abs(ref), np.abs(q)))
    for _ in range(200):
        ops.ema_update(ema, p, 0.1)
        ref = ref + float(a32) * (q - ref)
    err = np.abs(ema.double().cpu().numpy() - ref)
    print("200 updates: worst error %.3f of 10 step bounds" % float((err / (10 * step_bound)).max()))
    assert (err <= 10 * step_bound).all()


def test_argument_checks_return_before_launching(dev):
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import ScrabbleHipError, call
    buf, other = torch.zeros(64, device=dev), torch.ones(64, device=dev)
    off = buf[1:33]                                         # one float into the buffer: 4-byte, not 16-byte aligned
    for fn in (lambda: ops.ema_update(off, other[:32], 0.5), lambda: ops.ema_update(other[:32], off, 0.5),
               lambda: ops.swap_buffers(off, other[:32]), lambda: ops.swap_buffers(other[:32], off),
               lambda: ops.ema_update(buf, other, 1.5), lambda: ops.ema_update(buf, other, -0.1),
               lambda: ops.swap_buffers(buf[:48], buf[16:64])):            # overlapping halves
        with pytest.raises(ScrabbleHipError):
            fn()
    call("sg_ema_update", buf.data_ptr(), other.data_ptr(), 0, 0.5, ops._stream())          # n = 0: success, nothing changes
    call("sg_swap_f32", buf.data_ptr(), other.data_ptr(), 0, ops._stream())
    with pytest.raises(ScrabbleHipError):
        call("sg_ema_update", buf.data_ptr(), other.data_ptr(), -1, 0.5, ops._stream())
    assert torch.equal(buf, torch.zeros(64, device=dev)) and torch.equal(other, torch.ones(64, device=dev))


@pytest.mark.parametrize("n", SIZES)
def test_swap_buffers_exchanges_bitwise(dev, n):
    from scrabble_gan_amd import ops
    gen = torch.Generator().manual_seed(100 + n)
    a, b = _values(n, gen, dev), _values(n, gen, dev)
    a0, b0 = a.clone(), b.clone()
    ops.swap_buffers(a, b)
    assert torch.equal(a, b0) and torch.equal(b, a0)
    ops.swap_buffers(a, b)
    assert torch.equal(a, a0) and torch.equal(b, b0)


def _sheet_ref(imgs, cols, pad, fill):
    """numpy construction with the pixel expression of run_inference.generate / save_grid, in float32."""
    N, H, W = imgs.shape
    rows = (N + cols - 1) // cols
    out = np.full((rows * (H + pad) - pad, cols * (W + pad) - pad), fill, np.uint8)
    for i in range(N):
        r, c = divmod(i, cols)
        v = ((imgs[i] + 1.0) / 2.0).clip(0.0, 1.0)
        assert v.dtype == np.float32
        out[r * (H + pad):r * (H + pad) + H, c * (W + pad):c * (W + pad) + W] = np.round(v * 255.0).astype(np.uint8)
    return out


@pytest.mark.parametrize("N,H,W,cols,pad", [(5, 32, 16, 2, 2), (1, 32, 48, 4, 0), (16, 32, 160, 4, 2), (3, 32, 16, 3, 1)])
def test_image_sheet_is_byte_identical_to_numpy(dev, N, H, W, cols, pad):
    from scrabble_gan_amd import ops
    rng = np.random.default_rng(N * 1000 + W)
    imgs = rng.uniform(-1.2, 1.2, (N, H, W)).astype(np.float32)           # some values outside [-1, 1]
    flat = imgs.reshape(-1)
    flat[0], flat[1], flat[2], flat[3] = -1.0, 1.0, -3.0, 2.5
    k = np.arange(0, 255, dtype=np.float32)[: flat.size - 4]
    flat[4:4 + k.size] = ((k + np.float32(0.5)) / np.float32(255.0)) * 2 - 1    # products with 255 that land on (or next to) .5
    halves = ((flat + 1.0) / 2.0).clip(0.0, 1.0) * 255.0
    assert (np.abs(halves - np.floor(halves) - 0.5) == 0).sum() >= 8           # exact ties are among them: round-half-even is exercised
    for fill in (255, 7):
        got = ops.image_sheet_u8(torch.from_numpy(imgs).to(dev).unsqueeze(-1), cols, pad, fill).cpu().numpy()
        ref = _sheet_ref(imgs, cols, pad, fill)
        assert got.shape == ref.shape and got.dtype == np.uint8
        assert np.array_equal(got, ref), "sheet differs in %d bytes" % int((got != ref).sum())
        if pad:
            assert (got[H:H + pad] == fill).all() if got.shape[0] > H else True
            if cols > 1:
                assert (got[:, W:W + pad] == fill).all()
        if N % cols:                                                            # the unused cells of a ragged last row
            r, c = divmod(N, cols)
            assert (got[r * (H + pad):, c * (W + pad):] == fill).all()


# --------------------------------------------------------------------------------------------------------- host layer
@pytest.fixture(scope="module")
def NA(dev):
    from scrabble_gan_amd import net_architecture as NA_
    NA_.configure(device=dev, seed=3)
    return NA_


@pytest.fixture(scope="module")
def Gmod(NA):
    """One generator for the module (its orthogonal initialisers are the expensive part); tests put back what they change."""
    return NA.make_generator(128, (32, 160, 1), (32, 8192), None, "B3", 52, vis_model=False)


def test_weight_average_follows_the_float64_recursion(NA, dev):
    from scrabble_gan_amd import nn
    from scrabble_gan_amd.averaging import WeightAverage
    specs = [("a.w", (3, 3, 8, 8), nn.orthogonal, True), ("a.b", (8,), nn.zeros, True), ("c.w", (37, 5), nn.glorot_uniform, True),
             ("bn.mm", (8,), nn.zeros, False), ("bn.mv", (8,), nn.ones, False)]
    gen = torch.Generator().manual_seed(5)
    m = NA._Model("tiny", specs, gen)
    avg = WeightAverage(m, decay=0.999, start_step=2, warmup=True)
    assert torch.equal(avg.flat, m.store.flat) and avg.flat.data_ptr() != m.store.flat.data_ptr()
    ref = avg.flat.double().cpu().numpy()
    acc = np.zeros_like(ref)                                # bound of |buffer - recursion|: acc <- (1 - a) acc + this step's bound
    for t, coef in enumerate((1.0, 1.0, 1 - 1 / 10, 1 - 2 / 11, 1 - 3 / 12)):
        m.store.flat.add_(torch.randn(m.store.flat.numel(), generator=gen).to(dev) * 0.05)      # the weights move between updates
        w = m.store.flat.double().cpu().numpy()
        bound = 4 * EPS * (np.abs(w) + np.abs(avg.flat.double().cpu().numpy()))
        prev = avg.flat.double().cpu().numpy()
        avg.update()
        assert avg.t == t + 1
        step_ref = prev + float(np.float32(coef)) * (w - prev)             # one step from the buffer's own previous value
        assert (np.abs(avg.flat.double().cpu().numpy() - step_ref) <= bound).all(), t
        ref = ref + float(np.float32(coef)) * (w - ref)
        acc = (1 - float(np.float32(coef))) * acc + bound
        assert (np.abs(avg.flat.double().cpu().numpy() - ref) <= acc).all(), t
        if coef == 1.0:
            assert torch.equal(avg.flat, m.store.flat)
    avg.standing = torch.arange(m.store.state.numel(), device=dev, dtype=torch.float32)
    sd = avg.state_dict()
    other = WeightAverage(m, decay=0.999, start_step=2)
    other.load_state_dict(sd)
    assert other.t == 5 and torch.equal(other.flat, avg.flat) and torch.equal(other.standing, avg.standing)
    other.update()                                                          # the restored counter continues the schedule
    avg.update()
    assert torch.equal(other.flat, avg.flat) and other.t == avg.t == 6


def _second_generator(NA, weights):
    from scrabble_gan_amd import nn
    nn.FAST_INIT = True                 # every weight is loaded below
    try:
        G2 = NA.make_generator(128, (32, 160, 1), (32, 8192), None, "B3", 52, vis_model=False)
    finally:
        nn.FAST_INIT = False
    G2.store.load(weights)
    return G2


def test_applied_swaps_weights_in_and_out(NA, Gmod, dev):
    from scrabble_gan_amd import ops
    from scrabble_gan_amd.averaging import WeightAverage
    G = Gmod
    gen = torch.Generator().manual_seed(21)
    flat0, state0 = G.store.flat.clone(), G.store.state.clone()
    style = (torch.rand(2, 32, 32, 1, generator=gen) * 2 - 1).numpy()
    y = torch.randint(0, 52, (2, 2), generator=gen).numpy().astype(np.int32)

    def render(model):
        model.nl_gen.manual_seed(5)                         # the same NonLocalBlock kernels for every call
        return model([style, y], training=False).clone()

    NA.configure(deterministic=True)
    try:
        avg = WeightAverage(G, decay=0.5, warmup=False)
        G.store.flat.add_(torch.randn(G.store.flat.numel(), generator=gen).to(dev) * 0.01)      # the live weights move on ...
        ops.weights_changed()
        avg.update()                                        # ... and the average follows half way
        live_flat, live_state = G.store.flat.clone(), G.store.state.clone()
        assert not torch.equal(avg.flat, live_flat)
        live = render(G)                                    # warms the packed / transposed / Winograd filter caches of the LIVE weights
        G2 = _second_generator(NA, avg.export())
        ref = render(G2)
        assert not torch.equal(ref, live)
        with avg.applied() as m:
            assert m is G and all(torch.equal(G.store.p[k], G2.store.p[k]) for k in G.store.names)    # (not .flat: its padding moved too)
            inside = render(G)
        assert torch.equal(inside, ref)                     # fails when a cached filter copy of the live weights is used
        assert torch.equal(G.store.flat, live_flat) and torch.equal(G.store.state, live_state)
        assert torch.equal(render(G), live)
        with pytest.raises(KeyError):
            with avg.applied():
                raise KeyError("body fails")
        assert torch.equal(G.store.flat, live_flat) and torch.equal(G.store.state, live_state)
        assert torch.equal(render(G), live)
    finally:
        NA.configure(deterministic=False)
        G.store.flat.copy_(flat0)
        G.store.state.copy_(state0)
        ops.weights_changed()


class _NoCollectives:
    """A data-parallel reducer none of whose collectives may be called."""
    world_size, rank, sync_bn = 2, 0, True

    def _refuse(self, *a, **k):
        raise AssertionError("standing statistics must not communicate")

    all_reduce_sum = all_reduce_sum_async = wait = broadcast_object = shard = _refuse


def test_standing_statistics_against_the_oracle(NA, Gmod, dev):
    from scrabble_gan_amd import ops
    from scrabble_gan_amd.averaging import WeightAverage, standing_statistics
    G = Gmod
    gen = torch.Generator().manual_seed(72)
    flat0, state0 = G.store.flat.clone(), G.store.state.clone()
    try:
        P = perturb(G, gen)                                 # the weights that become the average (fp64 copies for the oracle)
        ops.weights_changed()
        avg = WeightAverage(G)
        G.store.flat.mul_(0.9)                              # the live weights differ from the average
        ops.weights_changed()
        B, L, nb = 3, 2, 2
        styles = [torch.rand(B, 32, 32, 1, generator=gen, dtype=torch.float64) * 2 - 1 for _ in range(nb)]
        ys = [torch.randint(0, 52, (B, L), generator=gen) for _ in range(nb)]
        nls_o, nls_g = nl_pair(64, gen, dev)
        nlu_o, nlu_g = nl_pair(64, gen, dev)
        nl = {"G.style": nls_g, "G.up": nlu_g}

        # reference: the fp64 oracle in training mode; its BatchNorm is wrapped (as tests/step_fixture.py wraps its ReLU) to record
        # the seven (mean, biased variance, count) triples of each batch
        seen = []
        bn = O.batch_norm_train

        def recording(x, *a, **k):
            out = bn(x, *a, **k)
            seen.append((out[1].detach().clone(), out[2].detach().clone(), x.numel() // x.shape[-1]))
            return out

        O.batch_norm_train = recording
        try:
            with torch.no_grad():
                for s, y in zip(styles, ys):
                    O.generator(s, y, P, nls_o, nlu_o, training=True)
        finally:
            O.batch_norm_train = bn
        names = ["B1.cbn1", "B1.cbn2", "B2.cbn1", "B2.cbn2", "B3.cbn1", "B3.cbn2", "bn"]
        assert len(seen) == 7 * nb
        ref_stats = {}
        for j, name in enumerate(names):
            per_batch = [seen[7 * i + j] for i in range(nb)]
            ref_stats[name + ".mm"] = sum(m for m, _, _ in per_batch) / nb
            ref_stats[name + ".mv"] = sum(v * c / (c - 1) for _, v, c in per_batch) / nb

        live_stats = {k: G.store.p[k].clone() for k in G.store.names if k.endswith((".mm", ".mv"))}
        G.reducer = _NoCollectives()
        try:
            with avg.applied():
                standing_statistics(avg, [(s.float().numpy(), y.numpy().astype(np.int32)) for s, y in zip(styles, ys)], nl=nl)
            got = avg.standing_named()
            assert set(got) == set(ref_stats)
            for k, v in ref_stats.items():
                # the tolerance of the moving-statistics assertion of tests/test_nets_gpu.py::test_train_step: close(..., 1e-4)
                close(got[k], v, 1e-4, "standing statistic " + k)
            for k, v in live_stats.items():                 # the live generator's statistics are untouched
                assert torch.equal(G.store.p[k], v), k

            # inference with the averaged weights and these statistics (tests/test_configs_gpu.py::test_generator_inference_matches_oracle: 1e-4)
            P_ref = dict(P)
            P_ref.update(ref_stats)
            with torch.no_grad():
                ref_img = O.generator(styles[0], ys[0], P_ref, nls_o, nlu_o, training=False)
            with avg.applied():
                img, _ = G.forward(styles[0].float().to(dev), ys[0].int().to(dev), nls_g, nlu_g, training=False)
            close(img, ref_img, 1e-4, "inference image with standing statistics")

            # without explicit kernels the passes draw from G's generators -- and put them back
            before = {a: getattr(G, a).get_state().clone() for a in ("nl_gen", "sn_gen")}
            with avg.applied():
                standing_statistics(avg, [(styles[0].float().numpy(), ys[0].numpy().astype(np.int32))])
            for a, s in before.items():
                assert torch.equal(getattr(G, a).get_state(), s), a
            for k, v in live_stats.items():
                assert torch.equal(G.store.p[k], v), k
        finally:
            G.reducer = NA.LOCAL
    finally:
        G.store.flat.copy_(flat0)
        G.store.state.copy_(state0)
        ops.weights_changed()


# --------------------------------------------------------------------------------------------------------- the loop
NUM_GEN = 6          # a ragged sheet: two rows of four cells, two of them unused


@pytest.fixture(scope="module")
def runs(dev, tmp_path_factory):
    """main() four times on the synthetic data, deterministic mode: plain; with averaging, standing statistics, sample sheets and
    legibility on (resumable, uninterrupted); and the same stopped after epoch 1 and resumed."""
    from scrabble_gan_amd import gin_config as gin, main as M, net_architecture as NA_
    base = open(os.path.join(ROOT, "configs", "scrabble_gan_mi355x.gin")).read()
    common = ["--synthetic", "--steps", "2", "--batch-size", "4", "--deterministic"]
    extra = ["--ema-decay", "0.9", "--ema-standing-batches", "1", "--samples-every", "1", "--legibility-every", "1"]
    dirs = {}

    def run(name, args):
        if name not in dirs:
            dirs[name] = tmp_path_factory.mktemp(name)
        d = dirs[name]
        cfg = d / "cfg.gin"
        cfg.write_text(base + "\nio.base_path = '%s/'\nshared_specs.num_gen = %d\n" % (d, NUM_GEN))
        gin.clear_config()
        NA_._model_counter[0] = 0                           # every run starts from the same initial weights
        try:
            M.main(["--gin", str(cfg)] + common + args)
        finally:
            gin.clear_config()

    try:
        run("plain", ["--epochs", "2"])
        run("ema", ["--epochs", "2", "--resumable"] + extra)
        run("resumed", ["--epochs", "1", "--resumable"] + extra)
        run("resumed", ["--epochs", "2", "--resumable"] + extra)
    finally:
        NA_.configure(deterministic=False)
    return dirs


def _ckpt(d, net, e):
    from safetensors.torch import load_file
    return load_file(str(d / "run" / "checkpoints" / net / str(e) / ("cktp-%d.safetensors" % e)))


def test_averaging_never_feeds_back(runs):
    plain, ema = runs["plain"], runs["ema"]
    assert (plain / "run" / "output" / "batch_summary.txt").read_text() == (ema / "run" / "output" / "batch_summary.txt").read_text()
    a, b = _ckpt(plain, "generator", 2), _ckpt(ema, "generator", 2)
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not (plain / "run" / "checkpoints" / "generator_ema").exists()
    assert not list((plain / "run" / "output").glob("image_at_epoch_*.png"))
    assert not (plain / "run" / "model" / "legibility_ema.csv").exists()


def test_averaged_checkpoints_sheets_and_legibility(runs):
    from PIL import Image
    from scrabble_gan_amd.legibility import LEGIBILITY_HEADER
    ema = runs["ema"]
    for e in (1, 2):
        g, a = _ckpt(ema, "generator", e), _ckpt(ema, "generator_ema", e)
        assert set(g) == set(a)
        differ = [k for k in g if not torch.equal(g[k], a[k])]
        assert any(not k.endswith((".mm", ".mv")) for k in differ), "the averaged weights equal the last iterate"
        assert any(k.endswith((".mm", ".mv")) for k in differ), "the averaged generator carries the live statistics"
        assert all(torch.isfinite(v).all() for v in a.values())
    random.seed(0)                                          # main's draw of the seed bucket: word length L = index + 1
    L = random.randint(4, 9) + 1
    rows = (NUM_GEN + 3) // 4
    for e in (1, 2):
        im = Image.open(ema / "run" / "output" / ("image_at_epoch_%04d.png" % e))
        assert im.mode == "L" and im.size == (4 * (16 * L + 2) - 2, rows * (32 + 2) - 2)
        px = np.asarray(im)
        assert (px[32 + 2:, 2 * (16 * L + 2):] == 255).all()        # the two unused cells of the last row
    lines = (ema / "run" / "model" / "legibility_ema.csv").read_text().strip().split("\n")
    assert lines[0] + "\n" == LEGIBILITY_HEADER and len(lines) == 3
    live = (ema / "run" / "model" / "legibility.csv").read_text().strip().split("\n")
    for row, row_live in zip(lines[1:], live[1:]):
        cols, cols_live = row.split(","), row_live.split(",")
        assert len(cols) == 6 and all(np.isfinite(float(c)) for c in cols)
        assert cols[:4] == cols_live[:4]                    # epoch, n and R's reading of the REAL batch do not depend on the generator


def test_resumed_run_continues_the_average(runs):
    from safetensors.torch import load_file
    a = load_file(str(runs["ema"] / "run" / "checkpoints" / "state" / "latest.safetensors"))
    b = load_file(str(runs["resumed"] / "run" / "checkpoints" / "state" / "latest.safetensors"))
    assert set(a) == set(b)
    keys = [k for k in a if k.startswith("G.ema/")]
    assert set(keys) == {"G.ema/flat", "G.ema/t", "G.ema/standing"}
    assert a["G.ema/t"].item() == 4
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    assert a["position"].tolist() == b["position"].tolist() == [1, 2]
    assert len((runs["resumed"] / "run" / "model" / "legibility_ema.csv").read_text().strip().split("\n")) == 3
