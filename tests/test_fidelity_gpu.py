"""The fidelity statistics on the GPU, through the C-ABI via ops: fragment layout (exact integer data), edge shapes, determinism,
argument checks, the feature accessors, evaluate_fidelity end to end and the train loop's hook.

Error bounds are derived, not measured.  The fp32 operands are widened to fp64 and a product of two fp32 values is exact in fp64,
so only the additions round: a sum of n terms in any order is within (n - 1) u sum |terms| of the true one, u = 2^-53; the
numpy reference (another order) has the same bound, hence the (n + 1) 2^-52 of the comparisons below."""
import os

import numpy as np
import pytest
import torch

from tests import fidelity_refs as FR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ints(rng, *shape):
    return rng.integers(-8, 9, shape).astype(np.float32)


# ------------------------------------------------------------------------------------------------------- 1. layout, exact
@pytest.mark.parametrize("n,D", [(4, 16), (4, 48)])
def test_moments_layout_is_exact_on_integer_data(dev, n, D):
    """Integer-valued data: every fp64 sum is exact, so the result must EQUAL the reference.  (4, 48) has off-diagonal tiles of
    MFMA blocks, which are not symmetric: a transposed or row-permuted accumulator store shows here."""
    from scrabble_gan_amd import ops
    x = _ints(np.random.default_rng(D), n, D)
    s, o = ops.feature_moments(_t(x, dev))
    want_s, want_o, _, _ = FR.moments_ref(x)
    assert np.array_equal(s.cpu().numpy(), want_s)
    assert np.array_equal(o.cpu().numpy(), want_o)


@pytest.mark.parametrize("S,m,D", [(1, 5, 16), (2, 20, 24)])
def test_kernel_sums_layout_is_exact_on_integer_data(dev, S, m, D):
    """gamma = 2^-4, coef0 = 1: the kernel values are multiples of 2^-12 below 2^20, every sum is exact in fp64."""
    from scrabble_gan_amd import ops
    rng = np.random.default_rng(100 + D)
    x, y = _ints(rng, m + 3, D), _ints(rng, m + 2, D)
    ix = np.stack([rng.choice(m + 3, m, replace=False) for _ in range(S)]).astype(np.int32)
    iy = np.stack([rng.choice(m + 2, m, replace=False) for _ in range(S)]).astype(np.int32)
    got = ops.poly_mmd_sums(_t(x, dev), _t(y, dev), _t(ix, dev), _t(iy, dev), gamma=2.0 ** -4, coef0=1.0).cpu().numpy()
    want, _ = FR.gram_sums_ref(x, y, ix, iy, 2.0 ** -4, 1.0)
    assert got.shape == (S, 3) and np.array_equal(got, want), (got, want)


# ------------------------------------------------------------------------------------------------------- 2. moments, edges
def _moments_case(dev, chunks, D, wide=0):
    """Accumulate the row chunks into one pair of buffers -> (sum, outer) tensors."""
    from scrabble_gan_amd import ops
    s = torch.zeros(D, device=dev, dtype=torch.float64)
    o = torch.zeros(D, D, device=dev, dtype=torch.float64)
    for c in chunks:
        if wide:                                   # a column slice of a wider tensor: ldx > D
            buf = torch.full((c.shape[0], D + wide), float("nan"), device=dev)
            buf[:, 5:5 + D] = _t(c, dev)
            xd = buf[:, 5:5 + D]
            assert not xd.is_contiguous() or c.shape[0] == 1
        else:
            xd = _t(c, dev)
        ops.feature_moments(xd, s, o)
    return s, o


@pytest.mark.parametrize("ns,D,wide", [((1,), 16, 0), ((5,), 24, 11), ((130,), 80, 0), ((67,), 1024, 0), ((3,), 1030, 0), ((7, 64, 1), 24, 0)])
def test_moments_edges(dev, ns, D, wide):
    rng = np.random.default_rng(D + sum(ns))
    chunks = [rng.standard_normal((n, D)).astype(np.float32) for n in ns]
    x = np.concatenate(chunks, 0)
    n = x.shape[0]
    s, o = _moments_case(dev, chunks, D, wide)
    want_s, want_o, abs_o, abs_s = FR.moments_ref(x)
    got_s, got_o = s.cpu().numpy(), o.cpu().numpy()
    assert np.all(np.abs(got_o - want_o) <= (n + 1) * 2.0 ** -52 * abs_o)
    assert np.all(np.abs(got_s - want_s) <= (n + 1) * 2.0 ** -52 * abs_s)
    assert torch.equal(o, o.T.contiguous()), "outer must be bitwise symmetric"
    s2, o2 = _moments_case(dev, chunks, D, wide)
    assert torch.equal(s, s2) and torch.equal(o, o2), "a second run from zeroed buffers must be bitwise equal"


# ------------------------------------------------------------------------------------------------------- 3. covariance
def test_covariance_against_two_pass_numpy(dev):
    """Mean 10, unit variance: outer - n mean mean^T cancels two digits.  cov = (outer - n m_a m_b) / (n - 1): outer carries
    (n - 1) u |X|^T|X|, each mean (n - 1) u from its sum and u from the division, the product n m_a m_b two more roundings, and
    n |m_a m_b| <= about (|X|^T|X|)[a,b] for this data -- below 4 n u (|X|^T|X|)[a,b] / (n - 1) in all."""
    from scrabble_gan_amd import ops
    n, D = 200, 24
    x = (10.0 + np.random.default_rng(7).standard_normal((n, D))).astype(np.float32)
    s, o = ops.feature_moments(_t(x, dev))
    mean, cov = ops.feature_cov(s, o, n)
    want_mean, want_cov = FR.cov_ref(x)
    _, _, abs_o, abs_s = FR.moments_ref(x)
    assert np.all(np.abs(cov.cpu().numpy() - want_cov) <= 4 * n * FR.U * abs_o / (n - 1))
    assert np.all(np.abs(mean.cpu().numpy() - want_mean) <= (n + 1) * 2.0 ** -52 * abs_s / n)


# ------------------------------------------------------------------------------------------------------- 4. kernel sums, edges
def _sums_bound(D, m, base):
    """gamma G + coef0 carries (D + 2) u of |gamma| |X|.|Y| + |coef0|, its cube three times that (to first order), the m^2 terms
    are added in some order."""
    return (3 * (D + 2) + m * m) * FR.U * base


@pytest.mark.parametrize("S,m,D,opt", [(1, 2, 16, {}), (3, 5, 24, {"shared": True, "gamma": 0.37, "coef0": -0.5}), (2, 70, 80, {"wide": 9}),
                                       (1, 33, 1030, {"null": True})])
def test_kernel_sums_edges(dev, S, m, D, opt):
    from scrabble_gan_amd import ops
    rng = np.random.default_rng(1000 + D)
    nx, ny = (m, m) if opt.get("null") else (m + 6, m + 3)
    x, y = rng.standard_normal((nx, D)).astype(np.float32), (0.5 + rng.standard_normal((ny, D))).astype(np.float32)
    ix = np.stack([rng.choice(nx, m, replace=False) for _ in range(S)]).astype(np.int32)
    iy = np.stack([rng.choice(ny, m, replace=False) for _ in range(S)]).astype(np.int32)
    if opt.get("shared"):
        ix[1], iy[2] = ix[0], iy[0]                     # index rows shared between subsets
    if opt.get("null"):
        ix = iy = np.arange(m, dtype=np.int32)[None]    # what NULL index pointers stand for
    gamma, coef0 = opt.get("gamma", 1.0 / D), opt.get("coef0", 1.0)
    xd, yd = _t(x, dev), _t(y, dev)
    if opt.get("wide"):
        bx = torch.full((nx, D + opt["wide"]), float("nan"), device=dev)
        by = torch.full((ny, D + 2 * opt["wide"]), float("nan"), device=dev)
        bx[:, 3:3 + D], by[:, 1:1 + D] = xd, yd
        xd, yd = bx[:, 3:3 + D], by[:, 1:1 + D]

    def run():
        if opt.get("null"):
            return ops.poly_mmd_sums(xd, yd, gamma=gamma, coef0=coef0)
        return ops.poly_mmd_sums(xd, yd, _t(ix, dev), _t(iy, dev), gamma=gamma, coef0=coef0)

    got = run()
    want, base = FR.gram_sums_ref(x, y, ix, iy, gamma, coef0)
    _, base_xx = FR.gram_sums_ref(x, x, ix, ix, gamma, coef0)
    _, base_yy = FR.gram_sums_ref(y, y, iy, iy, gamma, coef0)
    g = got.cpu().numpy()
    assert g.shape == (S, 3)
    for k, b in enumerate((base_xx, base_yy, base)):
        assert np.all(np.abs(g[:, k] - want[:, k]) <= _sums_bound(D, m, b)), (k, g[:, k], want[:, k])
    assert torch.equal(got, run()), "a repeat call must be bitwise equal"
    # y the same array as x, equal indices: the YY sum repeats the XX sum bit for bit, and XY - XX is the excluded diagonal
    if opt.get("null"):
        same = ops.poly_mmd_sums(xd, xd, gamma=gamma, coef0=coef0).cpu().numpy()
    else:
        same = ops.poly_mmd_sums(xd, xd, _t(ix, dev), _t(ix, dev), gamma=gamma, coef0=coef0).cpu().numpy()
    assert np.array_equal(same[:, 0], same[:, 1])
    X64 = x.astype(np.float64)
    for s in range(S):
        diag = ((gamma * np.sum(X64[ix[s]] ** 2, 1) + coef0) ** 3).sum()
        assert abs((same[s, 2] - same[s, 0]) - diag) <= _sums_bound(D, m, base_xx[s])


# ------------------------------------------------------------------------------------------------------- 5. arguments
def test_bad_arguments_are_refused_before_any_launch(dev):
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import ScrabbleHipError, call, lib
    x = torch.ones(8, 16, device=dev)
    s, o = torch.full((16,), 7.0, device=dev, dtype=torch.float64), torch.full((16, 16), 7.0, device=dev, dtype=torch.float64)
    mean, cov = torch.full_like(s, 5.0), torch.full_like(o, 5.0)
    ws, sums = torch.full((64,), 3.0, device=dev, dtype=torch.float64), torch.full((2, 3), 3.0, device=dev, dtype=torch.float64)
    P = lambda t: t.data_ptr()
    st = ops._stream()
    bad = [("sg_feature_moments", (P(x), 16, 8, 0, P(s), P(o), st)), ("sg_feature_moments", (P(x), 4097, 8, 4097, P(s), P(o), st)),
           ("sg_feature_moments", (P(x), 16, 0, 16, P(s), P(o), st)), ("sg_feature_moments", (P(x), 15, 8, 16, P(s), P(o), st)),
           ("sg_feature_moments", (None, 16, 8, 16, P(s), P(o), st)), ("sg_feature_moments", (P(x), 16, 8, 16, None, P(o), st)),
           ("sg_feature_moments", (P(x), 16, 8, 16, P(s), None, st)),
           ("sg_feature_cov", (P(s), P(o), 1.0, P(mean), P(cov), 16, st)), ("sg_feature_cov", (P(s), P(o), float("nan"), P(mean), P(cov), 16, st)),
           ("sg_feature_cov", (P(s), P(o), 8.0, P(mean), P(cov), 0, st)), ("sg_feature_cov", (P(s), P(o), 8.0, P(mean), P(cov), 4097, st)),
           ("sg_feature_cov", (None, P(o), 8.0, P(mean), P(cov), 16, st)), ("sg_feature_cov", (P(s), None, 8.0, P(mean), P(cov), 16, st)),
           ("sg_feature_cov", (P(s), P(o), 8.0, None, P(cov), 16, st)), ("sg_feature_cov", (P(s), P(o), 8.0, P(mean), None, 16, st))]
    mmd = dict(x=P(x), ldx=16, y=P(x), ldy=16, ix=None, iy=None, S=1, m=4, D=16, gamma=0.1, coef0=1.0, ws=P(ws), sums=P(sums), st=st)
    for change in ({"m": 0}, {"S": 0}, {"D": 0}, {"D": 4097, "ldx": 4097, "ldy": 4097}, {"ldx": 15}, {"ldy": 15}, {"x": None}, {"y": None},
                   {"ws": None}, {"sums": None}):
        bad.append(("sg_poly_mmd_sums", tuple({**mmd, **change}.values())))
    for name, args in bad:
        with pytest.raises(ScrabbleHipError, match="SG_ERR_ARG"):
            call(name, *args)
    torch.cuda.synchronize()
    assert (s == 7).all() and (o == 7).all() and (mean == 5).all() and (cov == 5).all() and (ws == 3).all() and (sums == 3).all(), \
        "a refused call must not launch anything"
    assert lib().sg_poly_mmd_workspace_doubles(0, 5) == -1 and lib().sg_poly_mmd_workspace_doubles(1, 0) == -1
    assert lib().sg_poly_mmd_workspace_doubles(2, 70) == 2 * (3 + 3 + 4)          # two tiles a side: 3 + 3 upper-triangle pairs, 4 XY tiles
    # m = 1 is legal: no pair i != j, one cross term
    one = ops.poly_mmd_sums(x[:1], 2 * x[:1], gamma=0.125, coef0=1.0).cpu().numpy()
    assert np.array_equal(one, [[0.0, 0.0, (0.125 * 32 + 1.0) ** 3]])
    # the wrappers check what they can see themselves
    for fn in (lambda: ops.feature_moments(x.double()), lambda: ops.feature_moments(x.t()), lambda: ops.feature_moments(x, s[:8], o),
               lambda: ops.feature_cov(s, o, 1), lambda: ops.poly_mmd_sums(x, x[:, :8]), lambda: ops.poly_mmd_sums(x, x, m=9),
               lambda: ops.poly_mmd_sums(x, x, torch.zeros(1, 4, device=dev, dtype=torch.int64), torch.zeros(1, 4, device=dev, dtype=torch.int64))):
        with pytest.raises(ValueError):
            fn()


# ------------------------------------------------------------------------------------------------------- 6. accessors
def _gen_states(*models):
    return [getattr(m, a).get_state().clone() for m in models for a in ("nl_gen", "sn_gen", "mask_gen") if hasattr(m, a)]


def test_feature_accessors(dev):
    """Deterministic mode: one adder per conv output, so two forward passes of the same images agree bit for bit."""
    from scrabble_gan_amd import data_utils as DU, fidelity, net_architecture as NA, nn, ops
    B, L = 3, 2
    images, _, _ = DU.synthetic_batch(B, L, seed=11)
    NA.configure(device=dev, seed=3, deterministic=True)
    try:
        for factory in (NA.make_recognizer, NA.make_my_recognizer):
            R = factory((32, 160, 1), None, 53, vis_model=False)
            before = _gen_states(R)
            f = R.features(images)
            with ops.bf16_only():
                out = R._trunk(NA._as_nhwc1(images, dev), False)
            feat, (b, T) = out[-2], out[-1]
            assert b == B and tuple(f.shape) == (B, feat.shape[1]) and f.dtype == torch.float32
            assert torch.equal(f, ops.gap_fwd(feat.contiguous().view(B, 1, T, -1), relu=False))
            f64 = feat.double().view(B, T, -1)
            assert (f.double() - f64.mean(1)).abs().max().item() <= (T + 1) * 2.0 ** -24 * f64.abs().mean(1).max().item()   # fp32 mean of T frames
            assert all(torch.equal(a, c) for a, c in zip(before, _gen_states(R)))
            assert tuple(fidelity.FeatureExtractor(R, "recognizer")(images).shape) == (B, fidelity.FeatureExtractor(R, "recognizer").dim)
        D = NA.make_discriminator((32, 160, 1), None, "B1", vis_model=False)
        for k in D.store.names:
            if k.endswith(".sigma"):
                D.store.p[k].fill_(0.25)                 # (zero-initialised: the NonLocalBlock would not reach the output)
        nl = nn.nonlocal_weights(64, torch.Generator().manual_seed(5), dev)
        h = D.features(images, nl)
        assert tuple(h.shape) == (B, 1024) and h.dtype == torch.float32 and torch.equal(h, D.forward(images, nl)[1][1])
        before = _gen_states(D)
        e1 = fidelity.FeatureExtractor(D, "discriminator")(images)
        e2 = fidelity.FeatureExtractor(D, "discriminator")(images)
        assert torch.equal(e1, e2), "the fidelity module's NonLocalBlock kernels are fixed, not redrawn"
        assert not torch.equal(e1, h)                    # ... and they do reach the features
        assert all(torch.equal(a, c) for a, c in zip(before, _gen_states(D)))
    finally:
        NA.configure(deterministic=False)


# ------------------------------------------------------------------------------------------------------- 7. end to end, tiny
def test_evaluate_fidelity_end_to_end(dev, tmp_path):
    from scrabble_gan_amd import data_utils as DU, fidelity, net_architecture as NA
    NA.configure(device=dev, seed=5, deterministic=True)      # (the last check below repeats G's pass and compares bit for bit)
    try:
        _end_to_end(dev, tmp_path, DU, fidelity, NA)
    finally:
        NA.configure(deterministic=False)


def _end_to_end(dev, tmp_path, DU, fidelity, NA):
    G = NA.make_generator(128, (32, 160, 1), (32, 8192), None, "B3", 52, vis_model=False)
    R = NA.make_recognizer((32, 160, 1), None, 53, vis_model=False)
    real = [DU.synthetic_batch(4, L, seed=20 + L)[:2] for L in (2, 3)]
    style = DU.synthetic_batch(4, 2, seed=9)[2]
    words = DU.synthetic_random_words(3, 10, seed=2)
    fake_labels = [np.array(words[L - 1][:4], np.int32) for L in (2, 3)]
    seen, orig = [], R.features
    R.features = lambda x: (seen.append(orig(x)), seen[-1])[1]         # the features evaluate_fidelity extracts, as it extracts them
    before = _gen_states(G, R)
    try:
        res = fidelity.evaluate_fidelity(G, R, real, style, fake_labels, space="recognizer", subsets=2, subset_size=4, seed=0)
    finally:
        del R.features
    assert all(torch.equal(a, c) for a, c in zip(before, _gen_states(G, R)))
    assert len(seen) == 4 and (res["n_real"], res["n_fake"], res["feature_space"], res["dim"]) == (8, 8, "recognizer", 512)
    fr, ff = torch.cat(seen[:2]).cpu().numpy(), torch.cat(seen[2:]).cpu().numpy()
    want_f = FR.frechet_samples_ref(fr, ff)                  # 8 rows in 512 dimensions: the small-matrix form of the reference
    ix, iy, m = fidelity.draw_subsets(8, 8, 2, 4, 0)
    want_k, want_ks, _ = FR.kid_ref(fr, ff, ix, iy, 1.0 / 512, 1.0)
    print("frechet %.12e (ref %.12e)  kid %.12e (ref %.12e)  kid_std %.12e (ref %.12e)" % (res["frechet"], want_f, res["kid"], want_k,
                                                                                         res["kid_std"], want_ks))
    assert m == 4 and np.isfinite(want_f) and want_f >= 0
    for got, want in ((res["frechet"], want_f), (res["kid"], want_k), (res["kid_std"], want_ks)):
        assert abs(got - want) <= 1e-9 * max(1.0, abs(want)), (got, want)
    # FeatureStats: save / load round-trips bitwise, merge of two halves = one pass (bound of test_moments_edges)
    feats = torch.cat(seen)
    whole = fidelity.FeatureStats(512, dev).update(feats)
    whole.save(str(tmp_path / "stats.npz"))
    back = fidelity.FeatureStats.load(str(tmp_path / "stats.npz"), dev)
    assert back.n == whole.n == 16 and torch.equal(back.sum, whole.sum) and torch.equal(back.outer, whole.outer)
    halves = fidelity.FeatureStats(512, dev).update(feats[:8]).merge(fidelity.FeatureStats(512, dev).update(feats[8:]))
    _, _, abs_o, abs_s = FR.moments_ref(feats.cpu().numpy())
    assert halves.n == 16
    assert np.all(np.abs((halves.outer - whole.outer).cpu().numpy()) <= 17 * 2.0 ** -52 * abs_o)
    assert np.all(np.abs((halves.sum - whole.sum).cpu().numpy()) <= 17 * 2.0 ** -52 * abs_s)
    # real statistics handed in replace the pass over the real words
    again = fidelity.evaluate_fidelity(G, R, None, style, fake_labels, real_stats=fidelity.FeatureStats(512, dev).update(torch.cat(seen[:2])))
    assert again["kid"] is None and again["frechet"] == res["frechet"] and again["n_real"] == 8


# ------------------------------------------------------------------------------------------------------- 8. train loop
def test_train_loop_writes_fidelity_csv_and_leaves_training_alone(dev, tmp_path):
    from scrabble_gan_amd import gin_config as gin, main as M, net_architecture as NA
    from scrabble_gan_amd.fidelity import FIDELITY_HEADER
    base = open(os.path.join(ROOT, "configs", "scrabble_gan_mi355x.gin")).read()
    common = ["--synthetic", "--steps", "2", "--epochs", "2", "--batch-size", "4", "--deterministic"]

    def run(name, args):
        d = tmp_path / name
        d.mkdir()
        cfg = d / "cfg.gin"
        cfg.write_text(base + "\nio.base_path = '%s/'\nshared_specs.num_gen = 4\n" % d)
        gin.clear_config()
        NA._model_counter[0] = 0                            # every run starts from the same initial weights
        try:
            M.main(["--gin", str(cfg)] + common + args)
        finally:
            gin.clear_config()
        return d

    try:
        plain = run("plain", [])
        fid = run("fid", ["--fidelity-every", "1", "--fidelity-samples", "16"])
    finally:
        NA.configure(deterministic=False)
    lines = (fid / "run" / "model" / "fidelity.csv").read_text().strip().split("\n")
    assert lines[0] + "\n" == FIDELITY_HEADER and len(lines) == 3
    for e, row in enumerate(lines[1:]):
        cols = row.split(",")
        assert len(cols) == 6 and int(cols[0]) == e + 1 and int(cols[1]) == 8 * (e + 1) and int(cols[2]) == 16
        assert all(np.isfinite(float(c)) for c in cols[3:]) and float(cols[5]) >= 0
    assert not (plain / "run" / "model" / "fidelity.csv").exists()
    a, b = (plain / "run" / "output" / "batch_summary.txt").read_text(), (fid / "run" / "output" / "batch_summary.txt").read_text()
    assert len(a.strip().split("\n")) == 5 and a == b, "the evaluation must not change what training computes"
