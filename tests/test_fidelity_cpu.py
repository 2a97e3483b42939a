"""Host side of the fidelity feature, no GPU: the Frechet distance on closed forms, the kernel-distance estimator from its three
Gram sums, the subset drawing that keeps out-of-range rows away from the kernel, and the command-line surface."""
import inspect

import numpy as np
import pytest

from tests import fidelity_refs as FR


def _orthogonal(rng, D):
    q, _ = np.linalg.qr(rng.standard_normal((D, D)))
    return q


def test_frechet_on_gaussians_with_a_shared_eigenbasis():
    """Covariances Q diag(a) Q^T and Q diag(b) Q^T commute: d^2 = |dmu|^2 + sum (sqrt a_i - sqrt b_i)^2."""
    from scrabble_gan_amd.fidelity import frechet_from_moments
    rng = np.random.default_rng(0)
    for D in (1, 6, 40):
        q = _orthogonal(rng, D)
        a, b = rng.uniform(0.5, 2.0, D), rng.uniform(0.5, 2.0, D)
        c1, c2 = (q * a) @ q.T, (q * b) @ q.T
        mu1, mu2 = rng.standard_normal(D), rng.standard_normal(D)
        want = np.sum((mu1 - mu2) ** 2) + np.sum((np.sqrt(a) - np.sqrt(b)) ** 2)
        bound = 1e-10 * (np.trace(c1) + np.trace(c2) + np.sum((mu1 - mu2) ** 2))
        got = frechet_from_moments(mu1, c1, mu2, c2)
        assert abs(got - want) <= bound, (D, got, want)
        assert abs(got - FR.frechet_ref(mu1, c1, mu2, c2)) <= bound
        assert abs(frechet_from_moments(mu1, c1, mu1, c1)) <= 1e-10 * 2 * np.trace(c1)


def test_frechet_stays_finite_for_rank_deficient_covariances():
    from scrabble_gan_amd.fidelity import frechet_from_moments
    rng = np.random.default_rng(1)
    xa, xb = rng.standard_normal((8, 32)), rng.standard_normal((8, 32)) + 0.5        # 8 samples in D = 32: rank 7
    (m1, c1), (m2, c2) = FR.cov_ref(xa), FR.cov_ref(xb)
    assert np.linalg.matrix_rank(c1) == 7
    d2 = frechet_from_moments(m1, c1, m2, c2)
    bound = 1e-10 * (np.trace(c1) + np.trace(c2) + np.sum((m1 - m2) ** 2))
    assert np.isfinite(d2) and d2 >= -bound
    same = frechet_from_moments(m1, c1, m1, c1)
    assert np.isfinite(same) and same >= -bound


def test_kid_from_sums_is_the_direct_estimator():
    from scrabble_gan_amd.fidelity import kid_from_sums
    rng = np.random.default_rng(2)
    S, m, D = 3, 7, 5
    x, y = rng.standard_normal((20, D)).astype(np.float32), (rng.standard_normal((15, D)) + 0.3).astype(np.float32)
    ix = np.stack([rng.choice(20, m, replace=False) for _ in range(S)]).astype(np.int32)
    iy = np.stack([rng.choice(15, m, replace=False) for _ in range(S)]).astype(np.int32)
    sums, _ = FR.gram_sums_ref(x, y, ix, iy, 1.0 / D, 1.0, tile=3)
    mean, std = kid_from_sums(sums, m)
    want_mean, want_std, vals = FR.kid_ref(x, y, ix, iy, 1.0 / D, 1.0)
    assert abs(mean - want_mean) <= 1e-12 * abs(want_mean) and abs(std - want_std) <= 1e-12 * abs(want_std), (mean, want_mean, std, want_std)
    with pytest.raises(ValueError):
        kid_from_sums(sums, 1)


def test_subset_drawing():
    from scrabble_gan_amd.fidelity import check_subsets, draw_subsets
    ix, iy, m = draw_subsets(50, 30, subsets=6, subset_size=12, seed=3)
    assert m == 12 and ix.shape == iy.shape == (6, 12) and ix.dtype == iy.dtype == np.int32
    ix2, iy2, _ = draw_subsets(50, 30, subsets=6, subset_size=12, seed=3)
    assert np.array_equal(ix, ix2) and np.array_equal(iy, iy2)                       # seeded
    assert not np.array_equal(ix, draw_subsets(50, 30, subsets=6, subset_size=12, seed=4)[0])
    for rows, n in ((ix, 50), (iy, 30)):
        assert rows.min() >= 0 and rows.max() < n
        assert all(len(set(r.tolist())) == 12 for r in rows)                         # without replacement within a subset
    assert len({tuple(r) for r in ix.tolist()}) == 6                                 # the subsets differ
    ix, iy, m = draw_subsets(9, 5, subsets=2, subset_size=1000, seed=0)              # m clamps to the smaller set
    assert m == 5 and ix.shape == (2, 5) and sorted(iy[0].tolist()) == [0, 1, 2, 3, 4] and ix.max() < 9
    for bad in ((1, 10, 2, 5), (10, 1, 2, 5), (10, 10, 2, 1), (10, 10, 0, 5)):
        with pytest.raises(ValueError):
            draw_subsets(bad[0], bad[1], subsets=bad[2], subset_size=bad[3])
    with pytest.raises(ValueError):
        check_subsets(np.array([[0, 5]], np.int32), 5)
    with pytest.raises(ValueError):
        check_subsets(np.array([[-1, 2]], np.int32), 5)


def test_evaluate_cli_fidelity_arguments():
    from scrabble_gan_amd import evaluate
    base = ["--recognizer-weights", "r/cktp-1", "--synthetic"]
    with pytest.raises(SystemExit):
        evaluate.parse_args(base + ["--fidelity", "100"])                            # needs a generator
    a = evaluate.parse_args(base + ["--fidelity", "100", "--generator-weights", "g/cktp-1", "--real-stats", "real.npz", "--kid-subsets", "10",
                                    "--kid-subset-size", "50"])
    assert (a.fidelity, a.feature_space, a.real_stats, a.kid_subsets, a.kid_subset_size) == (100, "recognizer", "real.npz", 10, 50)
    with pytest.raises(SystemExit):
        evaluate.parse_args(base + ["--fidelity", "100", "--generator-weights", "g", "--feature-space", "discriminator"])
    a = evaluate.parse_args(base + ["--fidelity", "100", "--generator-weights", "g", "--feature-space", "discriminator",
                                    "--discriminator-weights", "d/cktp-1"])
    assert a.feature_space == "discriminator" and a.discriminator_weights == "d/cktp-1"
    a = evaluate.parse_args(["--features-real", "a.npy", "--features-fake", "b.npy"])   # no networks: no --recognizer-weights
    assert a.features_real == "a.npy" and a.features_fake == "b.npy" and a.recognizer_weights is None and a.fidelity == 0
    for bad in (["--features-real", "a.npy"], ["--synthetic"], ["--recognizer-weights", "r"], base + ["--feature-space", "inception"]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(bad)
    off = evaluate.parse_args(base)
    assert off.fidelity == 0 and off.real_stats is None and off.features_real is None


def test_train_loop_surface():
    from scrabble_gan_amd import data_utils as DU, fidelity
    from scrabble_gan_amd.main import build_parser
    assert fidelity.FIDELITY_HEADER == "epoch,n_real,n_fake,frechet,kid,kid_std\n"
    params = inspect.signature(DU.train).parameters
    assert [params[k].default for k in ("fidelity_every", "fidelity_real_batches", "fidelity_samples")] == [0, 8, 256]
    ap = build_parser()
    assert ap.parse_args([]).fidelity_every == 0
    on = ap.parse_args(["--synthetic", "--fidelity-every", "2", "--fidelity-real-batches", "3", "--fidelity-samples", "64"])
    assert (on.fidelity_every, on.fidelity_real_batches, on.fidelity_samples) == (2, 3, 64)


def test_fake_word_batches_are_seeded_and_bucketed():
    from scrabble_gan_amd.fidelity import fake_word_batches
    words = [[[1]], [], [[1, 2, 3], [4, 5, 6]]]
    a, b = fake_word_batches(words, 11, 4, seed=0), fake_word_batches(words, 11, 4, seed=0)
    assert sum(len(x) for x in a) == 11 and all(np.array_equal(p, q) for p, q in zip(a, b))
    assert all(x.dtype == np.int32 and x.ndim == 2 and x.shape[1] in (1, 3) and 1 <= len(x) <= 4 for x in a)
    with pytest.raises(ValueError):
        fake_word_batches([[], []], 3, 4)
