"""Do G's words look like the real handwriting?  Frechet and kernel distances between real and generated words.

legibility.py tells whether G's words can be READ; a generator that collapses to one tidy hand scores best there.  This module
compares the DISTRIBUTIONS of real and generated words in a feature space:

    FeatureStats(D, device)                         streaming fp64 sum / outer-product sums of feature rows (ops.feature_moments)
    frechet_from_moments(mu1, c1, mu2, c2)          |mu1 - mu2|^2 + tr c1 + tr c2 - 2 tr (c1 c2)^(1/2)               (FID's formula)
    kernel_distance(feats_a, feats_b, ...)          unbiased MMD^2 with k(a,b) = (a.b / D + 1)^3 over random subsets (KID's formula)
    evaluate_fidelity(generator, feature_model, real_batches, style, fake_labels_batches, space=...)
    fidelity_from_features(a, b)                    the same two numbers from two precomputed [N,D] arrays

Feature spaces.  No Inception network is part of this project, so the space is one of the project's own networks: "recognizer"
(default) -- `RecognizerModel.features`, the mean over the frames of what R's Dense layer reads; R only ever trains on real words --
or "discriminator" -- `DiscriminatorModel.features`, the trunk's pooled 1024-vector, with ONE fixed set of NonLocalBlock kernels
(drawn here from a generator of this module's own) for every batch of both image sets.  Both pool over the width, so words of
every length land in one space.  NUMBERS IN THESE SPACES ARE NOT COMPARABLE WITH THE INCEPTION-BASED FID / KID OF PAPERS; they
compare checkpoints and settings of this project with each other.  `fidelity_from_features` takes features exported elsewhere
(Inception pool3, say) and applies the published formulas to them.

The statistics are fp64 and bitwise reproducible (csrc/fidelity.hip: exact products on the fp64 matrix cores, fixed summation
order, no atomics).  The matrix square root of the Frechet distance stays on the host: it runs once per evaluation on a D x D
matrix, and the symmetric eigenvalue route used here stays finite and non-negative for singular covariances (n < D)."""
from __future__ import annotations

import os
from typing import Iterable, Optional

import numpy as np
import torch

from . import nn, ops
from .legibility import preserved_rng

FIDELITY_HEADER = "epoch,n_real,n_fake,frechet,kid,kid_std\n"
SPACES = ("recognizer", "discriminator")
NL_SEED = 20240229          # the discriminator space's fixed NonLocalBlock kernels
_CHUNK = 8192               # rows per feature_moments call when whole arrays are given


class FeatureStats:
    """n, sum fp64 [D] and outer fp64 [D,D] = sum of x^T x of the feature rows seen so far, on the device.  Additive: `merge` of the
    statistics of two halves (or, later, an all-reduce over ranks) is the statistics of the whole."""

    def __init__(self, D: int, device):
        if not (1 <= int(D) <= ops.MAX_FEATURE_DIM):
            raise ValueError("feature dimension %r outside [1, %d]" % (D, ops.MAX_FEATURE_DIM))
        self.D, self.device, self.n = int(D), torch.device(device), 0
        self.sum = torch.zeros(self.D, device=self.device, dtype=torch.float64)
        self.outer = torch.zeros(self.D, self.D, device=self.device, dtype=torch.float64)

    def update(self, feats) -> "FeatureStats":
        """Add fp32 rows [n, D] (a device tensor)."""
        if feats.dim() != 2 or feats.shape[1] != self.D:
            raise ValueError("features %s: expected [n, %d]" % (tuple(feats.shape), self.D))
        for lo in range(0, feats.shape[0], _CHUNK):
            ops.feature_moments(feats[lo:lo + _CHUNK], self.sum, self.outer)
        self.n += int(feats.shape[0])
        return self

    def merge(self, other: "FeatureStats") -> "FeatureStats":
        if other.D != self.D:
            raise ValueError("cannot merge statistics of dimensions %d and %d" % (self.D, other.D))
        self.sum += other.sum.to(self.device)
        self.outer += other.outer.to(self.device)
        self.n += other.n
        return self

    def moments(self):
        """-> (mean [D], cov [D,D]) as fp64 numpy (unbiased covariance); one device-to-host copy."""
        if self.n < 2:
            raise ValueError("a covariance needs at least 2 rows, got %d" % self.n)
        mean, cov = ops.feature_cov(self.sum, self.outer, float(self.n))
        flat = torch.cat([mean, cov.reshape(-1)]).cpu().numpy()
        return flat[:self.D].copy(), flat[self.D:].reshape(self.D, self.D).copy()

    def save(self, path: str) -> None:
        with open(path, "wb") as f:          # (a file object: numpy appends no suffix to the name)
            np.savez(f, n=np.int64(self.n), sum=self.sum.cpu().numpy(), outer=self.outer.cpu().numpy())

    @classmethod
    def load(cls, path: str, device) -> "FeatureStats":
        with np.load(path) as z:
            n, s, o = int(z["n"]), np.asarray(z["sum"], np.float64), np.asarray(z["outer"], np.float64)
        if s.ndim != 1 or o.shape != (s.shape[0], s.shape[0]) or n < 0:
            raise ValueError("%s does not hold feature statistics (n, sum [D], outer [D,D])" % path)
        st = cls(s.shape[0], device)
        st.n = n
        st.sum.copy_(torch.from_numpy(s))
        st.outer.copy_(torch.from_numpy(o))
        return st


def frechet_from_moments(mu1, c1, mu2, c2) -> float:
    """Frechet distance between N(mu1, c1) and N(mu2, c2), fp64 numpy.  tr (c1 c2)^(1/2) = sum of the square roots of the
    eigenvalues of the symmetric M = c1^(1/2) c2 c1^(1/2), with c1^(1/2) from eigh(c1) and eigenvalues that are zero to within
    the solver's error (negative ones among them) set to 0: finite and non-negative up to rounding for singular covariances too."""
    mu1, mu2 = np.asarray(mu1, np.float64), np.asarray(mu2, np.float64)
    c1, c2 = np.asarray(c1, np.float64), np.asarray(c2, np.float64)
    if mu1.ndim != 1 or mu2.shape != mu1.shape or c1.shape != (mu1.shape[0],) * 2 or c2.shape != c1.shape:
        raise ValueError("moments of shapes %s %s %s %s" % (mu1.shape, c1.shape, mu2.shape, c2.shape))
    def clamped(ev):
        # an eigenvalue below the solver's own error (D eps |matrix|, the threshold of numpy's matrix_rank) is a zero of a singular
        # matrix; its square root would put sqrt(eps) -- eight digits, not sixteen -- into the result for every missing rank
        ev = ev.copy()
        ev[ev < len(ev) * np.finfo(np.float64).eps * max(ev.max(), 0.0)] = 0.0
        return ev

    w, v = np.linalg.eigh((c1 + c1.T) / 2)
    root1 = (v * np.sqrt(clamped(w))) @ v.T
    m = root1 @ ((c2 + c2.T) / 2) @ root1
    tr_root = np.sqrt(clamped(np.linalg.eigvalsh((m + m.T) / 2))).sum()
    d = mu1 - mu2
    return float(d @ d + np.trace(c1) + np.trace(c2) - 2.0 * tr_root)


def kid_from_sums(sums, m: int):
    """sums [S,3] = {sum_{i!=j} k(X_i,X_j), sum_{i!=j} k(Y_i,Y_j), sum_{i,j} k(X_i,Y_j)} per subset of m rows each -> (mean, std) over the
    subsets of the unbiased MMD^2 estimate (sxx + syy) / (m (m - 1)) - 2 sxy / m^2."""
    m = int(m)
    if m < 2:
        raise ValueError("the unbiased estimator needs subsets of at least 2 rows, got %d" % m)
    s = np.asarray(sums, np.float64).reshape(-1, 3)
    est = (s[:, 0] + s[:, 1]) / (m * (m - 1.0)) - 2.0 * s[:, 2] / (float(m) * m)
    return float(est.mean()), float(est.std())


def draw_subsets(n_a: int, n_b: int, subsets: int = 100, subset_size: int = 1000, seed: int = 0):
    """Row indices of `subsets` random subsets of m = min(subset_size, n_a, n_b) rows of each set, drawn without replacement within
    a subset from np.random.default_rng(seed) -> (ix int32 [S,m] into a, iy int32 [S,m] into b, m).  Checked here, on the host: the
    kernel cannot check a row index without reading through it."""
    n_a, n_b, subsets = int(n_a), int(n_b), int(subsets)
    m = min(int(subset_size), n_a, n_b)
    if m < 2:
        raise ValueError("kernel distance needs at least 2 rows per set and subset (sets of %d and %d rows, subset size %d)"
                         % (n_a, n_b, subset_size))
    if subsets < 1:
        raise ValueError("at least one subset")
    rng = np.random.default_rng(seed)
    ix, iy = np.empty((subsets, m), np.int32), np.empty((subsets, m), np.int32)
    for s in range(subsets):
        ix[s] = rng.choice(n_a, m, replace=False)
        iy[s] = rng.choice(n_b, m, replace=False)
    check_subsets(ix, n_a)
    check_subsets(iy, n_b)
    return ix, iy, m


def check_subsets(idx, n: int) -> None:
    idx = np.asarray(idx)
    if idx.dtype != np.int32 or idx.ndim != 2 or idx.size == 0 or idx.min() < 0 or idx.max() >= n:
        raise ValueError("subset indices must be int32 [S,m] within [0, %d)" % n)


def kernel_distance(feats_a, feats_b, subsets: int = 100, subset_size: int = 1000, seed: int = 0):
    """KID between two sets of fp32 feature rows on the device: mean and standard deviation over `subsets` random subsets of the
    unbiased MMD^2 estimate with the cubic polynomial kernel (gamma = 1 / D, coef0 = 1).  -> (kid, kid_std)"""
    if feats_a.dim() != 2 or feats_b.dim() != 2 or feats_a.shape[1] != feats_b.shape[1]:
        raise ValueError("features %s and %s: expected [n_a, D] and [n_b, D]" % (tuple(feats_a.shape), tuple(feats_b.shape)))
    ix, iy, m = draw_subsets(feats_a.shape[0], feats_b.shape[0], subsets, subset_size, seed)
    dev = feats_a.device
    sums = ops.poly_mmd_sums(feats_a, feats_b, torch.from_numpy(ix).to(dev), torch.from_numpy(iy).to(dev),
                             gamma=1.0 / feats_a.shape[1], coef0=1.0)
    return kid_from_sums(sums.cpu().numpy(), m)


class FeatureExtractor:
    """images -> fp32 [B, dim] in the space of `model`.  space = "recognizer": model.features(images); "discriminator":
    model.features(images, nl) with ONE set of NonLocalBlock kernels drawn at construction from a fixed seed, so the metric does
    not depend on the per-call re-draw of nl_mode "reference" (and draws nothing from the model's own generator)."""

    def __init__(self, model, space: str = "recognizer"):
        if space not in SPACES:
            raise ValueError("feature space %r: one of %s" % (space, ", ".join(SPACES)))
        if not hasattr(model, "features"):
            raise ValueError("%s has no features() accessor" % type(model).__name__)
        self.model, self.space, self.nl = model, space, None
        if space == "recognizer":
            self.dim = int(model.store.p["dense.w"].shape[0])
        else:
            trunk = model.trunk
            self.dim = int(trunk.cout[-1])
            if trunk.attn and trunk.nl_mode != "persistent":
                C = trunk.cout[trunk.names.index(trunk.attn[0])]
                self.nl = nn.nonlocal_weights(C, torch.Generator().manual_seed(NL_SEED), model.device)

    def __call__(self, images):
        if self.space == "recognizer":
            return self.model.features(images)
        return self.model.features(images, nl=self.nl)


def _images_of(batch):
    return batch[0] if isinstance(batch, (tuple, list)) else batch


def evaluate_fidelity(generator, feature_model, real_batches: Optional[Iterable], style, fake_labels_batches: Iterable,
                      space: str = "recognizer", real_stats: Optional[FeatureStats] = None, subsets: int = 100, subset_size: int = 1000,
                      seed: int = 0) -> dict:
    """Frechet and kernel distance between real words and G's inference-mode rendering of `fake_labels_batches` (int [B,L] arrays,
    one word length per batch; word i of a batch in the style of image (words so far + i) modulo len(style)).
    `real_batches`: images [B,32,16L,1] or (images, labels) pairs.  `real_stats`: the real set's FeatureStats from an earlier pass
    -- the Frechet distance then uses them instead of the statistics of `real_batches`, which may be None (no kernel distance then:
    it needs the rows themselves); an EMPTY FeatureStats is filled from `real_batches` for the caller to save.  Runs under legibility.preserved_rng: a training run draws what it would have drawn anyway.
    -> {frechet, kid, kid_std, n_real, n_fake, feature_space, dim}"""
    extract = FeatureExtractor(feature_model, space)
    dev = feature_model.device
    style = np.asarray(style, np.float32) if not torch.is_tensor(style) else style
    with preserved_rng(generator, feature_model):
        real_feats = [extract(_images_of(b)) for b in real_batches] if real_batches is not None else []
        fake_feats, done = [], 0
        for labels in fake_labels_batches:
            labels = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels, np.int32)
            sel = [(done + i) % len(style) for i in range(len(labels))]
            fake_feats.append(extract(generator([style[sel], labels], training=False)))
            done += len(labels)
    if not fake_feats or (real_stats is None and not real_feats):
        raise ValueError("evaluate_fidelity needs generated words and real words (or the real set's statistics)")
    fake = torch.cat(fake_feats, 0)
    real = torch.cat(real_feats, 0) if real_feats else None
    s_fake = FeatureStats(extract.dim, dev).update(fake)
    s_real = real_stats if real_stats is not None else FeatureStats(extract.dim, dev)
    if s_real.D != extract.dim:
        raise ValueError("real statistics have dimension %d, the %s space has %d" % (s_real.D, space, extract.dim))
    if s_real.n == 0:
        if real is None:
            raise ValueError("empty real statistics and no real words")
        s_real.update(real)
    out = {"frechet": frechet_from_moments(*s_real.moments(), *s_fake.moments()), "kid": None, "kid_std": None,
           "n_real": s_real.n, "n_fake": s_fake.n, "feature_space": space, "dim": extract.dim}
    if real is not None:
        out["kid"], out["kid_std"] = kernel_distance(real, fake, subsets, subset_size, seed)
    return out


def fidelity_from_features(a, b, subsets: int = 100, subset_size: int = 1000, seed: int = 0, device=None) -> dict:
    """The same numbers from two precomputed feature arrays [N_a, D], [N_b, D] (e.g. np.load of exported Inception pool3
    features): `a` is the real set.  The statistics still run on the device."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("feature arrays %s and %s: expected [N_a, D] and [N_b, D]" % (a.shape, b.shape))
    dev = torch.device(device if device is not None else "cuda:0")
    ta, tb = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    sa, sb = FeatureStats(a.shape[1], dev).update(ta), FeatureStats(a.shape[1], dev).update(tb)
    kid, kid_std = kernel_distance(ta, tb, subsets, subset_size, seed)
    return {"frechet": frechet_from_moments(*sa.moments(), *sb.moments()), "kid": kid, "kid_std": kid_std, "n_real": sa.n, "n_fake": sb.n,
            "feature_space": "file", "dim": int(a.shape[1])}


def fake_word_batches(random_words, n_words: int, batch_size: int, seed: int = 0):
    """`n_words` words drawn from the bucketed word lists (random_words[L - 1] = index lists of L characters) with a generator of
    its own, grouped into batches of one word length -> list of int32 [B,L] arrays, B <= batch_size."""
    rng = np.random.default_rng(seed)
    buckets = [k for k, b in enumerate(random_words) if len(b)]
    if not buckets or n_words < 1:
        raise ValueError("no words to draw from")
    by_len = {}
    for _ in range(int(n_words)):
        k = buckets[int(rng.integers(len(buckets)))]
        by_len.setdefault(k, []).append(random_words[k][int(rng.integers(len(random_words[k])))])
    out = []
    for k in sorted(by_len):
        rows = np.asarray(by_len[k], np.int32)
        out += [rows[lo:lo + batch_size] for lo in range(0, len(rows), batch_size)]
    return out


class EpochFidelity:
    """The train loop's hook (`--fidelity-every`).  The first `real_batches` training batches the loop hands to `observe` are kept
    (the images, not their features: R keeps training, and both sets must be seen by the SAME network at every evaluation), the
    generated words and their styles are drawn once from a generator of this object's own; `evaluate` appends nothing itself and
    draws nothing from the streams training uses."""

    def __init__(self, random_words, my_imgs, batch_size: int, real_batches: int = 8, samples: int = 256, subsets: int = 100,
                 subset_size: int = 1000, seed: int = 0):
        self.want, self.kept = int(real_batches), []
        self.labels = fake_word_batches(random_words, samples, batch_size, seed)
        rng = np.random.default_rng(seed + 1)
        self.style_idx = [int(i) for i in rng.integers(0, len(my_imgs), min(int(samples), 64))]
        self.my_imgs, self.subsets, self.subset_size, self.seed = my_imgs, subsets, subset_size, seed

    def observe(self, images) -> None:
        if len(self.kept) < self.want:
            self.kept.append(images.clone() if torch.is_tensor(images) else np.array(images, copy=True))

    def evaluate(self, generator, recognizer) -> dict:
        imgs = [self.my_imgs[i] for i in self.style_idx]
        style = torch.stack(imgs, 0) if torch.is_tensor(imgs[0]) else np.stack([np.asarray(m) for m in imgs], 0)
        return evaluate_fidelity(generator, recognizer, self.kept, style, self.labels, space="recognizer", subsets=self.subsets,
                                 subset_size=self.subset_size, seed=self.seed)


def append_csv(path: str, epoch: int, res: dict) -> None:
    new = not os.path.exists(path)
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "a") as f:
        if new:
            f.write(FIDELITY_HEADER)
        f.write(",".join(str(v) for v in (epoch, res["n_real"], res["n_fake"], res["frechet"], res["kid"], res["kid_std"])) + "\n")
