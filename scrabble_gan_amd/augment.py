"""Differentiable augmentation of the discriminator's inputs (DiffAugment, Zhao et al. 2020; not in the reference).

With a few tens of thousands of training words D, a full BigGAN ResNet, can memorise the real set.  The remedy is to show D only
randomly transformed images -- real and generated alike, from the same transform family -- and to back-propagate G's gradient
through the transform (ops.augment / ops.augment_bwd, csrc/augment.hip).  This module is the policy: which transform each
sample gets.  One fp32 row of 12 numbers per sample (the kernels' parameter table, include/scrabble_hip.h):

    c beta | a00 a01 a02 a10 a11 a12 | x0 y0 x1 y1          identity: 1 0 | 1 0 0 0 1 0 | 0 0 0 0

Families (each applied to a sample with probability p, all composed into the sample's one row):
    color        beta ~ U(-0.5, 0.5), c ~ U(0.5, 1.5)                          (brightness offset, contrast about the sample mean)
    translation  integer shifts ty in [-H/8, H/8], tx in [-W/8, W/8]           (constant padding)
    cutout       an H/2 x W/2 rectangle, centre uniform over the image, clipped to it
    affine       shear in x in +-0.3, scales in [0.9, 1.1], about the image centre (handwriting slant and size)

The sampler owns a numpy Generator: it never draws from `random`, numpy's global stream or the models' generators, so a run
with augmentation draws everything else exactly as a run without it.  Data parallel: every rank holds an identically seeded
sampler, draws the rows of the GLOBAL batch and keeps its shard (data_utils.train_step), like the other per-step host draws."""
from __future__ import annotations

import numpy as np

FAMILIES = ("color", "translation", "cutout", "affine")
IDENTITY = np.array([1, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0], np.float32)

# the limits check() enforces; the backward kernel's 3 x 3 search window is derived from the matrix limits (csrc/augment.hip)
CONTRAST = (0.5, 1.5)
BRIGHTNESS = (-0.5, 0.5)
SCALE = (0.9, 1.1)
SHEAR = 0.3
SHIFT_MAX = 65536.0      # |a02|, |a12|: far beyond any image here; keeps the fp32 inverse map within 0.01 pixel


def parse_policy(policy) -> tuple:
    names = tuple(s.strip() for s in policy.split(",") if s.strip()) if isinstance(policy, str) else tuple(policy)
    for s in names:
        if s not in FAMILIES:
            raise ValueError("unknown augmentation family %r (known: %s)" % (s, ", ".join(FAMILIES)))
    return tuple(f for f in FAMILIES if f in names)            # fixed draw order, whatever order the caller wrote


class DiffAugment:
    def __init__(self, policy="color,translation,cutout", p=1.0, seed=0, pad=0.0):
        self.families = parse_policy(policy)
        if not 0.0 <= p <= 1.0:
            raise ValueError("p must be in [0, 1], got %r" % (p,))
        self.p, self.pad, self.seed = float(p), float(pad), int(seed)
        self.rng = np.random.Generator(np.random.PCG64(self.seed))

    def sample(self, n: int, H: int, W: int) -> np.ndarray:
        """-> float32 [n,12]: one row per sample.  Every enabled family draws its gate and its variates for all n samples (so the
        stream position after a call depends on n and the policy only, not on p or the outcomes)."""
        rng = self.rng
        c, beta = np.ones(n), np.zeros(n)
        sxs, sys_, sh = np.ones(n), np.ones(n), np.zeros(n)
        tx, ty = np.zeros(n), np.zeros(n)
        cut = np.zeros((n, 4))
        for fam in self.families:
            on = rng.random(n) < self.p
            if fam == "color":
                b, k = rng.uniform(*BRIGHTNESS, n), rng.uniform(*CONTRAST, n)
                beta, c = np.where(on, b, beta), np.where(on, k, c)
            elif fam == "translation":
                dy, dx = rng.integers(-(H // 8), H // 8 + 1, n), rng.integers(-(W // 8), W // 8 + 1, n)
                ty, tx = np.where(on, dy, ty), np.where(on, dx, tx)
            elif fam == "cutout":
                ch, cw = H // 2, W // 2
                cy, cx = rng.integers(0, H, n), rng.integers(0, W, n)
                y0, x0 = cy - ch // 2, cx - cw // 2
                rect = np.stack([np.clip(x0, 0, W), np.clip(y0, 0, H), np.clip(x0 + cw, 0, W), np.clip(y0 + ch, 0, H)], 1)
                cut = np.where(on[:, None], rect, cut)
            else:
                s, kx, ky = rng.uniform(-SHEAR, SHEAR, n), rng.uniform(*SCALE, n), rng.uniform(*SCALE, n)
                sh, sxs, sys_ = np.where(on, s, sh), np.where(on, kx, sxs), np.where(on, ky, sys_)
        # source = centre + [[sxs, sh], [0, sys]] (output - centre) + (tx, ty); without `affine` the offsets are the integer shifts
        mx, my = (W - 1) / 2.0, (H - 1) / 2.0
        out = np.empty((n, 12), np.float64)
        out[:, 0], out[:, 1] = c, beta
        out[:, 2], out[:, 3], out[:, 4] = sxs, sh, mx - sxs * mx - sh * my + tx
        out[:, 5], out[:, 6], out[:, 7] = 0.0, sys_, my - sys_ * my + ty
        out[:, 8:] = cut
        return out.astype(np.float32)

    def sample_pair(self, n: int, fake_hw, real_hw):
        """The rows of one step: independent tables for the n generated and the n real images (fake first)."""
        return self.sample(n, *fake_hw), self.sample(n, *real_hw)

    def state(self) -> dict:
        return self.rng.bit_generator.state

    def set_state(self, st: dict) -> None:
        self.rng.bit_generator.state = st

    # the state as one int64 tensor-able list (PCG64: 128-bit state and increment as four 32-bit limbs each, has_uint32, uinteger)
    def state_words(self) -> list:
        st = self.state()
        assert st["bit_generator"] == "PCG64"
        limbs = lambda v: [(v >> (32 * k)) & 0xffffffff for k in range(4)]
        return limbs(st["state"]["state"]) + limbs(st["state"]["inc"]) + [int(st["has_uint32"]), int(st["uinteger"])]

    def set_state_words(self, words) -> None:
        w = [int(v) for v in words]
        join = lambda l: sum(v << (32 * k) for k, v in enumerate(l))
        self.set_state({"bit_generator": "PCG64", "state": {"state": join(w[0:4]), "inc": join(w[4:8])}, "has_uint32": w[8], "uinteger": w[9]})

    @staticmethod
    def check(params) -> None:
        """Raises ValueError for a table with a row outside the families' limits.  ops.augment_bwd's search window relies on the
        matrix limits: run tables from elsewhere through this before they reach the kernels."""
        p = np.asarray(params, np.float32)
        if p.ndim != 2 or p.shape[1] != 12:
            raise ValueError("params must be [n,12], got %s" % (p.shape,))
        f = np.float32
        bad = ~np.isfinite(p).all(1)
        bad |= (p[:, 0] < f(CONTRAST[0])) | (p[:, 0] > f(CONTRAST[1])) | (p[:, 1] < f(BRIGHTNESS[0])) | (p[:, 1] > f(BRIGHTNESS[1]))
        bad |= (p[:, 2] < f(SCALE[0])) | (p[:, 2] > f(SCALE[1])) | (p[:, 6] < f(SCALE[0])) | (p[:, 6] > f(SCALE[1]))
        bad |= (np.abs(p[:, 3]) > f(SHEAR)) | (p[:, 5] != 0)
        bad |= (np.abs(p[:, 4]) > f(SHIFT_MAX)) | (np.abs(p[:, 7]) > f(SHIFT_MAX))
        bad |= (p[:, 8:] != np.round(p[:, 8:])).any(1)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError("augmentation row %d is outside the limits (contrast %s, brightness %s, scales %s, |shear| <= %s, a10 == 0, "
                             "|offset| <= %g, integer cutout): %s" % (i, CONTRAST, BRIGHTNESS, SCALE, SHEAR, SHIFT_MAX, p[i].tolist()))


def step_tables(augment, n_global: int, fake_hw, real_hw, device, reducer=None):
    """What train_step hands the kernels: (params_fake, params_real, pad) as device tensors of this rank's shard.  `augment` is a
    DiffAugment (drawn here, for the GLOBAL batch, then sharded) or ready device tables (params_fake, params_real[, pad])."""
    import torch
    if isinstance(augment, DiffAugment):
        pf, pr = augment.sample_pair(n_global, fake_hw, real_hw)
        both = torch.from_numpy(np.concatenate([pf, pr], 0)).to(device, non_blocking=True)
        pf, pr = both[:n_global], both[n_global:]
        if reducer is not None and reducer.world_size > 1 and getattr(reducer, "shard_inputs", True):
            pf, pr = reducer.shard(pf), reducer.shard(pr)
        return pf, pr, augment.pad
    if len(augment) not in (2, 3):
        raise TypeError("augment must be a DiffAugment or (params_fake, params_real[, pad])")
    return augment[0], augment[1], float(augment[2]) if len(augment) == 3 else 0.0
