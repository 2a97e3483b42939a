"""Cost of the differentiable augmentation (HIP events).
    python tools/bench_augment.py [--batch 128] [--rounds 30] [--inner 10] [--steps 5] [--out FILE]
(1) ops.augment + ops.augment_bwd on a [batch, 32, 160, 1] tensor with sampler rows of all four families, beside ops.add -- the existing
bandwidth sweep -- over the SAME number of bytes: the pair moves 16 B per pixel (x read, y written; dy read, dx written), ops.add
12 B per element, so it runs over 4/3 as many elements.  Alternating rounds in one process, per round `--inner` launches between two
events after a warm-up; median / min / max per launch and the algorithmic GB/s at the median.
(2) train_step images/s at that batch (word length 10, fp32) without and with `augment=`, alternating steps from one set of weights."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrabble_gan_amd import data_utils as DU, net_architecture as NA, net_loss, nn, ops, optimizers  # noqa: E402
from scrabble_gan_amd.augment import DiffAugment  # noqa: E402


def kernels(args, dev, lines):
    B, H, W = args.batch, 32, 160
    n = B * H * W
    gen = torch.Generator(device=dev).manual_seed(0)
    x, dy = torch.rand(B, H, W, 1, device=dev, generator=gen) * 2 - 1, torch.randn(B, H, W, 1, device=dev, generator=gen)
    params = torch.from_numpy(DiffAugment("color,translation,cutout,affine", seed=0).sample(B, H, W)).to(dev)
    n_add = (4 * n // 3 + 3) // 4 * 4
    a, b, out = (torch.randn(n_add, device=dev, generator=gen) for _ in range(3))

    def pair():
        _, ctx = ops.augment(x, params)
        ops.augment_bwd(dy, ctx)

    sweeps = [("augment fwd + bwd", 16 * n, pair),
              ("augment fwd", 8 * n, lambda: ops.augment(x, params)),
              ("ops.add, same bytes as the pair", 12 * n_add, lambda: ops.add(a, b, out=out))]
    for _ in range(3):
        for _, _, fn in sweeps:
            for _ in range(args.inner):
                fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in sweeps}
    for _ in range(args.rounds):
        for name, _, fn in sweeps:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.inner)
    lines.append("[%d, %d, %d, 1] fp32 (%.2f MB per tensor), %d rounds x %d launches, alternating" % (B, H, W, n * 4 / 1e6, args.rounds, args.inner))
    lines.append("%-34s %10s %10s %10s %10s" % ("per call (ms)", "median", "min", "max", "GB/s"))
    med = {}
    for name, nbytes, _ in sweeps:
        t = times[name]
        med[name] = statistics.median(t)
        lines.append("%-34s %10.4f %10.4f %10.4f %10.0f" % (name, med[name], min(t), max(t), nbytes / (med[name] * 1e-3) / 1e9))
    lines.append("augment fwd + bwd / ops.add over the same bytes = %.2f" % (med[sweeps[0][0]] / med[sweeps[2][0]]))


def steps(args, dev, lines):
    B, L = args.batch, 10
    nn.FAST_INIT = True                     # timing only: skip the QR initialisers
    try:
        G = NA.make_generator(128, (32, 160, 1), (32, 8192), None, "B3", 52, vis_model=False)
        D = NA.make_discriminator((32, 160, 1), None, "B1", vis_model=False)
        R = NA.make_recognizer((32, 160, 1), None, 53, vis_model=False)
        S = NA.make_style_promoter((32, 160, 1), None, "B1", vis_model=False)
    finally:
        nn.FAST_INIT = False
    gan = NA.make_gan(G, D, R, S, vis_model=False)
    images, labels, my_imgs = DU.synthetic_batch(B, L, seed=1)
    words = DU.synthetic_random_words(10, 200, seed=1)
    fake = np.array(words[L - 1][:B], np.int32)
    dv = [torch.from_numpy(t).to(dev) for t in (images, labels, my_imgs, fake)]
    opts = [optimizers.Adam(2e-4, 0.0, 0.999) for _ in range(4)]
    aug = DiffAugment("color,translation,cutout", seed=0)

    def step(augment):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        DU.train_step(0, 0, 1, dv[0], dv[1], D, R, S, gan, opts[0], opts[1], opts[2], opts[3], dv[2], B, 128, net_loss.hinge, 1, 1, words, 10, "",
                      fake_labels=dv[3], verbose=False, sync=False, augment=augment)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _ in range(2):
        step(None), step(aug)
    t_off, t_on = [], []
    for _ in range(args.steps):
        t_off.append(step(None))
        t_on.append(step(aug))
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    lines.append("train_step, batch %d, word length %d, fp32, %d alternating steps after 2 warm-up steps each (host clock around a synchronised step)" % (B, L, args.steps))
    lines.append("augment off: median %.2f ms (min %.2f, max %.2f) = %.1f images/s" % (m_off * 1e3, min(t_off) * 1e3, max(t_off) * 1e3, B / m_off))
    lines.append("augment on : median %.2f ms (min %.2f, max %.2f) = %.1f images/s  (color,translation,cutout)" % (m_on * 1e3, min(t_on) * 1e3, max(t_on) * 1e3, B / m_on))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    NA.configure(device=dev, seed=0)
    lines = []
    kernels(args, dev, lines)
    lines.append("")
    steps(args, dev, lines)
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
