"""Cost of the fidelity statistics beside the recognizer's own forward pass (HIP events, median of synchronised repeats).
    python tools/bench_fidelity.py [--iters 20] [--out profiles/fidelity_timing.txt]
feature_moments at (n, D) = (128, 512) and (128, 1024); poly_mmd_sums at S = 100 subsets of m = 1000 out of 10 000 rows, D = 512 and
1024; R.features and R.logits at B = 128, L = 10.  The one condition (checked, exit status 1 otherwise): accumulating a batch's
statistics at (128, 1024) costs less than producing the batch's features (R.logits).  The kernel-sums rate counts the fp64
multiply-adds of the 64x64 tiles that are launched (upper triangle for XX / YY) against the device's fp64 matrix peak."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrabble_gan_amd import fidelity, net_architecture as NA, ops  # noqa: E402
from scrabble_gan_amd._lib import lib  # noqa: E402

FP64_MATRIX_PEAK_TFLOPS = 78.6      # MI355X data sheet, fp64 matrix


def median_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    NA.configure(device=dev, seed=0)
    R = NA.make_recognizer((32, 160, 1), None, 53, vis_model=False)
    rng = np.random.default_rng(0)
    lines = ["# python tools/bench_fidelity.py --iters %d  (one MI355X; HIP events, median / min / max of %d synchronised repeats)" % (args.iters, args.iters),
             "%-52s %10s %10s %10s" % ("what (ms)", "median", "min", "max")]
    med = {}

    def row(name, fn):
        med[name] = median_ms(fn, args.iters)
        lines.append("%-52s %10.3f %10.3f %10.3f" % ((name,) + med[name]))
        print(lines[-1], flush=True)

    for n, D in ((128, 512), (128, 1024)):
        x = torch.from_numpy(rng.standard_normal((n, D)).astype(np.float32)).to(dev)
        s = torch.zeros(D, device=dev, dtype=torch.float64)
        o = torch.zeros(D, D, device=dev, dtype=torch.float64)
        row("feature_moments n=%d D=%d" % (n, D), lambda: ops.feature_moments(x, s, o))
        row("feature_cov D=%d" % D, lambda: ops.feature_cov(s, o, 1000.0))
    S, m, N = 100, 1000, 10000
    ix, iy, _ = fidelity.draw_subsets(N, N, S, m, 0)
    ixd, iyd = torch.from_numpy(ix).to(dev), torch.from_numpy(iy).to(dev)
    tiles = lib().sg_poly_mmd_workspace_doubles(S, m)
    for D in (512, 1024):
        a = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32)).to(dev)
        b = torch.from_numpy(rng.standard_normal((N, D)).astype(np.float32)).to(dev)
        name = "poly_mmd_sums S=%d m=%d D=%d" % (S, m, D)
        row(name, lambda: ops.poly_mmd_sums(a, b, ixd, iyd))
        tf = tiles * 64 * 64 * D * 2 / (med[name][0] * 1e-3) / 1e12
        lines.append("    %d tiles of 64x64x%d: %.2f TFLOP/s fp64 = %.1f %% of the %.1f TFLOP/s fp64 matrix peak"
                     % (tiles, D, tf, 100 * tf / FP64_MATRIX_PEAK_TFLOPS, FP64_MATRIX_PEAK_TFLOPS))
        print(lines[-1], flush=True)
    B, L = 128, 10
    img = torch.from_numpy(rng.uniform(-1, 1, (B, 32, 16 * L, 1)).astype(np.float32)).to(dev)
    row("B=%d L=%d: R.logits" % (B, L), lambda: R.logits(img))
    row("B=%d L=%d: R.features" % (B, L), lambda: R.features(img))
    ratio = med["feature_moments n=128 D=1024"][0] / med["B=128 L=10: R.logits"][0]
    lines.append("feature_moments (128, 1024) / R.logits (B = 128, L = 10) = %.3f (must stay below 1)" % ratio)
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")
    return 0 if ratio < 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
