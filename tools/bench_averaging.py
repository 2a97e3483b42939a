"""Cost of the averaged generator's per-step sweep beside the Adam launch over the same buffer (HIP events).
    python tools/bench_averaging.py [--rounds 30] [--inner 10] [--out FILE]
Both sweeps run over flat fp32 buffers the size of G's `store.flat`, filled with random values, from the same build, alternating
in one process: per round `--inner` launches of each between two events, after a warm-up of both.  By byte counts ema_update
moves 12 B per weight (read ema, read p, write ema) against Adam's 28 B (read g; read and write p, m, v); swap_buffers (16 B) is
listed for scale.  Reported per launch: median / min / max over the rounds, the algorithmic GB/s at the median, and the ratio."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrabble_gan_amd import net_architecture as NA, nn, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    NA.configure(device=dev, seed=0)
    nn.FAST_INIT = True                     # only the size of the buffer matters here
    try:
        n = NA.make_generator(128, (32, 160, 1), (32, 8192), None, "B3", 52, vis_model=False).store.flat.numel()
    finally:
        nn.FAST_INIT = False
    gen = torch.Generator(device=dev).manual_seed(0)
    p, g, ema = (torch.randn(n, device=dev, generator=gen) * 0.05 for _ in range(3))
    m, v = torch.zeros(n, device=dev), torch.rand(n, device=dev, generator=gen) * 1e-4
    other = torch.randn(n, device=dev, generator=gen)
    sweeps = [("ema_update (12 B/weight)", 12, lambda: ops.ema_update(ema, p, 1e-4)),
              ("adam_update (28 B/weight)", 28, lambda: ops.adam_update(p, g, m, v, 2e-4, 0.0, 0.999)),
              ("swap_buffers (16 B/weight)", 16, lambda: ops.swap_buffers(ema, other))]
    for _ in range(3):                      # warm-up: code objects loaded, clocks up
        for _, _, fn in sweeps:
            for _ in range(args.inner):
                fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _, _ in sweeps}
    for _ in range(args.rounds):
        for name, _, fn in sweeps:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / args.inner)
    lines = ["buffer: %d fp32 weights (%.1f MB), %d rounds x %d launches, alternating" % (n, n * 4 / 1e6, args.rounds, args.inner),
             "%-30s %10s %10s %10s %10s" % ("per launch (ms)", "median", "min", "max", "GB/s")]
    med = {}
    for name, nbytes, _ in sweeps:
        t = times[name]
        med[name] = statistics.median(t)
        lines.append("%-30s %10.4f %10.4f %10.4f %10.0f" % (name, med[name], min(t), max(t), nbytes * n / (med[name] * 1e-3) / 1e9))
    ratio = med[sweeps[0][0]] / med[sweeps[1][0]]
    lines.append("ema_update / adam_update = %.3f of the Adam launch (by bytes: 12 / 28 = %.3f)" % (ratio, 12 / 28))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
