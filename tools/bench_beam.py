"""Cost of the CTC prefix beam search beside the greedy decode and the recognizer's own forward pass (HIP events, median of
synchronised repeats after warm-up calls).
    python tools/bench_beam.py [--iters 20] [--out FILE]
One shape: B = 256, L = 10 -> T = 39 frames, C = 53, the logits of an untrained recognizer on uniform noise (a flat
distribution: every cut is contested, the worst case for the merge and cut phases).  Rows: R.logits (for scale), ctc_log_probs,
the greedy decode, ops.ctc_beam_decode for beam in {8, 32, 64} without an LM and with a trigram (lm_weight 0.7, len_bonus 0.5),
and the fp64 Python reference (tests/beam_refs.beam_ref, one CPU thread, wall clock) on 8 of the samples at beam 8."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrabble_gan_amd import net_architecture as NA, ops  # noqa: E402
from tests import beam_refs as BR  # noqa: E402


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
    B, L, C = 256, 10, 53
    R = NA.make_recognizer((32, 160, 1), None, C, vis_model=False)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(-1, 1, (B, 32, 16 * L, 1)).astype(np.float32)).to(dev)
    table = BR.log_softmax_rows(rng.standard_normal((C * C, C)) * 2).astype(np.float32)
    lm = torch.from_numpy(table).to(dev)
    logits = R.logits(x)
    T = logits.shape[1]
    lp = ops.ctc_log_probs(logits)
    tag = "B=%d L=%d T=%d C=%d: " % (B, L, T, C)
    lines = ["%-52s %10s %10s %10s" % ("what (ms)", "median", "min", "max")]

    def row(name, fn):
        med, lo, hi = median_ms(fn, args.iters)
        lines.append("%-52s %10.3f %10.3f %10.3f" % (tag + name, med, lo, hi))
        print(lines[-1], flush=True)
        return med

    forward = row("R.logits", lambda: R.logits(x))
    row("ctc_log_probs", lambda: ops.ctc_log_probs(logits))
    row("ctc_greedy_decode", lambda: ops.ctc_greedy_decode(logits))
    worst = 0.0
    for beam in (8, 32, 64):
        row("ctc_beam_decode beam=%d" % beam, lambda: ops.ctc_beam_decode(lp, beam=beam))
        worst = row("ctc_beam_decode beam=%d + trigram" % beam,
                    lambda: ops.ctc_beam_decode(lp, beam=beam, lm=lm, lm_order=3, lm_weight=0.7, len_bonus=0.5))
    host = lp[:8].double().cpu().numpy()
    t0 = time.perf_counter()
    for b in range(8):
        BR.beam_ref(host[b], 8, table, 3, 0.7, 0.5)
    lines.append("%-52s %10.3f" % ("beam_ref (Python fp64, CPU) beam=8 + trigram, 8 samples", (time.perf_counter() - t0) * 1e3))
    print(lines[-1], flush=True)
    lines.append("beam 64 + trigram costs %.2f x the recognizer's forward pass at this batch" % (worst / forward))
    print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
