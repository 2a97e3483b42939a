"""Cost of reading the recognizer beside the recognizer's own forward pass (HIP events, median of synchronised repeats).
    python tools/bench_decode.py [--iters 20] [--words 10000] [--out FILE]
Shapes: (B = 128, L = 10 -> T = 39) and (B = 256, L = 23 -> T = 91), C = 53; the lexicon has `--words` words of 1..10 characters
and is scored at the first shape.  Per shape: R.logits (for scale), transcribe = R.logits + greedy decode, the decode kernel
alone, edit distance + sums; at the first shape: ctc_log_probs, ctc_score_words alone and R.score_words end to end."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrabble_gan_amd import net_architecture as NA, ops  # noqa: E402


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
    ap.add_argument("--words", type=int, default=10000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    NA.configure(device=dev, seed=0)
    R = NA.make_recognizer((32, 160, 1), None, 53, vis_model=False)
    rng = np.random.default_rng(0)
    seen = set()
    while len(seen) < args.words:
        seen.add(tuple(int(c) for c in rng.integers(0, 52, int(rng.integers(1, 11)))))
    lex = sorted(seen)
    words = np.full((len(lex), 10), -1, np.int32)
    for i, w in enumerate(lex):
        words[i, :len(w)] = w
    words_d = torch.from_numpy(words).to(dev)
    wlen_d = torch.from_numpy(np.array([len(w) for w in lex], np.int32)).to(dev)
    lines = ["%-44s %10s %10s %10s" % ("what (ms)", "median", "min", "max")]

    def row(name, fn):
        lines.append("%-44s %10.3f %10.3f %10.3f" % ((name,) + median_ms(fn, args.iters)))
        print(lines[-1], flush=True)

    for B, L in ((128, 10), (256, 23)):
        x = torch.from_numpy(rng.uniform(-1, 1, (B, 32, 16 * L, 1)).astype(np.float32)).to(dev)
        ref = torch.from_numpy(rng.integers(0, 52, (B, L)).astype(np.int32)).to(dev)
        ref_len = torch.full((B,), L, device=dev, dtype=torch.int32)
        sums = torch.zeros(4, device=dev, dtype=torch.float64)
        logits = R.logits(x)
        T = logits.shape[1]
        tag = "B=%d L=%d T=%d: " % (B, L, T)
        row(tag + "R.logits", lambda: R.logits(x))
        row(tag + "R.transcribe", lambda: R.transcribe(x))
        row(tag + "ctc_greedy_decode alone", lambda: ops.ctc_greedy_decode(logits))
        hyp, hyp_len, _ = ops.ctc_greedy_decode(logits)
        row(tag + "edit_distance + legibility_sums", lambda: ops.legibility_sums(ops.edit_distance(hyp, hyp_len, ref, ref_len), ref_len, sums))
        if (B, L) == (128, 10):
            lp = ops.ctc_log_probs(logits)
            row(tag + "ctc_log_probs", lambda: ops.ctc_log_probs(logits))
            row(tag + "ctc_score_words alone, W=%d" % len(lex), lambda: ops.ctc_score_words(lp, words_d, wlen_d))
            row(tag + "R.score_words, W=%d" % len(lex), lambda: R.score_words(x, words_d, wlen_d))
            row(tag + "ctc_score_words + row argmin", lambda: torch.min(ops.ctc_score_words(lp, words_d, wlen_d), 1))
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
