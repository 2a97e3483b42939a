"""Character / word error rates of a trained recognizer, and what it reads from a trained generator.

    python -m scrabble_gan_amd.evaluate --recognizer-weights run/checkpoints/recognizer/15/cktp-15 [--my-rec] \
        (--data DIR | --synthetic) [--batches 20] [--batch-size 64] [--lexicon words.txt] \
        [--generator-weights run/checkpoints/generator/15/cktp-15 --words machine learning]

`--data DIR` is the bucket-folder layout the train loop reads (<DIR>/<L>/<name>.png + .txt); `--synthetic` takes the
uniform-noise batches of `main.py --synthetic` (no dataset at hand: the rates then only show that the path runs).
With `--lexicon FILE` (one word per line) every image is also read as the lexicon word of lowest CTC cost.  With
`--generator-weights` each of `--words` is rendered in inference mode and read back.  Prints ONE JSON line:
{cer, wer, n_words, n_chars[, cer_lexicon, wer_lexicon][, read_back: [{target, read, distance}], cer_fake, wer_fake]}."""
from __future__ import annotations

import argparse
import itertools
import json

import numpy as np

CHAR_VEC = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--recognizer-weights", required=True, help="checkpoint prefix (without .safetensors)")
    ap.add_argument("--my-rec", action="store_true", help="the BiLSTM recognizer (make_my_recognizer)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--data", default=None, metavar="DIR", help="bucket folders <DIR>/<L>/<name>.png + .txt")
    src.add_argument("--synthetic", action="store_true", help="synthetic batches (no dataset at hand)")
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--bucket-size", type=int, default=10, help="longest word length read from --data / drawn by --synthetic")
    ap.add_argument("--lexicon", default=None, metavar="FILE", help="one word per line: also report the lexicon-constrained read")
    ap.add_argument("--generator-weights", default=None, help="generator checkpoint prefix: read back --words")
    ap.add_argument("--words", nargs="+", default=["machine", "learning"])
    ap.add_argument("--char-vec", default=CHAR_VEC)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.batches < 1 or args.batch_size < 1:
        ap.error("--batches and --batch-size must be positive")
    return args


def read_lexicon(path, char_vec):
    """One word per line; blank lines dropped, duplicates dropped (first occurrence kept)."""
    seen, out = set(), []
    with open(path) as f:
        for line in f:
            w = line.strip()
            if w and w not in seen:
                if any(c not in char_vec for c in w):
                    raise ValueError("lexicon word %r has characters outside the character vector" % w)
                seen.add(w)
                out.append(w)
    if not out:
        raise ValueError("%s holds no words" % path)
    return out


def main(argv=None):
    args = parse_args(argv)
    import torch
    from . import legibility, net_architecture as NA
    NA.configure(device=torch.device(args.device))
    in_dim, n_classes = (32, 160, 1), len(args.char_vec)
    factory = NA.make_my_recognizer if args.my_rec else NA.make_recognizer
    R = factory(in_dim, None, n_classes + 1, vis_model=False)
    R.load_weights(args.recognizer_weights)
    if args.synthetic:
        from .main import synthetic_dataset
        dataset = synthetic_dataset(args.batch_size, in_dim, args.bucket_size, n_classes)
    else:
        from .data_io import load_prepare_data
        dataset = load_prepare_data(in_dim, args.batch_size, args.data.rstrip("/") + "/", args.char_vec, args.bucket_size)
    lexicon = read_lexicon(args.lexicon, args.char_vec) if args.lexicon else None
    out = legibility.evaluate_recognizer(R, itertools.islice(dataset, args.batches), args.char_vec, lexicon)
    if args.generator_weights:
        G = NA.make_generator(128, in_dim, (32, 8192), None, "B3", n_classes, vis_model=False)
        G.load_weights(args.generator_weights)
        style = np.random.default_rng(0).uniform(-1, 1, (max(1, min(len(args.words), 16)),) + in_dim).astype(np.float32)
        rb = legibility.read_back(G, R, style, args.words, args.char_vec)
        out["read_back"] = rb
        out["cer_fake"] = sum(r["distance"] for r in rb) / max(1, sum(len(r["target"]) for r in rb))
        out["wer_fake"] = sum(r["distance"] != 0 for r in rb) / len(rb)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
