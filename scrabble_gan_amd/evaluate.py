"""Character / word error rates of a trained recognizer, and what it reads from a trained generator.

    python -m scrabble_gan_amd.evaluate --recognizer-weights run/checkpoints/recognizer/15/cktp-15 [--my-rec] \
        (--data DIR | --synthetic) [--batches 20] [--batch-size 64] [--lexicon words.txt] \
        [--beam 16 [--lm-corpus words.txt | --lm lm.npz] [--lm-order 2] [--lm-weight 0.5] [--len-bonus 0.0]] \
        [--generator-weights run/checkpoints/generator/15/cktp-15 --words machine learning]
        [--fidelity 10000 [--feature-space recognizer|discriminator] [--discriminator-weights PREFIX] [--real-stats real.npz]
         [--kid-subsets 100] [--kid-subset-size 1000]]
    python -m scrabble_gan_amd.evaluate --features-real A.npy --features-fake B.npy

`--data DIR` is the bucket-folder layout the train loop reads (<DIR>/<L>/<name>.png + .txt); `--synthetic` takes the
uniform-noise batches of `main.py --synthetic` (no dataset at hand: the rates then only show that the path runs).
With `--lexicon FILE` (one word per line) every image is also read as the lexicon word of lowest CTC cost.  With
`--generator-weights` each of `--words` is rendered in inference mode and read back.  With `--beam W` (W > 0) every image is
also read by a CTC prefix beam search W strings wide (open vocabulary), optionally rescored by a character n-gram LM counted
from `--lm-corpus FILE` (one word per line, order `--lm-order`; words with characters outside `--char-vec` are skipped and
counted on stderr) or loaded from `--lm FILE.npz` (legibility.CharLM.save); `--lm-weight` scales the LM's log-probabilities and
`--len-bonus` is added per character.  Prints ONE JSON line:
{cer, wer, n_words, n_chars[, cer_lexicon, wer_lexicon][, cer_beam, wer_beam]
 [, read_back: [{target, read, distance[, read_beam, distance_beam, score_beam]}], cer_fake, wer_fake[, cer_fake_beam, wer_fake_beam]]
 [, frechet, kid, kid_std, n_real, n_fake, feature_space, dim]}.

`--fidelity N` (with `--generator-weights`) renders N words -- drawn from `--lexicon`, else from the labels of the real batches --
and reports the Frechet and kernel distances (fidelity.py) between the real batches and the renderings in the feature space of
the recognizer (default) or of a discriminator (`--discriminator-weights`).  THESE NUMBERS ARE NOT COMPARABLE WITH INCEPTION-BASED
FID / KID.  `--real-stats FILE.npz`: the real set's statistics are read from FILE if it exists (the Frechet distance then uses
them) and written there otherwise.  `--features-real A.npy --features-fake B.npy` applies the same formulas to two precomputed
[N,D] feature arrays (exported Inception pool3 features, say) and needs no network."""
from __future__ import annotations

import argparse
import itertools
import json

import numpy as np

CHAR_VEC = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'


def add_beam_arguments(ap):
    """The prefix-beam-search flags, shared with run_inference --read-back."""
    ap.add_argument("--beam", type=int, default=0, metavar="W", help="also read by a CTC prefix beam search W strings wide (0: off)")
    ap.add_argument("--lm-corpus", default=None, metavar="FILE", help="one word per line: count a character n-gram LM for the beam read")
    ap.add_argument("--lm", default=None, metavar="FILE.npz", help="a saved character n-gram LM (legibility.CharLM.save)")
    ap.add_argument("--lm-order", type=int, default=2, choices=[1, 2, 3], help="order of the LM counted from --lm-corpus")
    ap.add_argument("--lm-weight", type=float, default=0.0, help="weight of the LM's log-probabilities in the beam score")
    ap.add_argument("--len-bonus", type=float, default=0.0, help="added to the beam score per character")


def check_beam_arguments(ap, args):
    if not (0 <= args.beam <= 64):
        ap.error("--beam must lie in [0, 64]")
    if args.lm_corpus and args.lm:
        ap.error("--lm-corpus and --lm exclude each other")
    if (args.lm_corpus or args.lm) and not args.beam:
        ap.error("--lm-corpus / --lm need --beam W")


def load_lm(args, char_vec, device):
    """The CharLM the flags name, on `device`, or None."""
    import sys
    from .legibility import CharLM
    if args.lm:
        lm = CharLM.load(args.lm)
        if lm.char_vector != char_vec:
            raise ValueError("%s was counted over another character vector" % args.lm)
        return lm.to(device)
    if args.lm_corpus:
        with open(args.lm_corpus) as f:
            words = [w for w in (line.strip() for line in f) if w]
        lm = CharLM.from_words(words, char_vec, args.lm_order)
        print("%s: %d words, %d skipped (characters outside the character vector)" % (args.lm_corpus, len(words), lm.skipped), file=sys.stderr)
        return lm.to(device)
    return None


def beam_keywords(args, char_vec, device) -> dict:
    """Keyword arguments of legibility.evaluate_recognizer / read_back for the flags; empty at --beam 0."""
    if not args.beam:
        return {}
    return {"beam": args.beam, "lm": load_lm(args, char_vec, device), "lm_weight": args.lm_weight, "len_bonus": args.len_bonus}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--recognizer-weights", default=None, help="checkpoint prefix (without .safetensors)")
    ap.add_argument("--my-rec", action="store_true", help="the BiLSTM recognizer (make_my_recognizer)")
    src = ap.add_mutually_exclusive_group()
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
    ap.add_argument("--fidelity", type=int, default=0, metavar="N", help="render N words and report Frechet / kernel distances to the real batches")
    ap.add_argument("--feature-space", default="recognizer", choices=["recognizer", "discriminator"])
    ap.add_argument("--discriminator-weights", default=None, help="discriminator checkpoint prefix (--feature-space discriminator)")
    ap.add_argument("--real-stats", default=None, metavar="FILE.npz", help="the real set's statistics: read if present, written otherwise")
    ap.add_argument("--kid-subsets", type=int, default=100)
    ap.add_argument("--kid-subset-size", type=int, default=1000)
    ap.add_argument("--features-real", default=None, metavar="A.npy", help="precomputed real features [N,D]: no networks needed")
    ap.add_argument("--features-fake", default=None, metavar="B.npy")
    add_beam_arguments(ap)
    args = ap.parse_args(argv)
    check_beam_arguments(ap, args)
    if (args.features_real is None) != (args.features_fake is None):
        ap.error("--features-real and --features-fake go together")
    if args.kid_subsets < 1 or args.kid_subset_size < 2:
        ap.error("--kid-subsets must be >= 1 and --kid-subset-size >= 2")
    if args.features_real is None:
        if args.recognizer_weights is None:
            ap.error("--recognizer-weights is required")
        if args.data is None and not args.synthetic:
            ap.error("one of --data / --synthetic is required")
    if args.fidelity < 0 or args.fidelity == 1:
        ap.error("--fidelity needs at least 2 words")
    if args.fidelity and not args.generator_weights:
        ap.error("--fidelity needs --generator-weights")
    if args.fidelity and args.feature_space == "discriminator" and not args.discriminator_weights:
        ap.error("--feature-space discriminator needs --discriminator-weights")
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
    if args.features_real is not None:
        from . import fidelity
        out = fidelity.fidelity_from_features(np.load(args.features_real), np.load(args.features_fake), args.kid_subsets,
                                              args.kid_subset_size, device=args.device)
        print(json.dumps(out))
        return out
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
    batches = list(itertools.islice(dataset, args.batches))
    search = beam_keywords(args, args.char_vec, R.device)
    out = legibility.evaluate_recognizer(R, batches, args.char_vec, lexicon, **search)
    if args.generator_weights:
        G = NA.make_generator(128, in_dim, (32, 8192), None, "B3", n_classes, vis_model=False)
        G.load_weights(args.generator_weights)
        style = np.random.default_rng(0).uniform(-1, 1, (max(1, min(len(args.words), 16)),) + in_dim).astype(np.float32)
        rb = legibility.read_back(G, R, style, args.words, args.char_vec, **search)
        out["read_back"] = rb
        out["cer_fake"] = sum(r["distance"] for r in rb) / max(1, sum(len(r["target"]) for r in rb))
        out["wer_fake"] = sum(r["distance"] != 0 for r in rb) / len(rb)
        if search:
            out["cer_fake_beam"] = sum(r["distance_beam"] for r in rb) / max(1, sum(len(r["target"]) for r in rb))
            out["wer_fake_beam"] = sum(r["distance_beam"] != 0 for r in rb) / len(rb)
    if args.fidelity:
        out.update(_fidelity(args, NA, G, R, batches, lexicon, in_dim))
    print(json.dumps(out))
    return out


def _fidelity(args, NA, G, R, batches, lexicon, in_dim):
    """--fidelity: N words from the lexicon (or from the real batches' labels) rendered in random styles, against `batches`."""
    import os
    from . import fidelity
    longest = max(max(len(w) for w in lexicon), 1) if lexicon else max(np.asarray(lab).shape[1] for _, lab in batches)
    buckets = [[] for _ in range(longest)]
    if lexicon:
        for w in lexicon:
            buckets[len(w) - 1].append([args.char_vec.index(c) for c in w])
    else:
        for _, lab in batches:
            lab = np.asarray(lab.cpu() if hasattr(lab, "cpu") else lab)
            buckets[lab.shape[1] - 1] += [list(map(int, row)) for row in lab]
    model = R
    if args.feature_space == "discriminator":
        model = NA.make_discriminator(in_dim, None, "B1", vis_model=False)
        model.load_weights(args.discriminator_weights)
    stats = None
    if args.real_stats:
        dim = fidelity.FeatureExtractor(model, args.feature_space).dim
        stats = (fidelity.FeatureStats.load(args.real_stats, model.device) if os.path.exists(args.real_stats)
                 else fidelity.FeatureStats(dim, model.device))
    fresh = stats is not None and stats.n == 0
    style = np.random.default_rng(0).uniform(-1, 1, (16,) + tuple(in_dim)).astype(np.float32)
    res = fidelity.evaluate_fidelity(G, model, batches, style, fidelity.fake_word_batches(buckets, args.fidelity, args.batch_size),
                                     space=args.feature_space, real_stats=stats, subsets=args.kid_subsets,
                                     subset_size=args.kid_subset_size)
    if fresh:
        stats.save(args.real_stats)
    return res


if __name__ == "__main__":
    main()
