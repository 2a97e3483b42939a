"""Reading the recognizer: text, character / word error rates and lexicon-constrained reads.

ScrabbleGAN trains R so that G's handwriting can be read; `RecognizerModel.__call__` only ever returns the CTC cost.
This module turns R's frames into text on the device (csrc/ctc_decode.hip through ops):

    decode_text(labels, lengths, char_vector)                       int rows -> list of str
    evaluate_recognizer(recognizer, batches, char_vector, lexicon)  CER / WER of R on labelled images
    read_back(generator, recognizer, style, words, char_vector)     what R reads from G's rendering of each word

CER = sum of edit distances / sum of reference lengths, WER = share of words with a non-zero distance.  The sums are
fp64 on the device and additive (ops.legibility_sums), one device-to-host copy per evaluation.  With a lexicon the read
of an image is the candidate word of lowest CTC cost (ops.ctc_score_words over all candidates, then a row argmin)."""
from __future__ import annotations

import contextlib
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .net_architecture import _as_labels

LEGIBILITY_HEADER = "epoch,n,cer_real,wer_real,cer_fake,wer_fake\n"
MAX_WORD = 31          # longest candidate ops.ctc_score_words takes (2 * 31 + 1 extended-label states in one wavefront)


def decode_text(labels, lengths, char_vector: str) -> List[str]:
    """Rows of character indices (tensor / array / lists) and their lengths -> strings by `char_vector[index]`:
    the inverse of data_utils.encode_word."""
    if torch.is_tensor(labels):
        labels = labels.detach().cpu().numpy()
    if torch.is_tensor(lengths):
        lengths = lengths.detach().cpu().numpy()
    out = []
    for row, n in zip(labels, lengths):
        out.append("".join(char_vector[int(c)] for c in list(row)[:int(n)]))
    return out


def pack_words(words: Sequence, char_vector: Optional[str] = None):
    """Strings (encoded with `char_vector`) or index lists of mixed lengths -> (int32 [W,stride] padded with -1, int32 [W])."""
    rows = [[char_vector.index(c) for c in w] if isinstance(w, str) else [int(c) for c in w] for w in words]
    if not rows:
        raise ValueError("empty word list")
    stride = max(1, max(len(r) for r in rows))
    packed = np.full((len(rows), stride), -1, np.int32)
    for i, r in enumerate(rows):
        packed[i, :len(r)] = r
    return packed, np.array([len(r) for r in rows], np.int32)


@contextlib.contextmanager
def preserved_rng(*models):
    """Evaluation inside a training run: the per-call NonLocalBlock kernels, spectral-norm vectors and dropout masks are drawn
    from generators the models own; their states are put back on exit, so training draws what it would have drawn anyway."""
    saved = [(m, a, getattr(m, a).get_state()) for m in models if m is not None for a in ("nl_gen", "sn_gen", "mask_gen") if hasattr(m, a)]
    try:
        yield
    finally:
        for m, a, state in saved:
            getattr(m, a).set_state(state)


def _rates(sums) -> dict:
    s = sums.tolist()
    return {"cer": s[0] / s[1] if s[1] else float("nan"), "wer": s[2] / s[3] if s[3] else float("nan"),
            "n_words": int(s[3]), "n_chars": int(s[1])}


def _score_batch(recognizer, images, labels, sums, lexicon=None, sums_lex=None):
    """One labelled batch: best-path read (and the lexicon read) against `labels`, added into the fp64 sums."""
    dev = recognizer.device
    ref = _as_labels(labels, dev)
    if ref.dim() != 2 or not (1 <= ref.shape[1] <= 63):
        raise ValueError("labels must be [B,L] with 1 <= L <= 63, got %s" % (tuple(ref.shape),))
    B, L = ref.shape
    ref_len = torch.full((B,), L, device=dev, dtype=torch.int32)
    logits = recognizer.logits(images)
    frames = recognizer._ctc_frames(logits.shape[1])
    hyp, hyp_len, _ = ops.ctc_greedy_decode(logits, frames, want_logp=False)
    ops.legibility_sums(ops.edit_distance(hyp, hyp_len, ref, ref_len), ref_len, sums)
    if lexicon is not None:
        words, word_len = lexicon
        nll = ops.ctc_score_words(ops.ctc_log_probs(logits), words, word_len, frames)
        best = torch.min(nll, dim=1).indices                       # plumbing: the row argmin picks the read
        ops.legibility_sums(ops.edit_distance(words[best].contiguous(), word_len[best].contiguous(), ref, ref_len), ref_len, sums_lex)
    return hyp, hyp_len


def evaluate_recognizer(recognizer, batches: Iterable, char_vector: str, lexicon: Optional[Sequence] = None) -> dict:
    """CER / WER of `recognizer` (inference mode) over `batches`, an iterable of (images [B,32,16L,1], labels [B,L]) with one
    word length per batch (the loaders' contract).  -> {cer, wer, n_words, n_chars}, plus {cer_lexicon, wer_lexicon} when
    `lexicon` (strings over `char_vector`, or index lists; at most 31 characters each) is given."""
    dev = recognizer.device
    sums = torch.zeros(4, device=dev, dtype=torch.float64)
    lex = sums_lex = None
    if lexicon is not None:
        words, word_len = pack_words(lexicon, char_vector)
        if word_len.min() < 1 or word_len.max() > MAX_WORD:
            raise ValueError("lexicon words must have 1 to %d characters" % MAX_WORD)
        lex = (_as_labels(words, dev), _as_labels(word_len, dev))
        sums_lex = torch.zeros(4, device=dev, dtype=torch.float64)
    for images, labels in batches:
        _score_batch(recognizer, images, labels, sums, lex, sums_lex)
    out = _rates(sums)
    if lex is not None:
        r = _rates(sums_lex)
        out["cer_lexicon"], out["wer_lexicon"] = r["cer"], r["wer"]
    return out


def read_back(generator, recognizer, style, words: Sequence[str], char_vector: str) -> List[dict]:
    """G writes each word (inference mode; word i in the style of image i modulo the number of style images), R reads it.
    -> [{"target", "read", "distance"}] in the order of `words`."""
    style = np.asarray(style, np.float32) if not torch.is_tensor(style) else style
    out: List[Optional[dict]] = [None] * len(words)
    by_len = {}
    for i, w in enumerate(words):
        by_len.setdefault(len(w), []).append(i)
    for L, idx in sorted(by_len.items()):
        if not (1 <= L <= 63):
            raise ValueError("words must have 1 to 63 characters")
        labels = np.array([[char_vector.index(c) for c in words[i]] for i in idx], np.int32)
        sel = [i % len(style) for i in idx]
        img = generator([style[sel], labels], training=False)
        hyp, hyp_len, _ = recognizer.transcribe(img)
        ref = _as_labels(labels, recognizer.device)
        ref_len = torch.full((len(idx),), L, device=recognizer.device, dtype=torch.int32)
        dist = ops.edit_distance(hyp, hyp_len, ref, ref_len).tolist()
        for i, text, d in zip(idx, decode_text(hyp, hyp_len, char_vector), dist):
            out[i] = {"target": words[i], "read": text, "distance": int(d)}
    return out


def epoch_legibility(generator, recognizer, images, labels, style, fake_labels) -> dict:
    """The train loop's hook: R on one real batch, and R on G's inference rendering of `fake_labels` in the styles of `style`.
    Draws nothing from the generators training uses.  -> {n, cer_real, wer_real, cer_fake, wer_fake}"""
    dev = recognizer.device
    with preserved_rng(generator, recognizer):
        s_real = torch.zeros(4, device=dev, dtype=torch.float64)
        s_fake = torch.zeros(4, device=dev, dtype=torch.float64)
        _score_batch(recognizer, images, labels, s_real)
        _score_batch(recognizer, generator([style, fake_labels], training=False), fake_labels, s_fake)
    real, fake = _rates(s_real), _rates(s_fake)
    return {"n": real["n_words"], "cer_real": real["cer"], "wer_real": real["wer"], "cer_fake": fake["cer"], "wer_fake": fake["wer"]}
