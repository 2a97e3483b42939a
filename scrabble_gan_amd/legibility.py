"""Reading the recognizer: text, character / word error rates and lexicon-constrained reads.

ScrabbleGAN trains R so that G's handwriting can be read; `RecognizerModel.__call__` only ever returns the CTC cost.
This module turns R's frames into text on the device (csrc/ctc_decode.hip through ops):

    decode_text(labels, lengths, char_vector)                       int rows -> list of str
    evaluate_recognizer(recognizer, batches, char_vector, lexicon)  CER / WER of R on labelled images
    read_back(generator, recognizer, style, words, char_vector)     what R reads from G's rendering of each word
    CharLM.from_words(words, char_vector, order)                    character n-gram table for the beam read

Both take beam=W (and lm=CharLM, lm_weight, len_bonus): the read is then also taken by a CTC prefix beam search W strings wide
(ops.ctc_beam_decode), the most probable STRING rather than the most probable alignment, open vocabulary.

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


class CharLM:
    """Dense character n-gram LM for ops.ctc_beam_decode: `table` fp32 [C**(order-1), C] of log-probabilities, C =
    len(char_vector) + 1.  The row of a context is the last order-1 labels, oldest first, read as a number in base C, with the
    digit C-1 at a position before the start of the word; column c < C-1 is "next character c", column C-1 is end of word."""

    def __init__(self, table, order: int, char_vector: str, skipped: int = 0):
        table = torch.as_tensor(table, dtype=torch.float32).contiguous()
        C = len(char_vector) + 1
        if order not in (1, 2, 3) or tuple(table.shape) != (C ** (order - 1), C):
            raise ValueError("CharLM: order %r in {1,2,3} and table %s == %s" % (order, tuple(table.shape), (C ** (order - 1), C)))
        self.table, self.order, self.char_vector, self.skipped = table, int(order), char_vector, int(skipped)

    @staticmethod
    def context_index(labels: Sequence[int], order: int, C: int) -> int:
        """Table row for the character that follows `labels` (the prefix so far)."""
        idx = 0
        for k in range(order - 1, 0, -1):
            idx = idx * C + (int(labels[-k]) if len(labels) >= k else C - 1)
        return idx

    @classmethod
    def from_words(cls, words: Iterable[str], char_vector: str, order: int = 2, smoothing: float = 0.1) -> "CharLM":
        """Counts over `words` (each contributes its characters and one end-of-word) with `smoothing` added to every one of the
        C columns; every row exponentiates to a sum of 1.  Words with a character outside `char_vector` are skipped and counted
        in `.skipped`."""
        if order not in (1, 2, 3) or not smoothing > 0:
            raise ValueError("CharLM.from_words: order in {1,2,3} and smoothing > 0")
        C = len(char_vector) + 1
        index = {c: i for i, c in enumerate(char_vector)}
        counts = np.full((C ** (order - 1), C), float(smoothing), np.float64)
        skipped = 0
        for w in words:
            if any(c not in index for c in w):
                skipped += 1
                continue
            labels = [index[c] for c in w]
            for p in range(len(labels) + 1):
                counts[cls.context_index(labels[:p], order, C), labels[p] if p < len(labels) else C - 1] += 1.0
        return cls(np.log(counts / counts.sum(1, keepdims=True)).astype(np.float32), order, char_vector, skipped)

    def save(self, path: str) -> None:
        with open(path, "wb") as f:             # (a file object: numpy appends no suffix)
            np.savez(f, table=self.table.detach().cpu().numpy(), order=np.int64(self.order), char_vector=np.str_(self.char_vector))

    @classmethod
    def load(cls, path: str) -> "CharLM":
        with np.load(path) as z:
            return cls(z["table"], int(z["order"]), str(z["char_vector"]))

    def to(self, device) -> "CharLM":
        return CharLM(self.table.to(device), self.order, self.char_vector, self.skipped)


def _beam_read(recognizer, logits, frames, beam, lm, lm_weight, len_bonus):
    """Top string of the prefix beam search on `logits` -> (labels int32 [B,frames], lengths int32 [B], scores [B])."""
    if lm is not None and lm.table.shape[1] != logits.shape[2]:
        raise ValueError("the LM has %d columns, the recognizer %d classes" % (lm.table.shape[1], logits.shape[2]))
    table, order = (None, 1) if lm is None else (lm.table, lm.order)
    lab, ln, score = ops.ctc_beam_decode(ops.ctc_log_probs(logits), frames, beam=beam, lm=table, lm_order=order, lm_weight=lm_weight,
                                         len_bonus=len_bonus, nbest=1)
    return lab[:, 0].contiguous(), ln[:, 0].contiguous(), score[:, 0]


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


def _score_batch(recognizer, images, labels, sums, lexicon=None, sums_lex=None, beam=None, sums_beam=None):
    """One labelled batch: best-path read (and the lexicon read, and with beam = (width, lm, lm_weight, len_bonus) the beam read)
    against `labels`, added into the fp64 sums."""
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
    if beam is not None:
        b_hyp, b_len, _ = _beam_read(recognizer, logits, frames, *beam)
        ops.legibility_sums(ops.edit_distance(b_hyp, b_len, ref, ref_len), ref_len, sums_beam)
    return hyp, hyp_len


def evaluate_recognizer(recognizer, batches: Iterable, char_vector: str, lexicon: Optional[Sequence] = None, beam: int = 0,
                        lm: Optional[CharLM] = None, lm_weight: float = 0.0, len_bonus: float = 0.0) -> dict:
    """CER / WER of `recognizer` (inference mode) over `batches`, an iterable of (images [B,32,16L,1], labels [B,L]) with one
    word length per batch (the loaders' contract).  -> {cer, wer, n_words, n_chars}, plus {cer_lexicon, wer_lexicon} when
    `lexicon` (strings over `char_vector`, or index lists; at most 31 characters each) is given, plus {cer_beam, wer_beam} of
    the prefix beam search `beam` strings wide (rescored by `lm`, a CharLM on the recognizer's device) when beam > 0."""
    dev = recognizer.device
    sums = torch.zeros(4, device=dev, dtype=torch.float64)
    lex = sums_lex = None
    if lexicon is not None:
        words, word_len = pack_words(lexicon, char_vector)
        if word_len.min() < 1 or word_len.max() > MAX_WORD:
            raise ValueError("lexicon words must have 1 to %d characters" % MAX_WORD)
        lex = (_as_labels(words, dev), _as_labels(word_len, dev))
        sums_lex = torch.zeros(4, device=dev, dtype=torch.float64)
    search = sums_beam = None
    if beam:
        search = (int(beam), lm, float(lm_weight), float(len_bonus))
        sums_beam = torch.zeros(4, device=dev, dtype=torch.float64)
    for images, labels in batches:
        _score_batch(recognizer, images, labels, sums, lex, sums_lex, search, sums_beam)
    out = _rates(sums)
    if lex is not None:
        r = _rates(sums_lex)
        out["cer_lexicon"], out["wer_lexicon"] = r["cer"], r["wer"]
    if search is not None:
        r = _rates(sums_beam)
        out["cer_beam"], out["wer_beam"] = r["cer"], r["wer"]
    return out


def read_back(generator, recognizer, style, words: Sequence[str], char_vector: str, beam: int = 0, lm: Optional[CharLM] = None,
              lm_weight: float = 0.0, len_bonus: float = 0.0) -> List[dict]:
    """G writes each word (inference mode; word i in the style of image i modulo the number of style images), R reads it.
    -> [{"target", "read", "distance"}] in the order of `words`; with beam > 0 each row also carries the prefix beam search's
    {"read_beam", "distance_beam", "score_beam"} on the same rendering."""
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
        if beam:
            b_hyp, b_len, b_score = recognizer.transcribe_beam(img, beam=beam, lm=lm, lm_weight=lm_weight, len_bonus=len_bonus)
            b_hyp, b_len = b_hyp[:, 0].contiguous(), b_len[:, 0].contiguous()
            b_dist = ops.edit_distance(b_hyp, b_len, ref, ref_len).tolist()
            for i, text, d, sc in zip(idx, decode_text(b_hyp, b_len, char_vector), b_dist, b_score[:, 0].tolist()):
                out[i].update(read_beam=text, distance_beam=int(d), score_beam=float(sc))
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
