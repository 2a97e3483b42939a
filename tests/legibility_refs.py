"""Plain numpy / Python references of the decode kernels (csrc/ctc_decode.hip), shared by tests/test_legibility_cpu.py and
tests/test_ctc_decode_gpu.py.  Nothing here touches the code under test."""
import numpy as np


def log_probs_ref(logits):
    """fp64 lp = log_softmax(log(softmax(logits) + 1e-7)) over the last axis (K.ctc_batch_cost's view of the frames)."""
    x = np.asarray(logits, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    y = np.log(e / e.sum(-1, keepdims=True) + 1e-7)
    m = y.max(-1, keepdims=True)
    return y - (m + np.log(np.exp(y - m).sum(-1, keepdims=True)))


def greedy_ref(logits, input_length=None):
    """Best path: argmax per frame (numpy.argmax: lowest index on a tie), merge equal neighbours, drop blanks (= C-1).
    -> (labels int32 [B,input_length] padded with -1, lengths int32 [B], logp fp64 [B])."""
    logits = np.asarray(logits)
    B, T, C = logits.shape
    il = T if input_length is None else input_length
    lp = log_probs_ref(logits)
    labels = np.full((B, il), -1, np.int32)
    lengths = np.zeros(B, np.int32)
    logp = np.zeros(B, np.float64)
    for b in range(B):
        prev, n = -1, 0
        for t in range(il):
            s = int(np.argmax(logits[b, t]))
            logp[b] += lp[b, t, s]
            if s != C - 1 and s != prev:
                labels[b, n] = s
                n += 1
            prev = s
        lengths[b] = n
    return labels, lengths, logp


def edit_distance_ref(a, b):
    """The textbook Levenshtein DP with unit costs."""
    a, b = list(a), list(b)
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return D[len(a)][len(b)]


def render_path(rng, word, T, C, gain=8.0):
    """N(0,1) noise + `gain` on a path: two frames per character, one blank frame between characters, blank to the end."""
    x = rng.standard_normal((T, C)).astype(np.float32)
    path = []
    for i, c in enumerate(word):
        if i:
            path.append(C - 1)
        path += [c, c]
    path += [C - 1] * (T - len(path))
    assert len(path) == T, (word, T)
    x[np.arange(T), path] += gain
    return x


PLANTED_WORDS = [[7, 7, 7, 2, 2], [3], [10, 11], [5, 0, 5], [51, 50, 49, 48], [1, 2, 3, 4, 5], [20, 20], [0, 51, 0, 51, 0]]


def lexicon_problem(seed, B=8, W=67, T=19, C=53, Lmax=5):
    """The score-words fixture: a deduplicated lexicon of W words of mixed lengths 1..Lmax whose first B entries (shuffled into
    place) are PLANTED_WORDS, and logits [B,T,C] with sample b rendering planted word b.
    -> (logits float32, lexicon list of lists, planted index per sample)."""
    rng = np.random.default_rng(seed)
    assert B == len(PLANTED_WORDS)
    seen = {tuple(w) for w in PLANTED_WORDS}
    extra = []
    while len(extra) < W - B:
        w = tuple(int(c) for c in rng.integers(0, C - 1, int(rng.integers(1, Lmax + 1))))
        if w not in seen:                       # (a duplicated one-letter word once made the best-to-second gap zero)
            seen.add(w)
            extra.append(list(w))
    order = rng.permutation(W)
    pool = [list(w) for w in PLANTED_WORDS] + extra
    lexicon = [pool[i] for i in order]
    where = {int(src): pos for pos, src in enumerate(order)}
    planted = [where[b] for b in range(B)]
    logits = np.stack([render_path(rng, PLANTED_WORDS[b], T, C) for b in range(B)], 0)
    return logits, lexicon, planted
