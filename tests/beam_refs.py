"""Plain Python fp64 references of the CTC prefix beam search (csrc/ctc_beam.hip), shared by tests/test_beam_cpu.py and
tests/test_ctc_beam_gpu.py.  Nothing here imports the package under test.

The contract (blank = C-1, a prefix is a tuple of labels in [0, C-2]): the beam starts as {(): pb = 0, pnb = -inf, acc = 0};
per frame every entry l of the previous beam, tot = lse(pb, pnb),
    stays:    pb'(l)  (+)= tot + lp[t, blank];   pnb'(l) (+)= pnb + lp[t, last(l)]           (not for the empty prefix)
    extends:  pnb'(l+c) (+)= lp[t, c] + (pb if c == last(l) else tot)                        for every c < C-1
              acc(l+c) = acc(l) + len_bonus + lm_weight * lm[ctx(l), c]
(+) is log-add-exp over the contributions to the same STRING; the new beam is the `beam` strings of highest
lse(pb', pnb') + acc (a tie: the lower parent slot * C + c, stay = C-1).  A survivor's final score adds
lm_weight * lm[ctx(l), C-1] (end of word)."""
import itertools
import math

import numpy as np

NEG = -math.inf


def lse(a, b):
    m = max(a, b)
    if m == NEG:
        return NEG
    return m + math.log(math.exp(a - m) + math.exp(b - m))


def lm_context(prefix, order, C):
    """Row of the dense [C**(order-1), C] table: the last order-1 labels, oldest first, base C; a missing position is C-1."""
    idx = 0
    for k in range(order - 1, 0, -1):
        idx = idx * C + (prefix[-k] if len(prefix) >= k else C - 1)
    return idx


def log_softmax_rows(raw):
    raw = np.asarray(raw, np.float64)
    m = raw.max(-1, keepdims=True)
    return raw - (m + np.log(np.exp(raw - m).sum(-1, keepdims=True)))


def _search(lp, beam, lm, order, lm_weight, len_bonus, by_node):
    lp = np.asarray(lp, np.float64)
    T, C = lp.shape
    blank = C - 1
    if lm is not None:
        lm = np.asarray(lm, np.float64)
        assert lm.shape == (C ** (order - 1), C), lm.shape

    def credit(prefix, c):
        return len_bonus + (lm_weight * lm[lm_context(prefix, order, C), c] if lm is not None else 0.0)

    # an entry: [prefix, pb, pnb, acc, made, node].  by_node: `node` is a number drawn when the entry entered the beam and
    # `made` = (node of its parent, character) is what it was created as; an extension merges on that pair, not on the string
    entries = [[(), 0.0, NEG, 0.0, ("root",), 0]]
    min_gap, merges, next_node = math.inf, 0, 1
    for t in range(T):
        cand = {}           # identity -> [prefix, pb, pnb, acc, tie key, made, node or None]
        for slot, (prefix, pb, pnb, acc, made, node) in enumerate(entries):
            tot = lse(pb, pnb)
            last = prefix[-1] if prefix else -1
            ident = made if by_node else prefix
            e = cand.get(ident)
            if e is None:
                e = cand[ident] = [prefix, NEG, NEG, acc, slot * C + blank, made, node]
            else:
                merges += 1
                e[6] = node
            e[1] = lse(e[1], tot + lp[t, blank])
            if prefix:
                e[2] = lse(e[2], pnb + lp[t, last])
            for c in range(blank):
                child = prefix + (c,)
                ident = (node, c) if by_node else child
                e = cand.get(ident)
                if e is None:
                    e = cand[ident] = [child, NEG, NEG, acc + credit(prefix, c), slot * C + c, (node, c), None]
                else:
                    merges += 1
                e[2] = lse(e[2], lp[t, c] + (pb if c == last else tot))
        ranked = sorted(cand.values(), key=lambda e: (-(lse(e[1], e[2]) + e[3]), e[4]))
        if len(ranked) > beam:
            gap = (lse(ranked[beam - 1][1], ranked[beam - 1][2]) + ranked[beam - 1][3]) - (lse(ranked[beam][1], ranked[beam][2]) + ranked[beam][3])
            if not math.isnan(gap):             # (-inf) - (-inf): a cut among massless strings decides nothing
                min_gap = min(min_gap, gap)
        entries = []
        for e in ranked[:beam]:
            if e[6] is None:
                e[6], next_node = next_node, next_node + 1
            entries.append([e[0], e[1], e[2], e[3], e[5], e[6]])
    out = []
    for slot, (prefix, pb, pnb, acc, _, _) in enumerate(entries):
        s = lse(pb, pnb) + acc
        if lm is not None:
            s += lm_weight * lm[lm_context(prefix, order, C), blank]
        out.append((s, slot, prefix))
    out.sort(key=lambda e: (-e[0], e[1]))
    return [(s, p) for s, _, p in out], min_gap, merges


def beam_ref(lp, beam, lm=None, order=1, lm_weight=0.0, len_bonus=0.0):
    """lp [T,C] log-probabilities -> (survivors [(score, prefix)] best first, the smallest gap over all frames between the
    beam-th and the (beam+1)-th candidate score (inf when no cut happened), merges into an already-present string)."""
    return _search(lp, beam, lm, order, lm_weight, len_bonus, by_node=False)


def beam_node_ref(lp, beam, lm=None, order=1, lm_weight=0.0, len_bonus=0.0):
    """The deliberately WRONG identity (parent node, character): a prefix that fell out of the beam and is re-created no longer
    merges into its surviving child.  Only there to show that a fixture tells the two apart."""
    return _search(lp, beam, lm, order, lm_weight, len_bonus, by_node=True)


def collapse(path, blank):
    out, prev = [], -1
    for s in path:
        if s != blank and s != prev:
            out.append(s)
        prev = s
    return tuple(out)


def brute_force(lp):
    """All C**T alignments, collapsed; {string: log of the summed path probabilities}."""
    lp = np.asarray(lp, np.float64)
    T, C = lp.shape
    logs = {}
    for path in itertools.product(range(C), repeat=T):
        logs.setdefault(collapse(path, C - 1), []).append(sum(lp[t, s] for t, s in enumerate(path)))
    out = {}
    for k, v in logs.items():
        m = max(v)
        out[k] = m + math.log(sum(math.exp(x - m) for x in v))
    return out


def all_prefixes(T, C):
    """Every string of at most T labels: what a beam that never cuts holds after T frames."""
    return [p for n in range(T + 1) for p in itertools.product(range(C - 1), repeat=n)]


# ---------------------------------------------------------------------------------------- fixtures shared by the CPU and GPU tests
GUARD = 1e-3            # nat: below this gap a legitimate fp32 rounding difference may cut / rank another string
MAX_LEFT_OUT = 2        # of the 8 samples of a parity case
IDENTITY_SEED, IDENTITY_BEAM = 1840, 3
EXHAUSTIVE = {(5, 3): 0, (3, 4): 0}          # (T, C) -> seed; beam = nbest = 64 holds all 63 / 40 prefixes: no cut ever happens
CUT_4096_SEED = 2                            # the C = 64, beam = 64, T = 7 noise case (64 * 64 candidates per frame); picked on the reference:
#                                              seeds 0..7 leave 3 4 2 3 3 3 3 3 samples below the guard (64 cuts among 4096 candidates per frame)
# (name, kind, T, C, beam, seed)
PARITY_CASES = ([("planted", "planted", 19, 53, 8, s) for s in (0, 2)] + [("noise", "noise", 11, 53, 8, s) for s in (0, 1)] +
                [("noise", "noise", 7, 53, 4, s) for s in (0, 1, 2)] + [("noise", "noise", 7, 6, 64, 1)] +
                [("noise", "noise", 67, 53, 4, s) for s in (0, 1, 2)] + [("trigram", "trigram", 19, 53, 8, s) for s in (0, 2)] +
                [("cut4096", "noise", 7, 64, 64, CUT_4096_SEED)])
_cache = {}


def identity_logits():
    return np.float32(np.random.default_rng(IDENTITY_SEED).standard_normal((6, 3)) * 2)


def exhaustive_logits(T, C, B=6):
    return np.float32(np.random.default_rng(EXHAUSTIVE[(T, C)]).standard_normal((B, T, C)) * 2)


def parity_case(kind, T, C, beam, seed):
    """-> dict(logits float32 [8,T,C], lm float32 table or None, order, lm_weight, len_bonus, ref = [beam_ref(...) per sample],
    compared = [sample indices whose smallest cut gap is >= GUARD]).  Computed once per process; treat it as read-only."""
    from tests.legibility_refs import PLANTED_WORDS, log_probs_ref, render_path
    key = (kind, T, C, beam, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(seed)
    lm, order, lm_weight, len_bonus = None, 1, 0.0, 0.0
    if kind == "trigram":
        raw = rng.standard_normal((C * C, C)) * 2               # drawn FIRST
        lm, order, lm_weight, len_bonus = log_softmax_rows(raw).astype(np.float32), 3, 0.7, 0.5
    if kind == "noise":
        logits = np.stack([np.float32(rng.standard_normal((T, C))) * 3 for _ in range(8)], 0).astype(np.float32)
    else:
        logits = np.stack([render_path(rng, PLANTED_WORDS[b], T, C, 4.0 if kind == "trigram" else 8.0) for b in range(8)], 0)
    lp = log_probs_ref(logits)
    ref = [beam_ref(lp[b], beam, lm, order, lm_weight, len_bonus) for b in range(8)]
    out = dict(logits=logits, lm=lm, order=order, lm_weight=lm_weight, len_bonus=len_bonus, ref=ref,
               compared=[b for b in range(8) if ref[b][1] >= GUARD])
    _cache[key] = out
    return out


def rank_is_checked(survivors, r):
    """The string at rank r is compared only if the reference's gaps to both neighbours are >= GUARD."""
    s = [x[0] for x in survivors]
    up = r == 0 or s[r - 1] - s[r] >= GUARD
    down = r == len(s) - 1 or s[r] - s[r + 1] >= GUARD
    return up and down
