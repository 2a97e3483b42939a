"""The CTC prefix beam search's references and host side, without a GPU: tests/beam_refs.py against brute force, the
string-identity counter-example, legibility.CharLM, the command-line flags, and -- what keeps tests/test_ctc_beam_gpu.py honest
-- every guarded fixture's cap, asserted on the fp64 reference alone."""
import math

import numpy as np
import pytest

from tests import beam_refs as BR
from tests import legibility_refs as LR

CV = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'


# ---------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("T,C,n_prefixes", [(5, 3, 63), (3, 4, 40)])
def test_beam_ref_equals_brute_force_when_nothing_is_cut(T, C, n_prefixes):
    """beam = 64 holds every string of at most T labels, so the search is exact: each finite survivor is the log-sum over all
    C**T alignments that collapse to it (to 1e-12; measured 4e-15), strings that need more than T frames score -inf."""
    logits = BR.exhaustive_logits(T, C)
    worst = 0.0
    for b in range(logits.shape[0]):
        lp = LR.log_probs_ref(logits[b])
        survivors, gap, merges = BR.beam_ref(lp, 64)
        exact = BR.brute_force(lp)
        assert gap == math.inf and merges > 0
        assert sorted(p for _, p in survivors) == sorted(BR.all_prefixes(T, C)) and len(survivors) == n_prefixes
        assert [s for s, _ in survivors] == sorted((s for s, _ in survivors), reverse=True)
        for s, p in survivors:
            if p in exact:
                assert math.isfinite(s)
                worst = max(worst, abs(s - exact[p]))
            else:                                           # a repeated label needs a blank in between: more than T frames
                assert s == -math.inf and len(p) + sum(a == b for a, b in zip(p, p[1:])) > T
        assert sum(math.isfinite(s) for s, _ in survivors) == len(exact)
        assert abs(math.log(sum(math.exp(v) for v in exact.values()))) < 1e-9          # the strings partition the alignments
        assert survivors[0][0] - survivors[1][0] >= 0.06, "fixture: the top gap of sample %d fell below 0.06 nat" % b
    print("beam_ref vs brute force, T=%d C=%d: max error %.2e" % (T, C, worst))
    assert worst <= 1e-12


def test_identity_is_string_equality_on_the_1840_case():
    """beam = 3 on six frames of three classes: the prefix (0,1,0) drops out while (0,1,0,1) survives, is re-created from (0,1),
    and its extension by 1 must merge into the survivor.  Merging on (parent node, char) instead reads another word."""
    lp = LR.log_probs_ref(BR.identity_logits())
    right, gap, merges = BR.beam_ref(lp, BR.IDENTITY_BEAM)
    wrong, _, _ = BR.beam_node_ref(lp, BR.IDENTITY_BEAM)
    assert right[0][1] == (0, 1, 0, 1) and abs(right[0][0] - (-1.6140)) < 5e-5
    assert wrong[0][1] == (0, 1) and abs(wrong[0][0] - (-1.9728)) < 5e-5
    assert right[0][1] != wrong[0][1]
    assert gap >= 0.13 and merges > 0
    exact = BR.brute_force(lp)                              # a beam can only lose mass
    assert right[0][0] <= exact[(0, 1, 0, 1)] + 1e-12


def test_node_identity_agrees_where_nothing_is_cut():
    lp = LR.log_probs_ref(BR.exhaustive_logits(3, 4)[0])
    a, _, _ = BR.beam_ref(lp, 64)
    b, _, _ = BR.beam_node_ref(lp, 64)
    assert [p for _, p in a] == [p for _, p in b] and np.allclose([s for s, _ in a if math.isfinite(s)], [s for s, _ in b if math.isfinite(s)], atol=1e-12)


def test_lm_terms_of_the_reference():
    """One frame, beam wide enough: score(c) = lp[c] + len_bonus + w * (lm[start, c] + lm[ctx(c), eow]); the empty string
    takes lp[blank] + w * lm[start, eow]."""
    C, w, bonus = 4, 0.7, 0.5
    rng = np.random.default_rng(3)
    lp = LR.log_probs_ref(rng.standard_normal((1, C)))
    for order in (1, 2, 3):
        lm = BR.log_softmax_rows(rng.standard_normal((C ** (order - 1), C)))
        got = dict((p, s) for s, p in BR.beam_ref(lp, 8, lm, order, w, bonus)[0])
        start = BR.lm_context((), order, C)
        assert start == {1: 0, 2: C - 1, 3: (C - 1) * C + (C - 1)}[order]
        assert abs(got[()] - (lp[0, C - 1] + w * lm[start, C - 1])) < 1e-12
        for c in range(C - 1):
            want = lp[0, c] + bonus + w * (lm[start, c] + lm[BR.lm_context((c,), order, C), C - 1])
            assert abs(got[(c,)] - want) < 1e-12


# ---------------------------------------------------------------------------------------- the guarded GPU fixtures
@pytest.mark.parametrize("name,kind,T,C,beam,seed", BR.PARITY_CASES)
def test_parity_fixture_satisfies_its_cap_on_the_reference(name, kind, T, C, beam, seed):
    """At most 2 of the 8 samples may fall below the 1e-3 nat guard, the case must merge, and every sample fills its beam."""
    case = BR.parity_case(kind, T, C, beam, seed)
    assert BR.GUARD == 1e-3 and BR.MAX_LEFT_OUT == 2
    left_out = 8 - len(case["compared"])
    print("%s T=%d C=%d beam=%d seed=%d: %d of 8 below the guard, %d merges, smallest cut gap %.2e"
          % (name, T, C, beam, seed, left_out, sum(r[2] for r in case["ref"]), min(r[1] for r in case["ref"])))
    assert left_out <= BR.MAX_LEFT_OUT
    assert sum(r[2] for r in case["ref"]) > 0
    assert all(len(r[0]) == beam and all(math.isfinite(s) for s, _ in r[0]) for r in case["ref"])
    assert sum(BR.rank_is_checked(case["ref"][b][0], 0) for b in case["compared"]) >= 4, "too few top strings would be compared"
    if kind == "trigram":
        assert case["lm"].shape == (C * C, C) and np.allclose(np.exp(case["lm"].astype(np.float64)).sum(1), 1.0, atol=1e-5)


def test_planted_fixture_reads_its_words_on_the_reference():
    """Gain 8: the top string of the reference is the planted word, which is also the best path, for beam 1, 8 and 64."""
    case = BR.parity_case("planted", 19, 53, 8, 0)
    lp = LR.log_probs_ref(case["logits"])
    lab, ln, _ = LR.greedy_ref(case["logits"])
    for b, word in enumerate(LR.PLANTED_WORDS):
        assert list(lab[b, :ln[b]]) == word
        for beam in (1, 8, 64):
            assert list(BR.beam_ref(lp[b], beam)[0][0][1]) == word


# ---------------------------------------------------------------------------------------- CharLM
def test_char_lm_rows_are_normalised_and_hand_counted():
    from scrabble_gan_amd.legibility import CharLM
    cv = "abc"
    C = 4
    lm = CharLM.from_words(["ab", "abc", "b"], cv, order=2, smoothing=0.1)
    t = lm.table.double().numpy()
    assert lm.order == 2 and t.shape == (C, C) and lm.table.dtype.is_floating_point and lm.skipped == 0
    assert np.allclose(np.exp(t).sum(1), 1.0, atol=1e-6)
    # rows by hand (context -> counts of a, b, c, end): start: a 2, b 1; after a: b 2; after b: c 1, end 2; after c: end 1
    counts = np.array([[0, 2, 0, 0], [0, 0, 1, 2], [0, 0, 0, 1], [2, 1, 0, 0]], np.float64) + 0.1
    assert np.allclose(t, np.log(counts / counts.sum(1, keepdims=True)), atol=1e-6)
    for order in (1, 3):
        lm = CharLM.from_words(["ab", "abc", "b"], cv, order=order)
        assert lm.table.shape == (C ** (order - 1), C) and np.allclose(np.exp(lm.table.double().numpy()).sum(1), 1.0, atol=1e-5)
    uni = CharLM.from_words(["ab", "abc", "b"], cv, order=1, smoothing=0.5).table.double().numpy()
    assert np.allclose(np.exp(uni[0]), (np.array([2, 3, 1, 3]) + 0.5) / 11.0, atol=1e-6)


def test_char_lm_trigram_context_at_word_start():
    from scrabble_gan_amd.legibility import CharLM
    C = 4
    assert CharLM.context_index([], 3, C) == 3 * C + 3                  # both positions missing
    assert CharLM.context_index([1], 3, C) == 3 * C + 1                 # oldest first: (missing, b)
    assert CharLM.context_index([0, 1, 2], 3, C) == 1 * C + 2
    assert CharLM.context_index([0, 1, 2], 2, C) == 2 and CharLM.context_index([], 2, C) == 3 and CharLM.context_index([2], 1, C) == 0
    for prefix in ([], [1], [0, 1, 2]):
        for order in (1, 2, 3):
            assert CharLM.context_index(prefix, order, C) == BR.lm_context(tuple(prefix), order, C)
    lm = CharLM.from_words(["ba"], "abc", order=3, smoothing=0.25)
    t = np.exp(lm.table.double().numpy())
    assert abs(t[3 * C + 3, 1] - 1.25 / 2.0) < 1e-6                     # start of word -> b
    assert abs(t[3 * C + 1, 0] - 1.25 / 2.0) < 1e-6                     # (missing, b) -> a
    assert abs(t[1 * C + 0, 3] - 1.25 / 2.0) < 1e-6                     # (b, a) -> end of word


def test_char_lm_save_load_and_foreign_characters(tmp_path):
    from scrabble_gan_amd.legibility import CharLM
    lm = CharLM.from_words(["cab", "café", "x-ray", "abba"], "abc", order=2)
    assert lm.skipped == 2
    only = CharLM.from_words(["cab", "abba"], "abc", order=2)
    assert np.array_equal(lm.table.numpy(), only.table.numpy())
    path = str(tmp_path / "lm.npz")
    lm.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["char_vector", "order", "table"]
    back = CharLM.load(path)
    assert back.order == 2 and back.char_vector == "abc" and np.array_equal(back.table.numpy(), lm.table.numpy())
    assert lm.to("cpu").table.dtype == lm.table.dtype
    with pytest.raises(ValueError):
        CharLM(np.zeros((3, 4), np.float32), 2, "abc")


# ---------------------------------------------------------------------------------------- command line
def test_evaluate_flags():
    from scrabble_gan_amd import evaluate as E
    base = ["--recognizer-weights", "w", "--synthetic"]
    a = E.parse_args(base)
    assert (a.beam, a.lm_corpus, a.lm, a.lm_order, a.lm_weight, a.len_bonus) == (0, None, None, 2, 0.0, 0.0)
    assert E.beam_keywords(a, CV, "cpu") == {}                          # beam 0: evaluate_recognizer / read_back are called as before
    a = E.parse_args(base + ["--beam", "8", "--lm-corpus", "words.txt", "--lm-order", "3", "--lm-weight", "0.7", "--len-bonus", "0.5"])
    assert (a.beam, a.lm_corpus, a.lm_order, a.lm_weight, a.len_bonus) == (8, "words.txt", 3, 0.7, 0.5)
    a = E.parse_args(base + ["--beam", "4", "--lm", "lm.npz"])
    assert a.lm == "lm.npz"
    for bad in (["--beam", "65"], ["--beam", "-1"], ["--lm", "lm.npz"], ["--beam", "4", "--lm", "a.npz", "--lm-corpus", "b.txt"],
                ["--beam", "4", "--lm-order", "4"]):
        with pytest.raises(SystemExit):
            E.parse_args(base + bad)


def test_lm_flags_build_the_table(tmp_path, capsys):
    from scrabble_gan_amd import evaluate as E
    from scrabble_gan_amd.legibility import CharLM
    corpus = tmp_path / "words.txt"
    corpus.write_text("cab\n\nnaïve\nabba\n")
    a = E.parse_args(["--recognizer-weights", "w", "--synthetic", "--beam", "4", "--lm-corpus", str(corpus), "--lm-weight", "0.3"])
    kw = E.beam_keywords(a, "abc", "cpu")
    assert sorted(kw) == ["beam", "len_bonus", "lm", "lm_weight"] and kw["beam"] == 4 and kw["lm_weight"] == 0.3
    assert kw["lm"].order == 2 and kw["lm"].skipped == 1 and "1 skipped" in capsys.readouterr().err
    kw["lm"].save(str(tmp_path / "lm.npz"))
    a = E.parse_args(["--recognizer-weights", "w", "--synthetic", "--beam", "4", "--lm", str(tmp_path / "lm.npz")])
    assert np.array_equal(E.load_lm(a, "abc", "cpu").table.numpy(), CharLM.from_words(["cab", "abba"], "abc").table.numpy())
    with pytest.raises(ValueError):
        E.load_lm(a, "abcd", "cpu")


def test_run_inference_flags_and_rows():
    from scrabble_gan_amd import run_inference as RI
    base = ["--weights", "g", "--read-back", "--recognizer-weights", "r"]
    assert RI.parse_args(base).beam == 0
    a = RI.parse_args(base + ["--beam", "16", "--lm-weight", "0.5"])
    assert a.beam == 16 and a.lm_weight == 0.5
    with pytest.raises(SystemExit):
        RI.parse_args(["--weights", "g", "--beam", "16"])
    row = {"target": "ab", "read": "ab", "distance": 0}
    assert RI.format_read_back(row) == "ab\tab\t0"
    row.update(read_beam="a", distance_beam=1, score_beam=-1.5)
    assert RI.format_read_back(row) == "ab\tab\t0\ta\t1\t-1.5000"
