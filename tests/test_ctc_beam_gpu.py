"""CTC prefix beam search on the GPU (csrc/ctc_beam.hip -> ops.ctc_beam_decode -> recognizers -> legibility) against the plain
Python fp64 references of tests/beam_refs.py.

Strings must be EQUAL; scores are held with the `close` helper of tests/test_ops_gpu.py at its default 2e-5 of the reference's
largest entry, as tests/test_ctc_decode_gpu.py holds lp and nll; -inf compares by position.  Where the reference itself ranks
two candidates closer than 1e-3 nat (tests/beam_refs.GUARD) a legitimate fp32 rounding difference may cut or order them the other
way: such a sample (cut) or rank (order) is left out, at most 2 samples of 8 per case, a cap tests/test_beam_cpu.py asserts on the
reference alone.  A device error above the guard makes these tests fail, not pass."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import beam_refs as BR  # noqa: E402
from tests import legibility_refs as LR  # noqa: E402
from tests.test_ops_gpu import close  # noqa: E402

TOL = 2e-5          # `close`'s default
CV = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'


def decode(dev, logits, beam, nbest=None, input_length=None, lm=None, order=1, lm_weight=0.0, len_bonus=0.0):
    """logits [B,T,C] (numpy) -> numpy (labels [B,nbest,il], lengths [B,nbest], scores [B,nbest]) of the device search on the
    device's own lp."""
    from scrabble_gan_amd import ops
    lp = ops.ctc_log_probs(torch.from_numpy(np.ascontiguousarray(logits, np.float32)).to(dev))
    table = None if lm is None else torch.from_numpy(np.ascontiguousarray(lm, np.float32)).to(dev)
    lab, ln, sc = ops.ctc_beam_decode(lp, input_length, beam=beam, lm=table, lm_order=order, lm_weight=lm_weight, len_bonus=len_bonus,
                                      nbest=beam if nbest is None else nbest)
    assert lab.dtype == torch.int32 and ln.dtype == torch.int32 and sc.dtype == torch.float32
    lab, ln, sc = lab.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()
    il = logits.shape[1] if input_length is None else input_length
    assert lab.shape == (logits.shape[0], sc.shape[1], il) and ln.shape == sc.shape
    for b in range(lab.shape[0]):                       # the rows are well formed: labels in [0, C-2] up to the length, -1 behind
        for r in range(lab.shape[1]):
            n = ln[b, r]
            assert 0 <= n <= il and (lab[b, r, n:] == -1).all() and (lab[b, r, :n] >= 0).all() and (lab[b, r, :n] < logits.shape[2] - 1).all()
    assert not np.isnan(sc).any() and (sc[:, :-1] >= sc[:, 1:]).all(), "scores are not sorted best first"
    return lab, ln, sc


def string(lab, ln, b, r):
    return tuple(int(c) for c in lab[b, r, :ln[b, r]])


def close_scores(got, ref, name):
    """`close` on the finite entries; -inf must sit at the same places on both sides."""
    got, ref = torch.as_tensor(np.asarray(got, np.float64)), torch.as_tensor(np.asarray(ref, np.float64))
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    gi, ri = torch.isinf(got), torch.isinf(ref)
    assert torch.equal(gi, ri) and (got[gi] < 0).all(), "%s: infinities differ" % name
    close(torch.where(gi, torch.zeros_like(got), got), torch.where(ri, torch.zeros_like(ref), ref), name=name)


# ---------------------------------------------------------------------------------------- 1. exhaustive
@pytest.mark.parametrize("T,C", [(5, 3), (3, 4)])
def test_exhaustive_against_brute_force(dev, T, C):
    """beam = nbest = 64 holds all 63 / 40 strings of at most T labels, so nothing is ever cut: every finite score is the log-sum
    over all C**T alignments of its string, strings that need more than T frames are -inf, the last slots are empty."""
    logits = BR.exhaustive_logits(T, C)
    lab, ln, sc = decode(dev, logits, 64)
    n_prefixes = len(BR.all_prefixes(T, C))
    for b in range(6):
        exact = BR.brute_force(LR.log_probs_ref(logits[b]))
        want = sorted(exact.values(), reverse=True)
        got = {string(lab, ln, b, r): sc[b, r] for r in range(n_prefixes)}
        assert sorted(got) == sorted(BR.all_prefixes(T, C)), "sample %d: the survivors are not the %d prefixes" % (b, n_prefixes)
        finite = [s for s in sc[b] if np.isfinite(s)]
        assert len(finite) == len(exact)
        close_scores(finite, want, "exhaustive T=%d C=%d sample %d: multiset of finite scores" % (T, C, b))
        close_scores([got[p] for p in exact], list(exact.values()), "exhaustive T=%d C=%d sample %d: score per string" % (T, C, b))
        assert string(lab, ln, b, 0) == max(exact, key=exact.get)                      # reference top gap >= 0.06 nat
        assert all(np.isneginf(s) for p, s in got.items() if p not in exact)
        assert (ln[b, n_prefixes:] == 0).all() and np.isneginf(sc[b, n_prefixes:]).all()


# ---------------------------------------------------------------------------------------- 2. identity
def test_prefix_identity_is_string_equality(dev):
    logits = BR.identity_logits()[None]
    ref, gap, _ = BR.beam_ref(LR.log_probs_ref(logits[0]), BR.IDENTITY_BEAM)
    lab, ln, sc = decode(dev, logits, BR.IDENTITY_BEAM)
    assert string(lab, ln, 0, 0) == (0, 1, 0, 1) == ref[0][1]
    close_scores(sc[0, :1], [-1.6140276972016037], "the 1840 case: top score")
    assert [string(lab, ln, 0, r) for r in range(3)] == [p for _, p in ref]           # gaps 0.36 and 0.32 nat
    close_scores(sc[0], [s for s, _ in ref], "the 1840 case: scores")


# ---------------------------------------------------------------------------------------- 3. parity with a guard
def check_parity(case, lab, ln, sc, name):
    compared_strings = 0
    for b in case["compared"]:
        survivors = case["ref"][b][0]
        print("%s sample %d: max |score error| %.3e" % (name, b, max(abs(sc[b, r] - survivors[r][0]) for r in range(len(survivors)))))
        close_scores(sc[b], [s for s, _ in survivors], "%s sample %d: nbest scores" % (name, b))
        for r, (_, prefix) in enumerate(survivors):
            if BR.rank_is_checked(survivors, r):
                assert string(lab, ln, b, r) == prefix, "%s sample %d rank %d: %s, reference %s" % (name, b, r, string(lab, ln, b, r), prefix)
                compared_strings += 1
    return compared_strings


@pytest.mark.parametrize("name,kind,T,C,beam,seed", BR.PARITY_CASES)
def test_parity_with_the_reference(dev, name, kind, T, C, beam, seed):
    """("cut4096": C = 64, beam = 64, T = 7 noise at seed beam_refs.CUT_4096_SEED, 4096 candidates per cut.)"""
    case = BR.parity_case(kind, T, C, beam, seed)
    assert 8 - len(case["compared"]) <= BR.MAX_LEFT_OUT and sum(r[2] for r in case["ref"]) > 0
    lab, ln, sc = decode(dev, case["logits"], beam, lm=case["lm"], order=case["order"], lm_weight=case["lm_weight"], len_bonus=case["len_bonus"])
    n = check_parity(case, lab, ln, sc, "%s T=%d C=%d beam=%d seed=%d" % (name, T, C, beam, seed))
    assert n >= 4, "only %d strings were compared" % n              # (tests/test_beam_cpu.py: at least 4 top strings are)


# ---------------------------------------------------------------------------------------- 4. planted words
@pytest.mark.parametrize("beam", [1, 8, 64])
def test_planted_words_are_read(dev, beam):
    """Gain 8, no LM: the top read is the planted word and the best path; a beam can only lose mass, so its score is at most the
    word's full CTC log-likelihood."""
    from scrabble_gan_amd import ops
    case = BR.parity_case("planted", 19, 53, 8, 0)
    logits = case["logits"]
    lab, ln, sc = decode(dev, logits, beam, nbest=1)
    x = torch.from_numpy(logits).to(dev)
    g_lab, g_len, _ = ops.ctc_greedy_decode(x)
    words = np.full((8, 5), -1, np.int32)
    for b, w in enumerate(LR.PLANTED_WORDS):
        words[b, :len(w)] = w
    nll = ops.ctc_score_words(ops.ctc_log_probs(x), torch.from_numpy(words).to(dev),
                              torch.tensor([len(w) for w in LR.PLANTED_WORDS], dtype=torch.int32, device=dev)).cpu().numpy()
    for b, w in enumerate(LR.PLANTED_WORDS):
        assert string(lab, ln, b, 0) == tuple(w) == tuple(int(c) for c in g_lab[b, :g_len[b]].cpu())
        assert sc[b, 0] <= -nll[b, b] + TOL * max(1.0, abs(nll[b, b])), (b, sc[b, 0], -nll[b, b])
        if beam == 8:
            close_scores(sc[b, :1], [case["ref"][b][0][0][0]], "planted sample %d: top score" % b)


# ---------------------------------------------------------------------------------------- 5. uniform LM
@pytest.mark.parametrize("order", [1, 2, 3])
def test_uniform_lm_changes_nothing_but_the_end_of_word_term(dev, order):
    """Every table entry -log C, lm_weight 1, len_bonus log C: each character's credit is fl(log C) - fl(log C) = 0, so the search
    is the one without an LM and every score is lower by the end-of-word term log C."""
    case = BR.parity_case("planted", 19, 53, 8, 0)
    C = 53
    logc = float(np.float32(math.log(C)))
    lm = np.full((C ** (order - 1), C), -logc, np.float32)
    lab0, ln0, sc0 = decode(dev, case["logits"], 8)
    lab1, ln1, sc1 = decode(dev, case["logits"], 8, lm=lm, order=order, lm_weight=1.0, len_bonus=logc)
    for b in case["compared"]:
        assert np.array_equal(lab0[b], lab1[b]) and np.array_equal(ln0[b], ln1[b])
        close_scores(sc1[b], sc0[b].astype(np.float64) - logc, "uniform LM order %d sample %d" % (order, b))
    check_parity(case, lab0, ln0, sc0, "planted, no LM")
    check_parity(dict(case, ref=[([(s - logc, p) for s, p in r[0]], r[1], r[2]) for r in case["ref"]]), lab1, ln1, sc1, "planted, uniform LM")


# ---------------------------------------------------------------------------------------- 6. edges
def test_edges(dev):
    case = BR.parity_case("planted", 19, 53, 8, 0)
    logits = case["logits"]
    full = decode(dev, logits, 8)
    # B = 1: a sample's result does not depend on its batch
    one = decode(dev, logits[3:4], 8)
    assert all(np.array_equal(a[0], f[3]) for a, f in zip(one, full))
    # nbest < beam: the first rows of the same search
    lab, ln, sc = decode(dev, logits, 8, nbest=3)
    assert np.array_equal(lab, full[0][:, :3]) and np.array_equal(ln, full[1][:, :3]) and np.array_equal(sc, full[2][:, :3])
    # beam = 1 on noise: one string, the reference's where its per-frame gap allows
    noise = BR.parity_case("noise", 11, 53, 8, 0)["logits"]
    lab, ln, sc = decode(dev, noise, 1)
    lp = LR.log_probs_ref(noise)
    compared = 0
    for b in range(8):
        ref, gap, _ = BR.beam_ref(lp[b], 1)
        if gap >= BR.GUARD:
            assert string(lab, ln, b, 0) == ref[0][1]
            close_scores(sc[b], [ref[0][0]], "beam 1 sample %d" % b)
            compared += 1
    assert compared >= 6
    # C = 2: one character and the blank
    two = np.float32(np.random.default_rng(5).standard_normal((4, 9, 2)) * 2)
    lab, ln, sc = decode(dev, two, 4)
    for b in range(4):
        ref, gap, _ = BR.beam_ref(LR.log_probs_ref(two[b]), 4)
        assert gap >= BR.GUARD, "fixture: C = 2 sample %d has a cut gap of %.2e" % (b, gap)
        close_scores(sc[b], [s for s, _ in ref], "C = 2 sample %d" % b)
        assert all(string(lab, ln, b, r) == ref[r][1] for r in range(4) if BR.rank_is_checked(ref, r))
    # input_length < T: the frames behind it do not matter, even as NaN
    poisoned = np.concatenate([logits[:, :11], np.full((8, 8, 53), np.nan, np.float32)], 1)
    a = decode(dev, poisoned, 8, input_length=11)
    b = decode(dev, np.ascontiguousarray(logits[:, :11]), 8)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    # an all-blank rendering reads as the empty string
    blank = np.float32(np.random.default_rng(6).standard_normal((2, 19, 53)))
    blank[:, :, 52] += 8.0
    lab, ln, sc = decode(dev, blank, 8)
    assert (ln[:, 0] == 0).all() and (lab[:, 0] == -1).all()
    ref = BR.beam_ref(LR.log_probs_ref(blank[0]), 8)[0]
    assert ref[0][1] == ()
    close_scores(sc[0, :1], [ref[0][0]], "empty-string winner")


def test_out_stride_padding_and_frame_limit(dev):
    """The C-ABI: an out_stride wider than input_length is filled with -1; input_length = 256 is taken (top read against the
    reference on a strongly planted path), 257 is SG_ERR_UNSUPPORTED."""
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import ScrabbleHipError, call
    case = BR.parity_case("planted", 19, 53, 8, 0)
    lp = ops.ctc_log_probs(torch.from_numpy(case["logits"]).to(dev))
    want = ops.ctc_beam_decode(lp, beam=8, nbest=2)
    lab = torch.full((8, 2, 40), 77, device=dev, dtype=torch.int32)
    ln = torch.full((8, 2), 77, device=dev, dtype=torch.int32)
    sc = torch.full((8, 2), 77.0, device=dev)
    call("sg_ctc_beam_decode", lp.data_ptr(), 8, 19, 53, 19, 8, None, 1, 0.0, 0.0, lab.data_ptr(), ln.data_ptr(), sc.data_ptr(), 2, 40, None, ops._stream())
    assert torch.equal(lab[:, :, :19], want[0]) and (lab[:, :, 19:] == -1).all() and torch.equal(ln, want[1]) and torch.equal(sc, want[2])

    T, C = 256, 5
    rng = np.random.default_rng(9)
    x = np.float32(rng.standard_normal((1, T + 1, C)))
    path = [C - 1] * (T + 1)
    word = []
    for t in range(3, T, 8):
        c = int(rng.integers(0, C - 1))
        path[t] = path[t + 1] = c
        word.append(c)
    x[0, np.arange(T + 1), path] += 8.0
    ref, gap, _ = BR.beam_ref(LR.log_probs_ref(x[0, :T]), 4)
    assert gap >= BR.GUARD and ref[0][1] == tuple(word) and len(word) == 32 and ref[0][0] - ref[1][0] >= BR.GUARD
    lab, ln, sc = decode(dev, x, 4, input_length=256)
    assert string(lab, ln, 0, 0) == tuple(word)
    close_scores(sc[0], [s for s, _ in ref], "input_length 256")
    assert ops.lib().sg_ctc_beam_workspace_bytes(1, 256, 4) >= 0 and ops.lib().sg_ctc_beam_workspace_bytes(1, 257, 4) == -1
    lp = ops.ctc_log_probs(torch.from_numpy(x).to(dev))
    lab = torch.full((1, 1, 257), 77, device=dev, dtype=torch.int32)
    ln = torch.full((1, 1), 77, device=dev, dtype=torch.int32)
    sc = torch.full((1, 1), 77.0, device=dev)
    with pytest.raises(ScrabbleHipError, match="SG_ERR_UNSUPPORTED"):
        call("sg_ctc_beam_decode", lp.data_ptr(), 1, 257, C, 257, 4, None, 1, 0.0, 0.0, lab.data_ptr(), ln.data_ptr(), sc.data_ptr(), 1, 257, None, ops._stream())
    with pytest.raises(ValueError):
        ops.ctc_beam_decode(lp, 257, beam=4)
    torch.cuda.synchronize()
    assert (lab == 77).all() and (ln == 77).all() and (sc == 77.0).all()


def test_bad_arguments_are_refused_before_any_launch(dev):
    """Every SG_ERR_ARG row of the header, on sentinel-filled outputs that stay untouched; then the host-side checks of ops."""
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import ScrabbleHipError, call
    B, T, C = 2, 5, 7
    lp = ops.ctc_log_probs(torch.randn(B, T, C, device=dev))
    lm = torch.zeros(C, C, device=dev)
    lab = torch.full((B, 4, T), 77, device=dev, dtype=torch.int32)
    ln = torch.full((B, 4), 77, device=dev, dtype=torch.int32)
    sc = torch.full((B, 4), 77.0, device=dev)
    good = dict(lp=lp.data_ptr(), B=B, T=T, C=C, input_length=T, beam=4, lm=None, lm_order=1, lm_weight=0.0, len_bonus=0.0,
                out_labels=lab.data_ptr(), out_len=ln.data_ptr(), out_score=sc.data_ptr(), nbest=4, out_stride=T, workspace=None)
    bad = [dict(lp=None), dict(out_labels=None), dict(out_len=None), dict(out_score=None), dict(B=0), dict(C=1), dict(C=65), dict(beam=0),
           dict(beam=65), dict(nbest=0), dict(nbest=5), dict(input_length=0), dict(input_length=T + 1), dict(out_stride=T - 1),
           dict(lm=lm.data_ptr(), lm_order=0), dict(lm=lm.data_ptr(), lm_order=4)]
    for change in bad:
        args = dict(good, **change)
        with pytest.raises(ScrabbleHipError, match="SG_ERR_ARG"):
            call("sg_ctc_beam_decode", *args.values(), ops._stream())
    torch.cuda.synchronize()
    assert (lab == 77).all() and (ln == 77).all() and (sc == 77.0).all()
    assert [ops.lib().sg_ctc_beam_workspace_bytes(*a) for a in ((0, 5, 4), (1, 0, 4), (1, 5, 0), (1, 5, 65))] == [-1] * 4
    call("sg_ctc_beam_decode", *dict(good, lm_order=9).values(), ops._stream())         # without an lm its order is not read
    assert (ln != 77).all()
    for kw in (dict(input_length=T + 1), dict(beam=0), dict(beam=65), dict(beam=4, nbest=5), dict(nbest=0), dict(lm=lm, lm_order=4),
               dict(lm=lm, lm_order=3), dict(lm=lm.double(), lm_order=2), dict(lm=lm.t(), lm_order=2), dict(lm=lm.cpu(), lm_order=2)):
        with pytest.raises(ValueError):
            ops.ctc_beam_decode(lp, **kw)
    with pytest.raises(ValueError):
        ops.ctc_beam_decode(lp.double())


# ---------------------------------------------------------------------------------------- 7. reproducibility
def test_two_calls_agree_bitwise(dev):
    from scrabble_gan_amd import ops
    for kind, T, C, beam, seed in (("trigram", 19, 53, 8, 0), ("noise", 7, 64, 64, BR.CUT_4096_SEED)):
        case = BR.parity_case(kind, T, C, beam, seed)
        lp = ops.ctc_log_probs(torch.from_numpy(case["logits"]).to(dev))
        lm = None if case["lm"] is None else torch.from_numpy(case["lm"]).to(dev)
        kw = dict(beam=beam, lm=lm, lm_order=case["order"], lm_weight=case["lm_weight"], len_bonus=case["len_bonus"], nbest=beam)
        a = ops.ctc_beam_decode(lp, **kw)
        b = ops.ctc_beam_decode(lp, **kw)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


# ---------------------------------------------------------------------------------------- 8. through the models
@pytest.mark.parametrize("which", ["recognizer", "my_recognizer"])
def test_models_transcribe_beam_and_legibility(dev, which):
    """L = 2, B = 4: transcribe_beam is ops.ctc_beam_decode on the model's own logits and default frames; evaluate_recognizer
    gains cer_beam / wer_beam with beam > 0 and returns today's keys without."""
    from scrabble_gan_amd import legibility, net_architecture as NA, ops
    NA.configure(device=dev, seed=3)
    R = (NA.make_recognizer if which == "recognizer" else NA.make_my_recognizer)((32, 32, 1), None, 53, vis_model=False)
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.uniform(-1, 1, (4, 32, 32, 1)).astype(np.float32)).to(dev)
    labels = rng.integers(0, 52, (4, 2)).astype(np.int32)
    lm = legibility.CharLM.from_words(["ab", "abc", "Zq", "cat"], CV, order=2).to(dev)
    ops.set_deterministic(True)
    try:
        logits = R.logits(x)
        frames = R._ctc_frames(logits.shape[1])
        got = R.transcribe_beam(x, beam=8, lm=lm, lm_weight=0.5, len_bonus=0.25, nbest=3)
        want = ops.ctc_beam_decode(ops.ctc_log_probs(logits), frames, beam=8, lm=lm.table, lm_order=2, lm_weight=0.5, len_bonus=0.25, nbest=3)
        plain = R.transcribe_beam(x)
        short = R.transcribe_beam(x, beam=4, input_length=5)
        greedy = R.transcribe(x)
        with_beam = legibility.evaluate_recognizer(R, [(x, labels)], CV, beam=8, lm=lm, lm_weight=0.5, len_bonus=0.25)
        without = legibility.evaluate_recognizer(R, [(x, labels)], CV)
        # the same rates from the rows transcribe_beam returns
        top = R.transcribe_beam(x, beam=8, lm=lm, lm_weight=0.5, len_bonus=0.25)
    finally:
        ops.set_deterministic(False)
    assert frames == 7 and got[0].shape == (4, 3, 7) and plain[0].shape == (4, 1, 7) and short[0].shape == (4, 1, 5)
    assert all(torch.equal(u, v) for u, v in zip(got, want))
    assert greedy[0].shape == (4, 7)
    assert set(without) == {"cer", "wer", "n_words", "n_chars"}
    assert set(with_beam) == set(without) | {"cer_beam", "wer_beam"} and all(with_beam[k] == without[k] for k in without)
    d = [LR.edit_distance_ref(top[0][b, 0, :top[1][b, 0]].tolist(), labels[b]) for b in range(4)]
    assert with_beam["cer_beam"] == sum(d) / 8 and with_beam["wer_beam"] == sum(v != 0 for v in d) / 4
    assert math.isfinite(with_beam["cer_beam"]) and math.isfinite(with_beam["wer_beam"])


def test_read_back_with_a_beam(dev):
    from scrabble_gan_amd import legibility, net_architecture as NA
    in_dim = (32, 160, 1)
    NA.configure(device=dev, seed=6)
    G = NA.make_generator(128, in_dim, (32, 8192), None, "B3", 52, vis_model=False)
    R = NA.make_recognizer(in_dim, None, 53, vis_model=False)
    style = np.random.default_rng(2).uniform(-1, 1, (2,) + in_dim).astype(np.float32)
    lm = legibility.CharLM.from_words(["ab", "de", "c"], CV, order=3).to(dev)
    with legibility.preserved_rng(G, R):
        plain = legibility.read_back(G, R, style, ["ab", "c", "de"], CV)
    with legibility.preserved_rng(G, R):
        rows = legibility.read_back(G, R, style, ["ab", "c", "de"], CV, beam=8, lm=lm, lm_weight=0.3)
    assert all(set(r) == {"target", "read", "distance"} for r in plain)
    for r in rows:
        assert set(r) == {"target", "read", "distance", "read_beam", "distance_beam", "score_beam"}
        assert set(r["read_beam"]) <= set(CV) and r["distance_beam"] == LR.edit_distance_ref(r["read_beam"], r["target"])
        assert math.isfinite(r["score_beam"]) and r["score_beam"] < 0
