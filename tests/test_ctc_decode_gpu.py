"""Reading the recognizer on the GPU (csrc/ctc_decode.hip -> ops -> RecognizerModel -> legibility / train): best-path
decoding, lexicon scores, edit distance and the fp64 metric sums against plain numpy / Python references
(tests/legibility_refs.py) and the fp64 CPU oracle's K.ctc_batch_cost.

Integer outputs (labels, lengths, distances, the sums) must be EXACT.  Float outputs (lp, out_logp, nll) are held with the
`close` helper of tests/test_ops_gpu.py at its default 2e-5 of the reference's largest entry -- the bound test_softmax_ctc
holds the CTC loss to; infinities compare by isinf on both sides."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import scrabble_oracle as O  # noqa: E402  (checker only)
from tests import legibility_refs as LR  # noqa: E402
from tests.test_ops_gpu import close  # noqa: E402

TOL = 2e-5          # `close`'s default


def close_inf(got, ref, name):
    """`close` on the finite entries; +inf must sit at the same places on both sides."""
    got, ref = got.detach().double().cpu(), torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert not torch.isnan(got).any(), name
    gi, ri = torch.isinf(got), torch.isinf(ref)
    assert torch.equal(gi, ri) and (got[gi] > 0).all(), "%s: infinities differ" % name
    close(torch.where(gi, torch.zeros_like(got), got), torch.where(ri, torch.zeros_like(ref), ref), name=name)


def oracle_scores(logits, lexicon, T):
    """[B,W] K.ctc_batch_cost (fp64, CPU) of every lexicon word on softmax(logits); one call per word, its own length."""
    probs = torch.softmax(torch.from_numpy(np.asarray(logits)).double(), -1)
    B = probs.shape[0]
    out = torch.empty(B, len(lexicon), dtype=torch.float64)
    for w, word in enumerate(lexicon):
        out[:, w] = O.ctc_batch_cost(torch.tensor([list(word)] * B), probs, T, len(word))[:, 0]
    return out


def dev_i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def check_decode(dev, logits, input_length=None, name=""):
    from scrabble_gan_amd import ops
    want_lab, want_len, want_logp = LR.greedy_ref(logits, input_length)
    lab, ln, logp = ops.ctc_greedy_decode(torch.from_numpy(logits).to(dev), input_length)
    assert lab.dtype == torch.int32 and ln.dtype == torch.int32
    assert np.array_equal(ln.cpu().numpy(), want_len), (name, ln.cpu().numpy(), want_len)
    assert np.array_equal(lab.cpu().numpy(), want_lab), name
    close(logp, torch.from_numpy(want_logp), name=name + " logp")
    close(ops.ctc_log_probs(torch.from_numpy(logits).to(dev)), torch.from_numpy(LR.log_probs_ref(logits)), name=name + " lp")
    return want_lab, want_len, logp


# ---------------------------------------------------------------------------------------- greedy decode
@pytest.mark.parametrize("B,T,C,input_length", [(5, 3, 2, None), (4, 19, 53, None), (4, 19, 53, 11), (4, 64, 53, None),
                                                (4, 65, 53, None), (3, 91, 53, None), (3, 123, 64, None)])
def test_greedy_decode_shapes(dev, B, T, C, input_length):
    """Random rows (blank favoured at the long shapes so that the decoded words stay within softmax_ctc's 31 characters), row 0 all
    blank, row 1 one character on every frame; with input_length < T the ignored frames shout a non-blank class.
    Property: the best path is ONE alignment of the word it decodes to, so the CTC loss of that word <= -logp(best path)."""
    from scrabble_gan_amd import ops
    rng = np.random.default_rng(1000 * T + C)
    logits = (rng.standard_normal((B, T, C)) * 2).astype(np.float32)
    if T > 31:
        logits[:, :, C - 1] += 7.0
    logits[0, :, C - 1] += 30.0
    logits[1, :, 0] += 30.0
    il = T if input_length is None else input_length
    if il < T:
        logits[:, il:, :] = -1e3
        logits[:, il:, 1 % (C - 1)] = 1e3
    lab, ln, logp = check_decode(dev, logits, input_length, "greedy %s" % ((B, T, C, input_length),))
    assert ln[0] == 0 and (lab[0] == -1).all() and ln[1] == 1 and lab[1, 0] == 0
    checked = 0
    x = torch.from_numpy(logits).to(dev)
    for b in range(B):
        n = int(ln[b])
        if 1 <= n <= 31:
            loss, _ = ops.softmax_ctc(x[b:b + 1].contiguous(), dev_i32(lab[b:b + 1, :n], dev), il, n, need_grad=False)
            bound = -logp[b].item()
            assert loss.item() <= bound + TOL * max(1.0, abs(bound)), (b, loss.item(), bound)
            checked += 1
    assert checked >= 2, "the property ran on %d rows" % checked


def test_greedy_decode_planted_rows(dev):
    """T = 91 (two chunks of frames), C = 53: every row is quiet noise with +8 on a planted path."""
    T, C = 91, 53
    blank = C - 1
    rng = np.random.default_rng(5)

    def row(path):
        x = (rng.standard_normal((T, C)) * 0.1).astype(np.float32)
        x[np.arange(T), path] += 8.0
        return x

    def path(**at):
        p = [blank] * T
        for t, c in at.items():
            p[int(t[1:])] = c
        return p
    free = [int(c) for c in rng.integers(0, blank, T)]
    rows = [(path(), []),                                            # all blank
            ([4] * T, [4]),                                          # one character on every frame
            (path(t0=0, t2=0), [0, 0]),                              # a, blank, a
            (path(t63=9, t64=9), [9]),                               # merged across the chunk carry
            (path(t63=9, t64=10), [9, 10]),
            (path(t62=9, t64=9), [9, 9]),                            # blank on frame 63: not merged
            (free, [c for i, c in enumerate(free) if i == 0 or c != free[i - 1]])]     # no blank anywhere
    tie = row(path())
    tie[40, :] = 0.0
    tie[40, 17] = tie[40, 5] = 3.0                                   # exact two-way tie: the lowest index wins
    logits = np.stack([row(p) for p, _ in rows] + [tie], 0)
    want = [w for _, w in rows] + [[5]]
    lab, ln, _ = check_decode(dev, logits, None, "planted")
    for b, w in enumerate(want):
        assert list(lab[b, :ln[b]]) == w, (b, list(lab[b, :ln[b]]), w)


def test_greedy_decode_rejects_bad_arguments(dev):
    from scrabble_gan_amd import ops
    from scrabble_gan_amd._lib import ScrabbleHipError, call
    x = torch.zeros(2, 5, 7, device=dev)
    with pytest.raises(ValueError):
        ops.ctc_greedy_decode(x, 6)
    lab, ln = torch.empty(2, 4, device=dev, dtype=torch.int32), torch.empty(2, device=dev, dtype=torch.int32)
    with pytest.raises(ScrabbleHipError, match="SG_ERR_ARG"):       # out_stride < input_length
        call("sg_ctc_greedy_decode", x.data_ptr(), lab.data_ptr(), ln.data_ptr(), None, 2, 5, 7, 5, 4, ops._stream())


# ---------------------------------------------------------------------------------------- score words
@pytest.fixture(scope="module")
def lexicon_case():
    """C = 53, Lmax = 5, T = 19, B = 8, W = 67 (seed picked on the CPU for the oracle alone: smallest best-to-second gap 4.5 nats)."""
    logits, lexicon, planted = LR.lexicon_problem(0)
    return logits, lexicon, planted, oracle_scores(logits, lexicon, 19)


def pack(lexicon):
    stride = max(len(w) for w in lexicon)
    words = np.full((len(lexicon), stride), -1, np.int32)
    for i, w in enumerate(lexicon):
        words[i, :len(w)] = w
    return words, np.array([len(w) for w in lexicon], np.int32)


def test_score_words_against_the_oracle(dev, lexicon_case):
    from scrabble_gan_amd import ops
    logits, lexicon, planted, ref = lexicon_case
    assert len({tuple(w) for w in lexicon}) == len(lexicon) == 67 and {len(w) for w in lexicon} == {1, 2, 3, 4, 5}
    srt = torch.sort(ref, 1).values
    assert (srt[:, 1] - srt[:, 0]).min().item() >= 1.0, "fixture: the oracle's best-to-second gap fell below 1 nat"
    assert ref.argmin(1).tolist() == planted
    words, word_len = pack(lexicon)
    x = torch.from_numpy(logits).to(dev)
    nll = ops.ctc_score_words(ops.ctc_log_probs(x), dev_i32(words, dev), dev_i32(word_len, dev))
    close_inf(nll, ref, "nll [B,W]")
    assert nll.argmin(1).tolist() == planted
    # W = 1
    one = ops.ctc_score_words(ops.ctc_log_probs(x), dev_i32(words[5:6], dev), dev_i32(word_len[5:6], dev))
    close_inf(one, ref[:, 5:6], "nll W=1")
    # all words of one length: the training loss of the same labels
    for L in (1, 3, 5):
        idx = [i for i, w in enumerate(lexicon) if len(w) == L]
        for i in idx[:4]:
            loss, _ = ops.softmax_ctc(x, dev_i32([lexicon[i]] * x.shape[0], dev), 19, L, need_grad=False)
            close(nll[:, i], loss, name="score_words vs softmax_ctc, word %d" % i)


def test_score_words_infinities(dev):
    """T = 7: a five-fold repeated letter needs 9 frames (+inf on both sides, never NaN); labels equal to the blank, labels
    below 0 and lengths outside [1, stride] are poisoned with +inf; input_length < T is honoured."""
    from scrabble_gan_amd import ops
    C, T, B = 53, 7, 3
    rng = np.random.default_rng(11)
    logits = rng.standard_normal((B, T, C)).astype(np.float32)
    lexicon = [[4, 4, 4, 4, 4], [4, 5, 4], [9], [4, 4, 4, 4]]        # infeasible, fine, fine, exactly 7 frames
    ref = oracle_scores(logits, lexicon, T)
    assert torch.isinf(ref[:, 0]).all() and torch.isfinite(ref[:, 1:]).all()
    words, word_len = pack(lexicon)
    x = torch.from_numpy(logits).to(dev)
    lp = ops.ctc_log_probs(x)
    close_inf(ops.ctc_score_words(lp, dev_i32(words, dev), dev_i32(word_len, dev)), ref, "nll T=7")
    close_inf(ops.ctc_score_words(lp, dev_i32(words, dev), dev_i32(word_len, dev), 5), oracle_scores(logits, lexicon, 5), "nll input_length=5")
    bad_words = np.array([[4, C - 1, 4, 0, 0], [4, -1, 4, 0, 0], [1, 2, 3, 4, 5], [1, 2, 3, 4, 5], [4, 5, 4, 0, 0]], np.int32)
    bad_len = np.array([3, 3, 0, 6, 3], np.int32)
    got = ops.ctc_score_words(lp, dev_i32(bad_words, dev), dev_i32(bad_len, dev)).cpu()
    assert torch.isinf(got[:, :4]).all() and (got[:, :4] > 0).all()
    close(got[:, 4], ref[:, 1], name="the good word beside the poisoned ones")


# ---------------------------------------------------------------------------------------- edit distance + sums
def run_edit(dev, pairs, hyp_stride=None, ref_stride=None):
    from scrabble_gan_amd import ops
    hs = hyp_stride or max(1, max(len(h) for h, _ in pairs))
    rs = ref_stride or max(1, max(len(r) for _, r in pairs))
    hyp, ref = np.full((len(pairs), hs), -7, np.int32), np.full((len(pairs), rs), -9, np.int32)
    for i, (h, r) in enumerate(pairs):
        hyp[i, :len(h)] = h
        ref[i, :len(r)] = r
    hl, rl = np.array([len(h) for h, _ in pairs], np.int32), np.array([len(r) for _, r in pairs], np.int32)
    return ops.edit_distance(dev_i32(hyp, dev), dev_i32(hl, dev), dev_i32(ref, dev), dev_i32(rl, dev)), rl


def test_edit_distance(dev):
    from scrabble_gan_amd._lib import ScrabbleHipError
    o = lambda s: [ord(c) for c in s]
    hand = [(o(""), o("")), (o(""), o("abc")), (o("abc"), o("")), (o("handwriting"), o("handwriting")), (o("kitten"), o("sitting"))]
    d, _ = run_edit(dev, hand)
    assert d.dtype == torch.int32 and d.tolist() == [0, 3, 3, 0, 3]
    rng = np.random.default_rng(3)
    pairs = [(list(rng.integers(0, 4, int(rng.integers(0, 40)))), list(rng.integers(0, 4, int(rng.integers(0, 40))))) for _ in range(32)]
    pairs.append((list(rng.integers(0, 3, 123)), list(rng.integers(0, 3, 63))))          # the limits: ref_len 63, hyp_len 123
    assert len(pairs) == 33
    d, _ = run_edit(dev, pairs)
    assert d.tolist() == [LR.edit_distance_ref(h, r) for h, r in pairs]
    with pytest.raises(ScrabbleHipError, match="SG_ERR_UNSUPPORTED"):
        run_edit(dev, hand, ref_stride=64)


def test_legibility_sums_are_additive_and_exact(dev):
    from scrabble_gan_amd import ops
    rng = np.random.default_rng(4)
    sums = torch.zeros(4, device=dev, dtype=torch.float64)
    want = np.zeros(4)
    for B in (33, 700):
        dist, ref_len = rng.integers(0, 5, B).astype(np.int32), rng.integers(1, 24, B).astype(np.int32)
        out = ops.legibility_sums(dev_i32(dist, dev), dev_i32(ref_len, dev), sums)
        assert out is sums
        want += [dist.sum(), ref_len.sum(), (dist != 0).sum(), B]
    assert sums.cpu().numpy().tolist() == want.tolist()


# ---------------------------------------------------------------------------------------- models
@pytest.mark.parametrize("which", ["recognizer", "my_recognizer"])
def test_model_logits_transcribe_score_words(dev, which):
    """Input (32, 32, 1): L = 2, the CTC head reads T = 7 frames; B = 3.  Deterministic conv kernels, so that two forward passes
    agree bitwise and `transcribe` can be held EXACTLY to the numpy decode of the logits `logits` returned."""
    from scrabble_gan_amd import net_architecture as NA, ops
    from tests.test_nets_gpu import close as close_net, perturb
    NA.configure(device=dev, seed=3)
    gen = torch.Generator().manual_seed(21)
    make, probs, tol = ((NA.make_recognizer, O.recognizer_probs, 1e-4) if which == "recognizer"
                        else (NA.make_my_recognizer, O.my_recognizer_probs, 2e-4))       # the forward bounds of tests/test_nets_gpu.py
    R = make((32, 32, 1), None, 53, vis_model=False)
    P = perturb(R, gen)
    B, L, T = 3, 2, 7
    x = torch.rand(B, 32, 16 * L, 1, generator=gen, dtype=torch.float64) * 2 - 1
    xg = x.float().to(dev)
    labels = torch.randint(0, 52, (B, L), generator=gen).int().to(dev)
    stats = {k: R.store.p[k].clone() for k in R.store.names if k.endswith((".mm", ".mv"))}
    ops.set_deterministic(True)
    try:
        before = R.forward(xg, labels, T, L, training=False, need_grad=False)[0].clone()
        logits = R.logits(xg)
        lab, ln, logp = R.transcribe(xg)
        lexicon = [[1], [2, 3], [4, 4], [5, 6, 7]]
        words, word_len = pack(lexicon)
        nll = R.score_words(xg, words, word_len)
        after = R.forward(xg, labels, T, L, training=False, need_grad=False)[0]
        cost = torch.stack([R.forward(xg, dev_i32([w] * B, dev), T, len(w), training=False, need_grad=False)[0] for w in lexicon[:3]], 1)
    finally:
        ops.set_deterministic(False)
    assert logits.shape[0] == B and logits.shape[2] == 53 and logits.shape[1] == (7 if which == "recognizer" else 8)
    close_net(torch.softmax(logits.double(), -1), probs(x, P), tol, "softmax(logits) " + which)
    want_lab, want_len, want_logp = LR.greedy_ref(logits.cpu().numpy(), T)
    assert np.array_equal(lab.cpu().numpy(), want_lab) and np.array_equal(ln.cpu().numpy(), want_len)
    close(logp, torch.from_numpy(want_logp), name="transcribe logp")
    close(nll[:, :3], cost, name="score_words vs the model's own CTC cost")       # [5,6,7] needs no more than 7 frames either:
    assert torch.isfinite(nll).all()
    assert torch.equal(before, after), "forward's cost moved after logits / transcribe / score_words"
    for k, v in stats.items():
        assert torch.equal(R.store.p[k], v), "moving statistic %s changed" % k


def test_evaluate_recognizer_with_a_lexicon(dev):
    """legibility.evaluate_recognizer over two batches of different word lengths against the same rates computed on the host from
    the frames R.logits returns (numpy best path, textbook distance; the lexicon read = row argmin of the downloaded scores)."""
    from scrabble_gan_amd import legibility, net_architecture as NA, ops
    NA.configure(device=dev, seed=3)
    R = NA.make_recognizer((32, 32, 1), None, 53, vis_model=False)
    cv = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'
    rng = np.random.default_rng(8)
    batches = [(rng.uniform(-1, 1, (3, 32, 16 * L, 1)).astype(np.float32), rng.integers(0, 52, (3, L)).astype(np.int32)) for L in (2, 1)]
    lexicon = ["a", "to", "Zq", "cat", "b"]
    words, word_len = legibility.pack_words(lexicon, cv)
    want = {"d": 0, "chars": 0, "wrong": 0, "n": 0, "d_lex": 0, "wrong_lex": 0}
    ops.set_deterministic(True)
    try:
        got = legibility.evaluate_recognizer(R, batches, cv, lexicon)
        for x, y in batches:
            logits = R.logits(torch.from_numpy(x).to(dev))
            lab, ln, _ = LR.greedy_ref(logits.cpu().numpy())
            best = R.score_words(torch.from_numpy(x).to(dev), words, word_len).cpu().numpy().argmin(1)
            for b in range(len(y)):
                d = LR.edit_distance_ref(lab[b, :ln[b]], y[b])
                dl = LR.edit_distance_ref(words[best[b], :word_len[best[b]]], y[b])
                want["d"] += d; want["wrong"] += d != 0; want["d_lex"] += dl; want["wrong_lex"] += dl != 0
                want["chars"] += len(y[b]); want["n"] += 1
    finally:
        ops.set_deterministic(False)
    assert got == {"cer": want["d"] / want["chars"], "wer": want["wrong"] / want["n"], "n_words": 6, "n_chars": 9,
                   "cer_lexicon": want["d_lex"] / want["chars"], "wer_lexicon": want["wrong_lex"] / want["n"]}


# ---------------------------------------------------------------------------------------- the train loop's hook
def test_train_legibility_hook(dev, tmp_path):
    """train(..., legibility_every=1): one epoch of two batches at batch size 4 on the synthetic dataset writes legibility.csv
    (header + one finite row); the twin run with legibility_every=0 writes none; same summaries, same final weights
    (deterministic mode; both runs start from one set of initial weights and the same host / generator seeds)."""
    from scrabble_gan_amd import data_utils as DU, legibility, net_architecture as NA, net_loss, ops, optimizers
    from scrabble_gan_amd.main import synthetic_dataset
    in_dim, bs, bucket = (32, 160, 1), 4, 3
    cv = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'
    NA.configure(device=dev, seed=6, deterministic=True)
    try:
        G = NA.make_generator(128, in_dim, (32, 8192), None, "B3", 52, vis_model=False)
        D = NA.make_discriminator(in_dim, None, "B1", vis_model=False)
        R = NA.make_recognizer(in_dim, None, 53, vis_model=False)
        S = NA.make_style_promoter(in_dim, None, "B1", vis_model=False)
        gan = NA.make_gan(G, D, R, S, vis_model=False)
        models = (G, D, R, S)
        snap = [(m.store.flat.clone(), m.store.state.clone()) for m in models]
        words = DU.synthetic_random_words(bucket, 20, seed=2)
        my_imgs = [DU.synthetic_batch(1, 10, in_dim, 52, seed=50 + i)[2][0] for i in range(6)]
        res = {}
        for every in (1, 0):
            for m, (flat, state) in zip(models, snap):
                m.store.flat.copy_(flat)
                m.store.state.copy_(state)
            ops.weights_changed()
            random.seed(12)
            np.random.seed(12)
            torch.manual_seed(12)
            for i, m in enumerate((G, D, S)):
                m.nl_gen.manual_seed(77 + i)
            opts = [optimizers.Adam(2e-4, 0.0, 0.999) for _ in range(4)]
            out = tmp_path / ("every%d" % every)
            DU.train(synthetic_dataset(bs, in_dim, bucket, 52, seed=3), G, D, R, S, gan, None, str(out / "ckpt"), opts[0], opts[1], opts[2],
                     opts[3], my_imgs, [None, None], 4, bs, 1, str(out / "model"), 128, str(out / "gen"), net_loss.hinge, 1, 0, words, bucket, cv,
                     max_batches_per_epoch=2, legibility_every=every)
            res[every] = ((out / "gen" / "batch_summary.txt").read_bytes(), (out / "gen" / "epoch_summary.txt").read_bytes(),
                          [m.store.flat.clone() for m in models], [m.store.state.clone() for m in models], random.random(), torch.rand(1).item(),
                          G.nl_gen.get_state().clone())
        # read_back on the same networks: G writes, R reads, in the order the words were given (two word lengths, one style reused)
        state = G.nl_gen.get_state().clone()
        with legibility.preserved_rng(G, R):
            rb = legibility.read_back(G, R, np.stack(my_imgs[:2], 0), ["ab", "c", "de"], cv)
        assert torch.equal(G.nl_gen.get_state(), state)
        assert [r["target"] for r in rb] == ["ab", "c", "de"]
        for r in rb:
            assert set(r["read"]) <= set(cv) and r["distance"] == LR.edit_distance_ref(r["read"], r["target"])
    finally:
        NA.configure(deterministic=False)
    rows = (tmp_path / "every1" / "model" / "legibility.csv").read_text().strip().split("\n")
    assert rows[0] + "\n" == legibility.LEGIBILITY_HEADER and len(rows) == 2
    cols = rows[1].split(",")
    assert len(cols) == 6 and int(cols[0]) == 1 and int(cols[1]) == bs and all(np.isfinite(float(c)) for c in cols)
    assert not (tmp_path / "every0" / "model" / "legibility.csv").exists()
    a, b = res[1], res[0]
    assert len(a[0].strip().split(b"\n")) == 3
    assert a[0] == b[0] and a[1] == b[1], "summaries differ between legibility_every = 1 and 0"
    for wa, wb in zip(a[2] + a[3], b[2] + b[3]):
        assert torch.equal(wa, wb)
    assert a[4] == b[4], "the hook consumed draws of the `random` stream"
    assert a[5] == b[5] and torch.equal(a[6], b[6]), "the hook consumed draws of a torch generator training uses"
