"""Host side of the legibility feature, no GPU: text decoding, the numpy references the GPU tests are held to (on the hand
cases whose answers are known), the evaluation CLI's argument parsing, the CSV header and the new train() keyword."""
import inspect

import numpy as np
import pytest

from tests import legibility_refs as LR

CV = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'


def test_decode_text_round_trips_encode_word():
    from scrabble_gan_amd import data_utils as DU, legibility
    words = ["auto", "Zz", "a", "handwriting", ""]
    packed, lengths = legibility.pack_words(words, CV)
    assert packed.dtype == np.int32 and packed.shape == (5, 11) and lengths.tolist() == [4, 2, 1, 11, 0]
    assert packed[0, :4].tolist() == DU.encode_word("auto", CV) and (packed[0, 4:] == -1).all()
    assert legibility.decode_text(packed, lengths, CV) == words
    import torch
    assert legibility.decode_text(torch.from_numpy(packed), torch.from_numpy(lengths), CV) == words
    assert legibility.pack_words([[0, 20], [3]])[0].tolist() == [[0, 20], [3, -1]]
    with pytest.raises(ValueError):
        legibility.pack_words(["a-b"], CV)


def _frames(path, C, T=None):
    x = np.zeros((len(path), C), np.float32)
    x[np.arange(len(path)), path] = 5.0
    return x


def test_greedy_reference_on_the_hand_cases():
    C = 5
    blank = C - 1
    cases = [([blank] * 6, []), ([2] * 6, [2]), ([0, blank, 0, blank, blank, blank], [0, 0]), ([0, 0, 1, 1, blank, 1], [0, 1, 1]),
             ([0, 1, 2, 3, 0, 1], [0, 1, 2, 3, 0, 1])]
    logits = np.stack([_frames(p, C) for p, _ in cases], 0)
    logits[3, 2, :] = 0.0
    logits[3, 2, 3] = logits[3, 2, 1] = 2.0                   # exact tie: numpy.argmax takes the lowest index
    lab, ln, logp = LR.greedy_ref(logits)
    for b, (_, want) in enumerate(cases):
        assert lab[b, :ln[b]].tolist() == want and (lab[b, ln[b]:] == -1).all()
    lp = LR.log_probs_ref(logits)
    assert np.allclose(np.exp(lp).sum(-1), 1.0) and np.isclose(logp[1], lp[1, :, 2].sum())
    lab4, ln4, _ = LR.greedy_ref(logits, input_length=4)     # frames 4, 5 ignored
    assert lab4.shape == (5, 4) and lab4[3, :ln4[3]].tolist() == [0, 1] and lab4[4, :ln4[4]].tolist() == [0, 1, 2, 3]


def test_edit_distance_reference_on_the_hand_cases():
    assert LR.edit_distance_ref("", "") == 0
    assert LR.edit_distance_ref("", "abc") == 3 and LR.edit_distance_ref("abc", "") == 3
    assert LR.edit_distance_ref("handwriting", "handwriting") == 0
    assert LR.edit_distance_ref("kitten", "sitting") == 3
    assert LR.edit_distance_ref([1, 2, 3], [2, 3]) == 1


def test_lexicon_fixture_is_deduplicated_and_planted():
    logits, lexicon, planted = LR.lexicon_problem(0)
    assert logits.shape == (8, 19, 53) and len(lexicon) == 67 == len({tuple(w) for w in lexicon})
    assert {len(w) for w in lexicon} == {1, 2, 3, 4, 5} and [7, 7, 7, 2, 2] in LR.PLANTED_WORDS
    assert [lexicon[i] for i in planted] == LR.PLANTED_WORDS
    lab, ln, _ = LR.greedy_ref(logits)
    assert [lab[b, :ln[b]].tolist() for b in range(8)] == LR.PLANTED_WORDS


def test_evaluate_cli_arguments(tmp_path):
    from scrabble_gan_amd import evaluate
    a = evaluate.parse_args(["--recognizer-weights", "r/cktp-1", "--synthetic"])
    assert a.synthetic and a.data is None and not a.my_rec and a.lexicon is None and a.generator_weights is None
    a = evaluate.parse_args(["--recognizer-weights", "r/cktp-1", "--my-rec", "--data", "bkts", "--lexicon", "w.txt", "--generator-weights",
                             "g/cktp-1", "--words", "ab", "Hello"])
    assert a.my_rec and a.data == "bkts" and a.lexicon == "w.txt" and a.generator_weights == "g/cktp-1" and a.words == ["ab", "Hello"]
    for bad in (["--synthetic"], ["--recognizer-weights", "r"], ["--recognizer-weights", "r", "--synthetic", "--data", "d"],
                ["--recognizer-weights", "r", "--synthetic", "--batches", "0"]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(bad)
    f = tmp_path / "lex.txt"
    f.write_text("cat\n\n dog \ncat\nZebra\n")
    assert evaluate.read_lexicon(str(f), CV) == ["cat", "dog", "Zebra"]
    f.write_text("it's\n")
    with pytest.raises(ValueError):
        evaluate.read_lexicon(str(f), CV)


def test_run_inference_read_back_needs_recognizer_weights():
    from scrabble_gan_amd import run_inference
    with pytest.raises(SystemExit):
        run_inference.main(["--weights", "g", "--read-back"])


def test_csv_header_and_train_keyword():
    from scrabble_gan_amd import data_utils as DU, legibility
    assert legibility.LEGIBILITY_HEADER == "epoch,n,cer_real,wer_real,cer_fake,wer_fake\n"
    params = inspect.signature(DU.train).parameters
    assert list(params)[-1] == "legibility_every" and params["legibility_every"].default == 0
    assert hasattr(legibility, "evaluate_recognizer") and hasattr(legibility, "read_back")


def test_rates_from_the_sums():
    import torch
    from scrabble_gan_amd import legibility
    r = legibility._rates(torch.tensor([3.0, 12.0, 2.0, 4.0], dtype=torch.float64))
    assert r == {"cer": 0.25, "wer": 0.5, "n_words": 4, "n_chars": 12}
