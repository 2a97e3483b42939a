"""Host side of the raw-corpus path (no GPU): words.txt parsing, the conversion plan, the default transcription path, the source
packing / descriptor rules of sg_resample_u8 and the RNG call sequence of RawWordCorpus."""
import inspect
import random

import numpy as np
import pytest

CV = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'

WORDS_TXT = """#--- words.txt ---------------------------------------------------------------#
# format: a01-000u-00-00 ok 154 408 768 27 51 AT A
a01-000u-00-00 ok 154 408 768 27 51 AT A
a01-000u-00-01 ok 154 507 766 213 48 NN MOVE
a01-000u-00-02 err 154 796 764 70 50 TO to
a01-000u-00-03 ok 154 919 757 166 78 VB stop
a01-000u-00-04 ok 154 1185 754 126 61 NPT Mr.
a01-000u-00-05 ok 156 395 932 441 100 NP Gaitskell
a01-000u-00-06 ok 156 395 932 441 100 NP extraordinarily
a01-000u-01-00 ok 156 901 958 147 79 IN from two words
a01-000u-01-01 ok 156 901 958 147 79 IN
"""


@pytest.fixture()
def words_txt(tmp_path):
    p = tmp_path / "gt" / "words.txt"
    p.parent.mkdir()
    p.write_text(WORDS_TXT)
    return str(p)


def test_words_txt_parsing(words_txt):
    from scrabble_gan_amd import dinterface as DI
    t = DI.parse_words_txt(words_txt)
    assert len(t) == 9                                       # the two comment lines are skipped
    assert t["a01-000u-00-00.png"] == "A" and t["a01-000u-00-01.png"] == "MOVE"
    assert t["a01-000u-00-02.png"] == "-1"                   # not 'ok': marked, whatever its transcription
    assert t["a01-000u-01-00.png"] == "words"                # the LAST whitespace token
    assert t["a01-000u-00-04.png"] == "Mr."
    assert t["a01-000u-01-01.png"] == "IN"                   # (a line without a transcription column: its last token)
    keep = {k: DI.keep_word(v, 10) for k, v in t.items()}
    assert keep["a01-000u-00-00.png"] and keep["a01-000u-00-05.png"]
    assert not keep["a01-000u-00-02.png"]                    # '-1' is not alphabetic
    assert not keep["a01-000u-00-04.png"]                    # 'Mr.' is not alphabetic
    assert not keep["a01-000u-00-06.png"]                    # 15 characters > bucket_size
    assert not DI.keep_word("", 10) and DI.keep_word("abcdefghij", 10) and not DI.keep_word("abcdefghijk", 10)


def test_conversion_plan_pairs_ids_with_buckets_and_sizes(words_txt):
    from scrabble_gan_amd import dinterface as DI
    t = DI.parse_words_txt(words_txt)
    files = ["/x/words/a01/a01-000u/a01-000u-00-%02d.png" % k for k in (5, 0, 1, 2, 3, 4, 6)] + ["/x/words/a01/a01-000u/zz-unknown.png"]
    plan, missing = DI.conversion_plan(files, t, (32, 160, 1), 10)
    assert missing == ["/x/words/a01/a01-000u/zz-unknown.png"]
    assert [(e[1], e[2], e[3], e[4]) for e in plan] == [("a01-000u-00-00", "A", 1, (32, 16)), ("a01-000u-00-01", "MOVE", 4, (32, 64)),
                                                        ("a01-000u-00-03", "stop", 4, (32, 64)), ("a01-000u-00-05", "Gaitskell", 9, (32, 144))]
    assert DI.conversion_plan(files, t, (48, 160, 1), 10)[0][1][4] == (48, 96)
    # cv2.resize's default: LINEAR, AREA when both factors are exactly 2
    from scrabble_gan_amd import ops
    assert DI.resample_mode(64, 128, 32, 64) == ops.RESAMPLE_AREA
    assert DI.resample_mode(64, 127, 32, 64) == DI.resample_mode(65, 128, 32, 64) == DI.resample_mode(32, 64, 32, 64) == ops.RESAMPLE_LINEAR


def test_default_transcription_path():
    from scrabble_gan_amd import dinterface as DI
    assert DI.default_transcription_file("data/IAM_mygan/img/") == "data/IAM_mygan/gt/words.txt"
    assert DI.default_transcription_file("data/IAM_mygan/img") == "data/IAM_mygan/gt/words.txt"
    assert DI.default_transcription_file("/abs/corpus/words/") == "/abs/corpus/gt/words.txt"


def test_reference_api_surface_of_the_converter():
    from scrabble_gan_amd import dinterface as DI
    assert list(inspect.signature(DI.init_reading).parameters) == ["train_input", "train_output", "target_size", "bucket_size"]
    assert list(inspect.signature(DI.convert_to_gan_reading_format_save).parameters)[:4] == ["input_dir", "output_dir", "target_size", "bucket_size"]
    assert inspect.signature(DI.convert_to_gan_reading_format_save).parameters["transcriptions"].default is None


def test_worker_count_follows_omp_num_threads(monkeypatch):
    from scrabble_gan_amd import dinterface as DI
    monkeypatch.setenv("OMP_NUM_THREADS", "4")
    assert DI.worker_count() == 4
    monkeypatch.setenv("OMP_NUM_THREADS", "512")
    assert DI.worker_count() == 16
    monkeypatch.delenv("OMP_NUM_THREADS")
    assert 1 <= DI.worker_count() <= 16


def test_descriptor_packing_follows_the_alignment_rules():
    from scrabble_gan_amd import ops
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((1, 1), (20, 333), (7, 16), (31, 17))]
    buf, offsets, strides = ops.pack_gray_images(images, pin=False)
    assert buf.dtype.is_floating_point is False and buf.dim() == 1
    flat = buf.numpy()
    for im, off, st in zip(images, offsets, strides):
        h, w = im.shape
        assert off % 16 == 0 and st % 16 == 0 and w <= st < w + 16
        rows = flat[off:off + h * st].reshape(h, st)
        assert (rows[:, :w] == im).all() and (rows[:, w:] == 0).all()
    assert offsets[-1] + 31 * strides[-1] <= buf.numel()
    desc = ops.resample_desc(offsets, strides, [im.shape for im in images], [0, 5120, 10240, 15360], 32, [16, 160, 160, 160], 160)
    d, need = ops.check_resample_desc(desc, buf.numel(), None, ops.RESAMPLE_OUT_U8)
    assert d.shape == (4, 8) and d.dtype == np.int64 and need == 15360 + 32 * 160
    assert list(d[1]) == [offsets[1], 20, 333, 336, 5120, 32, 160, 160]

    def bad(col, val, row=1, **kw):
        b = desc.copy()
        b[row, col] = val
        with pytest.raises(ValueError):
            ops.check_resample_desc(b, kw.get("src_bytes", buf.numel()), kw.get("out_elems"), kw.get("kind", ops.RESAMPLE_OUT_U8))
    bad(0, offsets[1] + 8)          # misaligned source offset
    bad(3, 332)                     # stride < sw
    bad(3, 340)                     # stride not a multiple of 16
    bad(4, 256)                     # overlaps the first image's output region
    bad(4, 15362, row=3)            # uint8 output: dst_off not a multiple of 4
    bad(1, 0)
    bad(2, 32769)
    bad(5, 4097)
    bad(6, 0)
    bad(1, 32, row=3)               # one more source row than the buffer holds
    with pytest.raises(ValueError):
        ops.check_resample_desc(desc, buf.numel() - 1, None, ops.RESAMPLE_OUT_U8)
    with pytest.raises(ValueError):
        ops.check_resample_desc(desc, buf.numel(), need - 1, ops.RESAMPLE_OUT_U8)
    b = desc.copy()
    b[3, 4] = 15362                 # fp32 output counts elements: no multiple-of-4 rule
    ops.check_resample_desc(b, buf.numel(), None, ops.RESAMPLE_OUT_F32)


def test_raw_corpus_draws_like_load_prepare_data(tmp_path):
    """A stub corpus with no pixels: the index draw consumes `random` and `np.random` exactly as load_prepare_data does for the same
    bucket populations (one np.random.choice over the bucket weights, then batch_size random.randint calls)."""
    from PIL import Image
    from scrabble_gan_amd import data_io
    populations = [3, 0, 5, 2]
    names = {}
    for b, n in enumerate(populations, start=1):
        d = tmp_path / str(b)
        d.mkdir()
        for k in range(n):
            word = "".join(CV[(7 * b + 3 * k + j) % 52] for j in range(b))
            Image.fromarray(np.full((32, 16 * b), (16 * b + k) % 256, np.uint8), mode="L").save(d / ("w%d_%02d.png" % (b, k)))
            (d / ("w%d_%02d.txt" % (b, k))).write_text(word)
            names[(b, k)] = word
    plan = [("", "w%d_%02d" % (b, k), names[(b, k)], b, (32, 16 * b)) for b, n in enumerate(populations, start=1) for k in range(n)]
    stub = data_io.RawWordCorpus.__new__(data_io.RawWordCorpus)
    stub.batch_size, stub.bucket_size, stub.input_dim, stub.quantize = 6, 4, (32, 160, 1), True
    stub._setup(plan, [(32, 16 * e[3]) for e in plan], [0] * len(plan), [16 * e[3] for e in plan], CV)
    assert stub.populations == populations

    gen = data_io.load_prepare_data((32, 160, 1), 6, str(tmp_path) + "/", CV, 4, raw=True)
    random.seed(11)
    np.random.seed(12)
    ref_batches = [next(gen) for _ in range(8)]
    ref_state = (random.getstate(), np.random.get_state()[1].copy(), np.random.get_state()[2])
    random.seed(11)
    np.random.seed(12)
    drawn = [stub.draw() for _ in range(8)]
    assert random.getstate() == ref_state[0]
    assert (np.random.get_state()[1] == ref_state[1]).all() and np.random.get_state()[2] == ref_state[2]
    for (bucket, rows), (imgs, labels) in zip(drawn, ref_batches):
        assert labels.shape == (6, bucket)
        assert len(rows) == 6 and all(len(stub._labels[k]) == bucket for k in rows)       # (the folder's listing order is not defined)
    # same bucket sequence, and per-bucket word lists equal to bucket_words over the folder's transcriptions
    assert [b for b, _ in drawn] == [lab.shape[1] for _, lab in ref_batches]
    from scrabble_gan_amd.data_utils import bucket_words
    want = bucket_words(list(names.values()), 4, CV)
    got = stub.random_words()
    for b in range(4):
        assert sorted(map(tuple, got[b])) == sorted(map(tuple, want[b]))
