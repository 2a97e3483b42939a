"""The raw-corpus path end to end on a 12-word IAM-layout fixture: the converter (dinterface), RawWordCorpus batches against the
converted folder read through DevicePrefetcher, the device style-image fit, and main.py --raw-words."""
import os
import random

import numpy as np
import pytest
import torch

from tests import margins
from tests import resample_refs as RR

pytestmark = pytest.mark.gpu

CV = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'
H = 32
# id -> (status, transcription); the last four are not converted
# (every word length 1 .. 10 occurs: the train step draws its fake words from any bucket)
KEPT = {"a01-000-00-00": "a", "a01-000-00-01": "to", "a01-000-00-02": "Hi", "a01-000-00-03": "cat", "a01-000-00-04": "Move",
        "a01-000-00-05": "machine", "a01-000-01-00": "house", "a01-000-01-01": "letter", "a01-000-01-02": "Gaitskell",
        "a01-000-01-03": "handwritin", "a01-000-01-04": "learning", "a01-000-01-05": "I"}
DROPPED = {"a01-000-02-00": ("err", "bad"), "a01-000-02-01": ("ok", "Mr."), "a01-000-02-02": ("ok", "extraordinary")}
NO_PNG = "a01-000-02-03"


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """-> (raw_dir, {id: source pixels}): random-size grey PNGs between 20x30 and 90x400 under words/a01/a01-000/, gt/words.txt with an
    err line, a non-alphabetic word, an over-length word and an id whose PNG is missing; one crop is exactly twice its target size."""
    from PIL import Image
    root = tmp_path_factory.mktemp("iam")
    wdir = root / "words" / "a01" / "a01-000"
    wdir.mkdir(parents=True)
    (root / "gt").mkdir()
    rng = np.random.default_rng(7)
    pixels, lines = {}, ["#--- words.txt ---#", "# id ok/err graylevel x y w h tag transcription"]
    for k, (wid, word) in enumerate(list(KEPT.items()) + [(i, w) for i, (_, w) in DROPPED.items()]):
        hh, ww = int(rng.integers(20, 91)), int(rng.integers(30, 401))
        if wid == "a01-000-00-03":
            hh, ww = 2 * H, 2 * (H // 2) * 3                 # both scale factors exactly 2: the converter takes AREA
        px = rng.integers(0, 256, (hh, ww), dtype=np.uint8)
        Image.fromarray(px, mode="L").save(wdir / (wid + ".png"))
        pixels[wid] = px
        status = DROPPED[wid][0] if wid in DROPPED else "ok"
        lines.append("%s %s 154 %d 768 %d %d NN %s" % (wid, status, 400 + k, ww, hh, word))
    lines.append("%s ok 154 1 2 3 4 NN ghost" % NO_PNG)
    (root / "gt" / "words.txt").write_text("\n".join(lines) + "\n")
    return str(root / "words") + "/", pixels


@pytest.fixture(scope="module")
def converted(corpus, tmp_path_factory, dev):
    import contextlib
    import io
    from scrabble_gan_amd import dinterface as DI
    out = str(tmp_path_factory.mktemp("reading")) + "/"
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        DI.init_reading(corpus[0], out, (H, 160, 1), 10)
    return out, log.getvalue()


def u8_reference(px, word):
    from scrabble_gan_amd import dinterface as DI
    dh, dw = H, (H // 2) * len(word)
    mode = DI.resample_mode(px.shape[0], px.shape[1], dh, dw)
    return RR.resample_ref(px, dh, dw, mode), RR.exact_pixels(px.shape[0], px.shape[1], dh, dw, dw, mode), mode


def test_converter_writes_the_bucket_folders(corpus, converted):
    from PIL import Image
    from scrabble_gan_amd import data_io, ops
    out, log = converted
    want = sorted("%d/%s%s" % (len(w), i, ext) for i, w in KEPT.items() for ext in (".png", ".txt"))
    got = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
    assert got == want
    assert sorted(os.listdir(out)) == sorted(str(b) for b in range(1, 11))
    modes = set()
    for wid, word in KEPT.items():
        with Image.open(os.path.join(out, str(len(word)), wid + ".png")) as im:
            assert im.mode == "L" and im.size == (16 * len(word), H)
            px = np.asarray(im)
        ref, exact, mode = u8_reference(corpus[1][wid], word)
        modes.add(mode)
        RR.check_u8(px, ref, "converted %s" % wid, exact)
        assert open(os.path.join(out, str(len(word)), wid + ".txt")).read() == word
    assert modes == {ops.RESAMPLE_LINEAR, ops.RESAMPLE_AREA}
    lines = log.strip().split("\n")
    assert "size of iamDB words: 16" in lines and "size of valid iamDB words: 12" in lines
    from collections import Counter
    assert lines[-1] == str(Counter(len(KEPT[i]) for i in sorted(KEPT)))
    gen = data_io.load_prepare_data((H, 160, 1), 4, out, CV, 10)
    imgs, labels = next(gen)
    assert imgs.shape == (4, H, 16 * labels.shape[1], 1) and imgs.dtype == np.float32


def test_raw_corpus_batches_equal_the_converted_folder(corpus, converted, dev):
    from scrabble_gan_amd import data_io
    from scrabble_gan_amd.data_utils import bucket_words, encode_word
    out, _ = converted
    # the converted folder through the existing path: uint8 pixels -> DevicePrefetcher (sg_normalize_u8); keyed by (label, pixels' id)
    by_id = {}
    for wid, word in KEPT.items():
        from PIL import Image
        with Image.open(os.path.join(out, str(len(word)), wid + ".png")) as im:
            u8 = np.array(im).reshape(1, H, 16 * len(word), 1)
        fp = next(data_io.DevicePrefetcher(iter([(u8, np.zeros((1, len(word)), np.int32))]), dev, depth=1))[0]
        by_id[wid] = fp.cpu().numpy()[0]
    rc = data_io.RawWordCorpus(corpus[0], None, CV, 10, (H, 160, 1), dev, batch_size=6, quantize=True)
    assert sorted(rc.ids) == sorted(KEPT) and rc.ids == sorted(rc.ids)
    # the same seeds as load_prepare_data on the converted folder: the same bucket sequence (the sample indices mean different files:
    # the folder's listing order is not defined, so samples are matched by file id and label)
    gen = data_io.load_prepare_data((H, 160, 1), 6, out, CV, 10, raw=True)
    random.seed(5)
    np.random.seed(5)
    ref_batches = [next(gen) for _ in range(6)]
    random.seed(5)
    np.random.seed(5)
    raw_batches = []
    for _ in range(6):
        imgs, labels = next(rc)
        raw_batches.append((imgs, labels, list(rc.last_ids)))
    for imgs, labels, ids in raw_batches:
        assert imgs.is_cuda and imgs.dtype == torch.float32 and imgs.shape == (6, H, 16 * labels.shape[1], 1) and labels.dtype == np.int32
        got = imgs.cpu().numpy()
        for k, wid in enumerate(ids):
            assert list(labels[k]) == encode_word(KEPT[wid], CV)
            assert got[k].tobytes() == by_id[wid].tobytes(), wid              # bitwise: quantised resample == PNG + sg_normalize_u8
    # every converted sample, whatever was drawn: one batch per bucket built by hand
    for wid, word in KEPT.items():
        k = rc.ids.index(wid)
        rc.draw = lambda k=k, b=len(word): (b, [k] * 2)
        imgs, labels = next(rc)
        assert imgs[0].cpu().numpy().tobytes() == by_id[wid].tobytes(), wid
    del rc.draw
    # the loader on the converted folder: the same buckets in the same order, and its pixels are the ones compared above
    id_of = {tuple(encode_word(w, CV)): i for i, w in KEPT.items()}
    assert [lab.shape[1] for _, lab in ref_batches] == [lab.shape[1] for _, lab, _ in raw_batches]
    for u8, labels in ref_batches:
        fp = next(data_io.DevicePrefetcher(iter([(u8, labels)]), dev, depth=1))[0].cpu().numpy()
        for k, lab in enumerate(labels):
            assert fp[k].tobytes() == by_id[id_of[tuple(lab)]].tobytes()
    # random words from the corpus's own labels == bucket_words over the folder's transcriptions (sets per bucket)
    folder_words = [open(os.path.join(d, f)).read() for d, _, fs in os.walk(out) for f in fs if f.endswith(".txt")]
    want, got = bucket_words(folder_words, 10, CV), rc.random_words()
    for b in range(10):
        assert sorted(map(tuple, got[b])) == sorted(map(tuple, want[b]))

    # quantize=False: the unrounded resample, within the fp32 tolerance of the fp64 reference
    rf = data_io.RawWordCorpus(corpus[0], None, CV, 10, (H, 160, 1), dev, batch_size=2, quantize=False)
    for wid, word in KEPT.items():
        k = rf.ids.index(wid)
        rf.draw = lambda k=k, b=len(word): (b, [k] * 2)
        imgs, _ = next(rf)
        px = corpus[1][wid]
        ref, _, mode = u8_reference(px, word)
        tol = RR.f32_tolerance(RR.taps_per_output(mode, px.shape[0], px.shape[1], H, 16 * len(word)))
        err = float(np.abs(imgs[1, :, :, 0].cpu().numpy().astype(np.float64) - RR.normalise(ref)).max())
        margins.record("raw corpus %s" % wid, err, tol)
        assert err <= tol, (wid, err, tol)


STYLE_SHAPES = [(20, 70), (64, 400), (48, 90), (32, 100)]       # shorter than 32; wider than 160 after scaling; narrower; exactly 32 high


def _style_dir(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(21)
    sdir = tmp_path / "style"
    sdir.mkdir()
    pixels = {}
    for k, (hh, ww) in enumerate(STYLE_SHAPES):
        px = rng.integers(0, 256, (hh, ww), dtype=np.uint8)
        Image.fromarray(px, mode="L").save(sdir / ("s%d.png" % k))
        pixels["s%d.png" % k] = px
    return str(sdir), pixels


def _legacy_fit(img, h, w, validate):
    """The parent commit's _fit_style_image, copied verbatim as the yardstick of the default path."""
    from PIL import Image
    ht, wt = img.shape
    if validate:
        rate = min(h / ht, w / wt)
        dim = (int(wt * rate), h) if rate == h / ht else (w, int(ht * rate))
        resample = Image.BICUBIC
    else:
        rate = h / float(ht)
        dim = (int(wt * rate), h)
        resample = Image.BOX
    img = np.asarray(Image.fromarray(img.astype('float32'), mode="F").resize(dim, resample))
    width = img.shape[-1]
    if width > w:
        final = img[:, :w]
    elif width < w:
        final = np.ones([img.shape[0], w]) * 255
        final[:, :width] = img
    else:
        final = img
    return (final - 127.5) / 127.5


def test_style_images_on_the_device(dev, tmp_path):
    from scrabble_gan_amd import data_io
    sdir, pixels = _style_dir(tmp_path)
    # default call: today's code, byte for byte (the parent's function on the same files in the same shuffled order)
    random.seed(9)
    tr, va = data_io.load_style_input((32, 160, 1), 4, 10, sdir)
    random.seed(9)
    files = os.listdir(sdir)
    random.shuffle(files)
    assert len(tr) == 3 and len(va) == 1
    for got, f in zip(tr, files[:3]):
        want = _legacy_fit(pixels[f], 32, 160, False)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    want = _legacy_fit(pixels[files[3]], 32, 160, True)
    assert va[0].dtype == want.dtype and va[0].tobytes() == want.tobytes()

    # device path: all four crops through both filters, against the fp64 reference
    for validate, mode in ((False, RR.AREA), (True, RR.CUBIC)):
        imgs = [pixels[f] for f in sorted(pixels)]
        got = data_io._fit_style_images_device(imgs, 32, 160, validate, dev)
        for px, g in zip(imgs, got):
            dh, dw = data_io.style_fit_dims(px.shape[0], px.shape[1], 32, 160, validate)
            assert g.shape == (dh, 160) and g.dtype == np.float32
            ref = RR.canvas_ref(px, dh, dw, 160, mode, fill=255)
            tol = RR.f32_tolerance(RR.taps_per_output(mode, px.shape[0], px.shape[1], dh, dw))
            err = float(np.abs(g.astype(np.float64) - RR.normalise(ref)).max())
            margins.record("style %dx%d validate=%s" % (px.shape + (validate,)), err, tol)
            assert err <= tol
            if dw < 160:
                assert (g[:, dw:] == 1.0).all()
    random.seed(9)
    tr_d, va_d = data_io.load_style_input((32, 160, 1), 4, 10, sdir, resample="device")
    assert len(tr_d) == 3 and len(va_d) == 1 and all(t.shape == (32, 160) for t in tr_d)
    for got, f in zip(tr_d, files[:3]):
        px = pixels[f]
        dh, dw = data_io.style_fit_dims(px.shape[0], px.shape[1], 32, 160, False)
        assert np.abs(got.astype(np.float64) - RR.normalise(RR.canvas_ref(px, dh, dw, 160, RR.AREA))).max() <= RR.f32_tolerance(
            RR.taps_per_output(RR.AREA, px.shape[0], px.shape[1], dh, dw))
    with pytest.raises(ValueError):
        data_io.load_style_input((32, 160, 1), 4, 10, sdir, resample="opencv")


def test_main_raw_words_runs_to_the_end(corpus, dev, tmp_path):
    from scrabble_gan_amd import gin_config as gin, main as M
    sdir, _ = _style_dir(tmp_path)
    cfg = tmp_path / "cfg.gin"
    base = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs", "scrabble_gan_mi355x.gin")).read()
    cfg.write_text(base + "\nio.base_path = '%s/'\nshared_specs.batch_size = 4\nshared_specs.num_gen = 4\n" % tmp_path)
    gin.clear_config()
    with pytest.raises(SystemExit):
        M.main(["--gin", str(cfg), "--synthetic", "--raw-words", corpus[0]])
    gin.clear_config()
    M.main(["--gin", str(cfg), "--raw-words", corpus[0], "--style-dir", sdir, "--steps", "2", "--epochs", "1", "--batch-size", "4"])
    out = tmp_path / "run" / "output"
    rows = (out / "batch_summary.txt").read_text().strip().split("\n")
    assert rows[0].startswith("disc_loss;disc_loss_real") and len(rows) == 3
    for r in rows[1:]:
        cols = r.split(";")
        assert len(cols) == 16 and all(np.isfinite(float(c)) for c in cols)
    assert len((out / "epoch_summary.txt").read_text().strip().split("\n")) == 2
    for net in ("generator", "recognizer"):
        assert (tmp_path / "run" / "checkpoints" / net / "1" / "cktp-1.safetensors").exists()
    gin.clear_config()
    # the bucket-folder path names the converter and --raw-words when the folder is missing
    with pytest.raises(FileNotFoundError, match="prepare_data.*--raw-words"):
        M.main(["--gin", str(cfg), "--steps", "1", "--epochs", "1"])
    gin.clear_config()
