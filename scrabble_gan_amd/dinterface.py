"""The one-time dataset conversion of the reference (src/dinterface/dinterface.py:4-20 and
src/dinterface/iam_handwriting_db.py:6-93): IAM word crops + words.txt -> bucket folders `<out>/<len>/<id>.png` + `<id>.txt`, every word
resized to (h, (h // 2) * len).

PNG decode / encode stay on the host (PIL, a thread pool); the resize is sg_resample_u8 on the GPU, one launch per chunk of at most
CHUNK_BYTES source bytes, so a corpus never has to fit anywhere at once.  cv2.resize's default filter is INTER_LINEAR, which OpenCV
replaces by INTER_AREA when both scale factors are exactly 2; the converter makes the same choice per image (resample_mode).
Differences from the reference, on purpose: the transcription file is `<input_dir>/../gt/words.txt` built with os.path (the
reference spells it with Windows separators, iam_handwriting_db.py:37); a PNG without a transcription or one that cannot be
decoded is reported and skipped (the reference's bare `except` around the resize has the same effect for unreadable files)."""
from __future__ import annotations

import os
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

import numpy as np

CHUNK_BYTES = 256 << 20
MAX_WORKERS = 16


def worker_count() -> int:
    """Threads for PNG decode / encode: OMP_NUM_THREADS when set, never the machine's CPU count; at most MAX_WORKERS."""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", ""))
    except ValueError:
        n = 8
    return max(1, min(MAX_WORKERS, n))


def default_transcription_file(input_dir: str) -> str:
    """<input_dir>/../gt/words.txt (the reference: input_dir.rstrip('img\\\\') + '\\\\gt\\\\words.txt')."""
    return os.path.join(os.path.dirname(os.path.normpath(input_dir)), "gt", "words.txt")


def parse_words_txt(path: str) -> dict:
    """{'<id>.png': transcription}: '#' lines skipped, id = token 0, a segmentation flag (token 1) other than 'ok' gives '-1',
    the transcription is the LAST whitespace token (iam_handwriting_db.py:40-51)."""
    transcriptions = {}
    with open(path, "r", encoding="utf8") as fi:
        for line in fi:
            if line.startswith("#"):
                continue
            labels = line.split()
            if len(labels) < 2:
                continue
            transcriptions[labels[0] + ".png"] = labels[-1].strip() if labels[1] == "ok" else "-1"
    return transcriptions


def keep_word(transcription: str, bucket_size: int) -> bool:
    """a-zA-Z only (str.isalpha, as the reference), 1 .. bucket_size characters (iam_handwriting_db.py:66,80)."""
    return transcription.isalpha() and 1 <= len(transcription) <= bucket_size


def list_pngs(input_dir: str):
    files = []
    for dirpath, _, filenames in os.walk(input_dir):
        files += [os.path.join(dirpath, f) for f in filenames if f.endswith(".png")]
    return sorted(files, key=lambda p: (os.path.basename(p), p))


def conversion_plan(files, transcriptions: dict, target_size, bucket_size: int):
    """-> (plan, missing): plan = [(path, id, word, bucket, (h, (h // 2) * len))] for every kept word, sorted by id;
    missing = the PNGs that have no transcription."""
    h = int(target_size[0])
    plan, missing = [], []
    for path in files:
        name = os.path.basename(path)
        word = transcriptions.get(name)
        if word is None:
            missing.append(path)
        elif keep_word(word, bucket_size):
            plan.append((path, os.path.splitext(name)[0], word, len(word), (h, (h // 2) * len(word))))
    plan.sort(key=lambda e: e[1])
    return plan, missing


def resample_mode(sh: int, sw: int, dh: int, dw: int) -> int:
    """cv2.resize's default: INTER_LINEAR, replaced by INTER_AREA when both scale factors are exactly 2."""
    from . import ops
    return ops.RESAMPLE_AREA if (sh == 2 * dh and sw == 2 * dw) else ops.RESAMPLE_LINEAR


def read_gray(path: str):
    """uint8 [h, w], or None (reported) when the file cannot be decoded."""
    from PIL import Image
    try:
        with Image.open(path) as im:
            a = np.asarray(im.convert("L"))
        if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError("empty image")
        return np.ascontiguousarray(a, dtype=np.uint8)
    except Exception:  # noqa: BLE001  (the reference's bare except, iam_handwriting_db.py:88)
        print("error at: {}".format(path))
        return None


def decode_all(paths, pool=None):
    if pool is not None:
        return list(pool.map(read_gray, paths))
    with ThreadPoolExecutor(max_workers=worker_count()) as ex:
        return list(ex.map(read_gray, paths))


def resize_on_device(images, sizes, device=None):
    """[uint8 [sh, sw]] , [(dh, dw)] -> [uint8 [dh, dw]]: one launch per filter the chunk needs (LINEAR, and AREA for exact halvings)."""
    import torch
    from . import ops
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    outs = [None] * len(images)
    modes = [resample_mode(im.shape[0], im.shape[1], dh, dw) for im, (dh, dw) in zip(images, sizes)]
    for mode in sorted(set(modes)):
        idx = [k for k, m in enumerate(modes) if m == mode]
        buf, offsets, strides = ops.pack_gray_images([images[k] for k in idx])
        dst, at = [], 0
        for k in idx:
            dst.append(at)
            at += (sizes[k][0] * sizes[k][1] + 3) & ~3
        desc = ops.resample_desc(offsets, strides, [images[k].shape for k in idx], dst, [sizes[k][0] for k in idx],
                                 [sizes[k][1] for k in idx], [sizes[k][1] for k in idx])
        flat = ops.resample_u8(buf.to(device, non_blocking=True), desc, mode, ops.RESAMPLE_OUT_U8).cpu().numpy()
        for k, off in zip(idx, dst):
            dh, dw = sizes[k]
            outs[k] = flat[off:off + dh * dw].reshape(dh, dw).copy()
    return outs


def _write_sample(args):
    from PIL import Image
    out_dir, name, word, pixels = args
    Image.fromarray(pixels, mode="L").save(os.path.join(out_dir, name + ".png"))
    with open(os.path.join(out_dir, name + ".txt"), "w", encoding="utf8") as fo:
        fo.write(word)


def convert_to_gan_reading_format_save(input_dir, output_dir, target_size, bucket_size, transcriptions=None):
    """Convert an IAM-layout word folder to the bucketed reading format (iam_handwriting_db.py:6-93).  transcriptions: the words.txt
    to use (default: <input_dir>/../gt/words.txt)."""
    for i in range(bucket_size):
        os.makedirs(os.path.join(output_dir, str(i + 1)), exist_ok=True)
    words = parse_words_txt(transcriptions or default_transcription_file(input_dir))
    print("size of iamDB words: {}".format(len(words)))
    plan, missing = conversion_plan(list_pngs(input_dir), words, target_size, bucket_size)
    for path in missing:
        print("error at: {} (no transcription)".format(path))

    valid_samples, transcription_lengths = 0, []
    with ThreadPoolExecutor(max_workers=worker_count()) as pool:
        start = 0
        while start < len(plan):
            chunk, images, nbytes = [], [], 0
            # decode in slices of a few hundred files until the chunk's source bytes reach the bound
            while start < len(plan) and nbytes < CHUNK_BYTES:
                part = plan[start:start + 512]
                start += len(part)
                for entry, img in zip(part, decode_all([e[0] for e in part], pool)):
                    if img is not None:
                        chunk.append(entry)
                        images.append(img)
                        nbytes += img.shape[0] * ((img.shape[1] + 15) & ~15)
            if not chunk:
                continue
            resized = resize_on_device(images, [e[4] for e in chunk])
            list(pool.map(_write_sample, [(os.path.join(output_dir, str(e[3])), e[1], e[2], px) for e, px in zip(chunk, resized)]))
            valid_samples += len(chunk)
            transcription_lengths += [e[3] for e in chunk]
    print("size of valid iamDB words: {}".format(valid_samples))
    print(Counter(transcription_lengths))


def init_reading(train_input, train_output, target_size, bucket_size):
    """dinterface.py:4-20 of the reference: convert the IAM words under train_input to the GAN reading format in train_output."""
    convert_to_gan_reading_format_save(train_input, train_output, target_size, bucket_size)
