"""On-disk dataset readers of the reference's host pipeline ("next" tier):
load_prepare_data (/root/reference/src/bigacgan/data_utils.py:14-84) and load_style_input (:87-195), and RawWordCorpus, which
reads the unconverted IAM word crops and resamples every batch on the GPU (sg_resample_u8) instead of reading resized copies.

Bucket folders `<read_dir>/<L>/<name>.png` + `<name>.txt` (one transcription line) as written by the reference's
one-time converter; the style folder holds free-size handwriting crops that are height-normalised to 32, then
cropped / white-padded to 160.  PNGs are read with PIL (OpenCV is not installed); the `random` / `np.random`
call sequences are the reference's, so a seeded run draws the same batches.  Resampling differs from OpenCV's
INTER_AREA / INTER_CUBIC kernels by design limits of PIL (BOX / BICUBIC are the closest filters) -- this only
touches the free-size style images, never the bucketed training words, whose pixels are read unchanged;
load_style_input(resample="device") fits them with sg_resample_u8's AREA / CUBIC definitions instead."""
from __future__ import annotations

import os
import random

import numpy as np

from .data_utils import encode_word, normalize_images


def _read_gray(path: str) -> np.ndarray:
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("L"))


def load_prepare_data(input_dim, batch_size, reading_dir, char_vector, bucket_size, raw=False):
    """Python generator of (images float32 [B,h,16L,c] in [-1,1], labels int32 [B,L]); one bucket per batch, the
    bucket drawn with probability proportional to its population, samples drawn with replacement.
    raw=True (not in the reference) yields the uint8 pixels [B,h,16L,c] instead: DevicePrefetcher normalises on the GPU."""
    data_buckets, bucket_weights, number_samples = {}, {}, 0
    for i in range(1, bucket_size + 1):
        imgs, labels = [], []
        bucket_dir = reading_dir + str(i) + '/'
        for file in [f for f in os.listdir(bucket_dir) if f.endswith(".txt")]:
            with open(bucket_dir + file, 'r', encoding='utf8') as f:
                label = encode_word(f.readline(), char_vector)
            imgs.append(_read_gray(os.path.join(bucket_dir, os.path.splitext(file)[0] + '.png')))
            labels.append(label)
            number_samples += 1
        data_buckets[i] = (imgs, labels)
    for i in range(1, bucket_size + 1):
        bucket_weights[i] = len(data_buckets[i][1]) / number_samples
    while True:
        bucket = int(np.random.choice(bucket_size, 1, p=list(bucket_weights.values()))[0]) + 1
        image_batch, label_batch = [], []
        for _ in range(batch_size):
            k = random.randint(0, len(data_buckets[bucket][1]) - 1)
            image_batch.append(data_buckets[bucket][0][k])
            label_batch.append(data_buckets[bucket][1][k])
        if raw:
            h, _, c = input_dim
            yield (np.array(image_batch, dtype=np.uint8).reshape(-1, h, int((h / 2) * bucket), c), np.array(label_batch).astype(np.int32))
        else:
            yield normalize_images(np.array(image_batch), input_dim, bucket), np.array(label_batch).astype(np.int32)


def _fit_style_image(img: np.ndarray, h: int, w: int, validate: bool) -> np.ndarray:
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


def style_fit_dims(ht: int, wt: int, h: int, w: int, validate: bool):
    """(dh, dw) a style crop is resampled to before it is cropped / padded to width w: _fit_style_image's `dim`."""
    if validate:
        rate = min(h / ht, w / wt)
        dim = (int(wt * rate), h) if rate == h / ht else (w, int(ht * rate))
    else:
        rate = h / float(ht)
        dim = (int(wt * rate), h)
    return dim[1], dim[0]


def _fit_style_images_device(images, h: int, w: int, validate: bool, device=None):
    """_fit_style_image for a list of crops in ONE sg_resample_u8 launch: INTER_AREA's definition for the train split, INTER_CUBIC's
    for the validation split (data_utils.py:144,179 of the reference), unrounded fp32 output, white padding, crop at width w."""
    import torch
    from . import ops
    if not images:
        return []
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    dims = [style_fit_dims(im.shape[0], im.shape[1], h, w, validate) for im in images]
    buf, offsets, strides = ops.pack_gray_images(images)
    dst = np.concatenate([[0], np.cumsum([dh * w for dh, _ in dims])[:-1]]).astype(np.int64)
    desc = ops.resample_desc(offsets, strides, [im.shape for im in images], dst, [d[0] for d in dims], [d[1] for d in dims], w)
    flat = ops.resample_u8(buf.to(device, non_blocking=True), desc, ops.RESAMPLE_CUBIC if validate else ops.RESAMPLE_AREA,
                           ops.RESAMPLE_OUT_F32, fill=255).cpu().numpy()
    return [flat[o:o + dh * w].reshape(dh, w).copy() for o, (dh, _) in zip(dst, dims)]


def load_style_input(input_dim, batch_size, bucket_size, style_dir="../../scrabble-gan/data/Utku_40/", resample="pil"):
    """-> (train_imgs, validate_imgs): lists of [32,160] arrays in [-1,1]; 95/5 split after random.shuffle.
    resample="pil" (default): PIL's BOX / BICUBIC on the host; "device": one sg_resample_u8 launch per split."""
    if resample not in ("pil", "device"):
        raise ValueError("resample must be 'pil' or 'device', got %r" % (resample,))
    h, w, _ = input_dim
    files = os.listdir(style_dir)
    random.shuffle(files)
    split = int(len(files) * 0.95)
    if resample == "device":
        images = [_read_gray(os.path.join(style_dir, f)) for f in files]
        return _fit_style_images_device(images[:split], h, w, False), _fit_style_images_device(images[split:], h, w, True)
    train = [_fit_style_image(_read_gray(os.path.join(style_dir, f)), h, w, False) for f in files[:split]]
    validate = [_fit_style_image(_read_gray(os.path.join(style_dir, f)), h, w, True) for f in files[split:]]
    return train, validate


def draw_batch_indices(populations, batch_size):
    """The draws of one load_prepare_data batch for bucket populations [n_1 .. n_bucket_size]: one np.random.choice over the
    bucket weights, then batch_size random.randint calls.  -> (bucket, 1-based; [sample index in the bucket])."""
    number_samples = sum(populations)
    weights = [n / number_samples for n in populations]
    bucket = int(np.random.choice(len(populations), 1, p=weights)[0]) + 1
    return bucket, [random.randint(0, populations[bucket - 1] - 1) for _ in range(batch_size)]


class RawWordCorpus:
    """Training batches straight from the unconverted IAM word crops (`raw_dir`/**.png + words.txt): every kept word is decoded once,
    the source pixels are packed into ONE device buffer, and each next() resamples its batch to (h, h/2 * L) with one sg_resample_u8
    launch (a second one only if the batch holds a crop of exactly twice the target size, which takes AREA as in the converter).
    An iterator with load_prepare_data's contract and RNG call sequence (draw_batch_indices); inside a bucket the samples are
    ordered by file id.  Yields (images fp32 [B,h,16L,1] on the device, labels int32 numpy), what DevicePrefetcher yields.
    quantize=True: the pixels are rounded to uint8 first, bit-identical to converting the words (dinterface) and reading the PNGs
    through DevicePrefetcher; quantize=False: the unrounded resample."""

    def __init__(self, raw_dir, transcriptions, char_vector, bucket_size, input_dim, device, batch_size=16, quantize=True):
        import torch
        from . import dinterface as DI, ops
        self._torch, self._ops = torch, ops
        self._device = torch.device(device)
        self.batch_size, self.bucket_size, self.input_dim, self.quantize = batch_size, bucket_size, input_dim, quantize
        words = DI.parse_words_txt(transcriptions or DI.default_transcription_file(raw_dir))
        plan, missing = DI.conversion_plan(DI.list_pngs(raw_dir), words, input_dim, bucket_size)
        for path in missing:
            print("error at: {} (no transcription)".format(path))
        images = DI.decode_all([e[0] for e in plan])
        plan = [e for e, im in zip(plan, images) if im is not None]
        images = [im for im in images if im is not None]
        if not plan:
            raise ValueError("no usable word under %s" % raw_dir)
        buf, offsets, strides = ops.pack_gray_images(images)
        print("raw word corpus: %d words, %d source bytes on the device" % (len(plan), buf.numel()))
        if self._device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(self._device)
            if buf.numel() > free:
                raise MemoryError("the raw word corpus needs %d bytes of device memory, %d are free: convert it with "
                                  "`python -m scrabble_gan_amd.prepare_data` and train on the bucket folders instead" % (buf.numel(), free))
        self._src = buf.to(self._device)
        self._setup(plan, [im.shape for im in images], offsets, strides, char_vector)

    def _setup(self, plan, shapes, offsets, strides, char_vector):
        """plan: [(path, id, word, bucket, (h, w))] sorted by id; the per-sample descriptor columns and the per-bucket index lists."""
        from .data_utils import encode_word
        from . import dinterface as DI
        self.ids = [e[1] for e in plan]
        self._labels = [encode_word(e[2], char_vector) for e in plan]
        self._cols = np.array([[off, sh, sw, st] for off, (sh, sw), st in zip(offsets, shapes, strides)], np.int64).reshape(len(plan), 4)
        self._modes = np.array([DI.resample_mode(sh, sw, e[4][0], e[4][1]) for e, (sh, sw) in zip(plan, shapes)], np.int64)
        self.buckets = {b: [k for k, e in enumerate(plan) if e[3] == b] for b in range(1, self.bucket_size + 1)}
        self.populations = [len(self.buckets[b]) for b in range(1, self.bucket_size + 1)]
        self.last_ids = []

    def random_words(self):
        """Per-bucket encoded word lists (0-based bucket = len - 1) from the corpus's own labels: what data_utils.bucket_words gives
        for the transcriptions of the converted folder."""
        return [[self._labels[k] for k in self.buckets[b]] for b in range(1, self.bucket_size + 1)]

    def draw(self):
        """-> (bucket, sample numbers of the batch): load_prepare_data's draws."""
        bucket, ks = draw_batch_indices(self.populations, self.batch_size)
        return bucket, [self.buckets[bucket][k] for k in ks]

    def __iter__(self):
        return self

    def __next__(self):
        torch, ops = self._torch, self._ops
        bucket, rows = self.draw()
        self.last_ids = [self.ids[k] for k in rows]
        h, _, c = self.input_dim
        w = int((h / 2) * bucket)
        B = len(rows)
        desc = np.empty((B, 8), np.int64)
        desc[:, :4] = self._cols[rows]
        desc[:, 4] = np.arange(B, dtype=np.int64) * (h * w)
        desc[:, 5], desc[:, 6], desc[:, 7] = h, w, w
        out = torch.empty(B * h * w, device=self._device, dtype=torch.float32)
        kind = ops.RESAMPLE_OUT_F32_QUANT if self.quantize else ops.RESAMPLE_OUT_F32
        modes = self._modes[rows]
        for mode in np.unique(modes):
            ops.resample_u8(self._src, desc[modes == mode], int(mode), kind, out=out)
        return out.view(B, h, w, c), np.array([self._labels[k] for k in rows]).astype(np.int32)

    def close(self):
        pass


class DevicePrefetcher:
    """Host pipeline of SURVEY 8(f)-3 around a raw (uint8) batch generator.  The GENERATOR is pulled on the consumer's thread
    (at construction for the first `depth` batches, then one more per next()): it draws from the global `random` /
    `np.random` streams that train_step's fake-label draw and main.py's style split use too, so pulling it from a background
    thread would interleave the two consumers of those streams by timing -- a seeded run would not reproduce and
    data-parallel ranks would not see the same global batch.  Here the interleaving is a fixed function of the
    call sequence; the generator's own draw order is the reference loader's.  A background thread does the byte work only:
    it stages the pixels in PINNED host buffers (torch's caching host allocator); next() queues an asynchronous
    host-to-device copy of the bytes (a quarter of the fp32 volume) and the GPU-side pixel normalisation (sg_normalize_u8 =
    data_utils.py:82) on the current stream and returns (images fp32 on the device, labels int32 numpy): train_step takes
    device tensors as they are.  depth = batches staged ahead."""

    def __init__(self, raw_batches, device, depth: int = 2):
        import queue
        import threading
        import torch
        self._torch = torch
        self._device = torch.device(device)
        self._it = iter(raw_batches)
        self._in = queue.Queue()
        self._q = queue.Queue()
        self._exhausted = False

        def work():
            while True:
                item = self._in.get()
                if item is None:
                    self._q.put(None)
                    return
                try:
                    u8, labels = item
                    u8 = np.ascontiguousarray(u8, dtype=np.uint8)
                    n = u8.size
                    pad = (-n) % 16                                   # the kernel converts 16 pixels per thread
                    buf = torch.empty(n + pad, dtype=torch.uint8, pin_memory=self._device.type == "cuda")
                    buf[:n].copy_(torch.from_numpy(u8.reshape(-1)))
                    if pad:
                        buf[n:].zero_()
                    self._q.put((buf, u8.shape, labels))
                except Exception as e:  # noqa: BLE001  (surface staging errors in the consumer)
                    self._q.put(e)

        self._thread = threading.Thread(target=work, daemon=True)
        self._thread.start()
        for _ in range(max(1, depth)):
            self._feed()

    def _feed(self):
        """Pull ONE batch from the generator on the calling thread and hand it to the staging thread."""
        if self._exhausted:
            return
        try:
            self._in.put(next(self._it))
        except StopIteration:
            self._exhausted = True
            self._in.put(None)

    def __iter__(self):
        return self

    def __next__(self):
        from . import ops
        item = self._q.get()
        if item is None:
            self._q.put(None)
            raise StopIteration
        if isinstance(item, Exception):
            raise item
        self._feed()
        buf, shape, labels = item
        n = int(np.prod(shape))
        dev8 = buf.to(self._device, non_blocking=True)
        return ops.normalize_u8(dev8)[:n].view(*shape), labels

    def close(self):
        if not self._exhausted:
            self._exhausted = True
            self._in.put(None)
