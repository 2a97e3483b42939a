"""Cost of the raw-corpus path (HIP events / host clock around synchronised work).
    python tools/bench_resample.py [--batch 128] [--rounds 30] [--inner 10] [--steps 3] [--words 2000] [--out FILE]
(1) a synthetic corpus of `--batch` ten-letter words with 100 x 300 sources: time per batch of RawWordCorpus.__next__ beside
DevicePrefetcher.__next__ on the converted copy of the same words (the yardstick), alternating; the sg_resample_u8 launch alone
(device descriptors, `--inner` launches between two events) and its algorithmic bytes/s (sources read once + fp32 batch written once)
against the 8 TB/s HBM roof; (2) the c2 train step at that batch (fp32, word length 10) for the 1 % bound; (3) the converter's wall
time on `--words` synthetic words beside PIL's Image.resize (BILINEAR) on 16 threads over the same files (decode + resize + encode)."""
import argparse
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrabble_gan_amd import data_io, data_utils as DU, dinterface as DI, net_architecture as NA, net_loss, nn, ops, optimizers  # noqa: E402

CV = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ'


def make_corpus(root, n, rng, length=None, size=None):
    from PIL import Image
    wdir = os.path.join(root, "words", "a01", "a01-000")
    os.makedirs(wdir)
    os.makedirs(os.path.join(root, "gt"))
    lines = []
    for k in range(n):
        L = length or int(rng.integers(1, 11))
        hh, ww = size or (int(rng.integers(40, 160)), int(rng.integers(30 * L, 60 * L + 40)))
        word = "".join(CV[int(c)] for c in rng.integers(0, 52, L))
        Image.fromarray(rng.integers(0, 256, (hh, ww), dtype=np.uint8), mode="L").save(os.path.join(wdir, "w-%05d.png" % k))
        lines.append("w-%05d ok 154 1 2 %d %d NN %s" % (k, ww, hh, word))
    open(os.path.join(root, "gt", "words.txt"), "w").write("\n".join(lines) + "\n")
    return os.path.join(root, "words") + "/"


def quiet(fn, *a, **k):
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def batches(args, dev, lines, tmp):
    B = args.batch
    rng = np.random.default_rng(0)
    raw = make_corpus(os.path.join(tmp, "b"), B, rng, length=10, size=(100, 300))
    read = os.path.join(tmp, "b", "reading") + "/"
    quiet(DI.init_reading, raw, read, (32, 160, 1), 10)
    rc = quiet(data_io.RawWordCorpus, raw, None, CV, 10, (32, 160, 1), dev, batch_size=B)
    pf = data_io.DevicePrefetcher(data_io.load_prepare_data((32, 160, 1), B, read, CV, 10, raw=True), dev)

    def timed(it):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        next(it)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    for _ in range(5):
        timed(rc), timed(pf)
    t_rc, t_pf = [], []
    for _ in range(args.rounds):
        t_rc.append(timed(rc))
        t_pf.append(timed(pf))

    # the launch alone: the whole corpus as one batch, descriptors already on the device
    desc = np.empty((B, 8), np.int64)
    desc[:, :4] = rc._cols
    desc[:, 4] = np.arange(B) * 32 * 160
    desc[:, 5], desc[:, 6], desc[:, 7] = 32, 160, 160
    ddev = torch.from_numpy(desc).to(dev)
    out = torch.empty(B * 32 * 160, device=dev, dtype=torch.float32)
    from scrabble_gan_amd._lib import call

    def launch():
        call("sg_resample_u8", rc._src.data_ptr(), ddev.data_ptr(), B, ops.RESAMPLE_LINEAR, ops.RESAMPLE_OUT_F32_QUANT, out.data_ptr(), 255, ops._stream())
    for _ in range(3 * args.inner):
        launch()
    torch.cuda.synchronize()
    t_k = []
    for _ in range(args.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.inner):
            launch()
        e1.record()
        torch.cuda.synchronize()
        t_k.append(e0.elapsed_time(e1) / args.inner)
    nbytes = int(rc._src.numel()) + out.numel() * 4
    lines.append("batch %d, word length 10, sources 100 x 300 uint8 -> [%d, 32, 160, 1] fp32; %d alternating rounds (host clock around one synchronised next())"
                 % (B, B, args.rounds))
    lines.append("%-52s %10s %10s %10s" % ("per batch (ms)", "median", "min", "max"))
    for name, t in (("RawWordCorpus.__next__ (resample on the device)", t_rc), ("DevicePrefetcher.__next__ on the converted copy", t_pf),
                    ("sg_resample_u8 alone (events, %d launches)" % args.inner, t_k)):
        lines.append("%-52s %10.4f %10.4f %10.4f" % (name, statistics.median(t), min(t), max(t)))
    mk = statistics.median(t_k)
    lines.append("kernel: %.2f MB read + written per launch = %.1f GB/s = %.2f %% of the 8 TB/s HBM roof"
                 % (nbytes / 1e6, nbytes / (mk * 1e-3) / 1e9, 100.0 * nbytes / (mk * 1e-3) / 8e12))
    pf.close()
    return statistics.median(t_rc), statistics.median(t_pf)


def step_time(args, dev, lines):
    B, L = args.batch, 10
    nn.FAST_INIT = True                     # timing only: skip the QR initialisers
    try:
        G = NA.make_generator(128, (32, 160, 1), (32, 8192), None, "B3", 52, vis_model=False)
        D = NA.make_discriminator((32, 160, 1), None, "B1", vis_model=False)
        R = NA.make_recognizer((32, 160, 1), None, 53, vis_model=False)
        S = NA.make_style_promoter((32, 160, 1), None, "B1", vis_model=False)
    finally:
        nn.FAST_INIT = False
    gan = NA.make_gan(G, D, R, S, vis_model=False)
    images, labels, my_imgs = DU.synthetic_batch(B, L, seed=1)
    words = DU.synthetic_random_words(10, 200, seed=1)
    fake = np.array(words[L - 1][:B], np.int32)
    dv = [torch.from_numpy(t).to(dev) for t in (images, labels, my_imgs, fake)]
    opts = [optimizers.Adam(2e-4, 0.0, 0.999) for _ in range(4)]
    ts = []
    for k in range(2 + args.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        DU.train_step(0, 0, 1, dv[0], dv[1], D, R, S, gan, opts[0], opts[1], opts[2], opts[3], dv[2], B, 128, net_loss.hinge, 1, 1, words, 10, "",
                      fake_labels=dv[3], verbose=False, sync=False)
        torch.cuda.synchronize()
        if k >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    lines.append("c2 train step (fp32, batch %d, word length 10), %d steps after 2 warm-up steps: median %.2f ms (min %.2f, max %.2f)"
                 % (B, args.steps, statistics.median(ts), min(ts), max(ts)))
    return statistics.median(ts)


def converter(args, dev, lines, tmp):
    from PIL import Image
    rng = np.random.default_rng(1)
    raw = make_corpus(os.path.join(tmp, "c"), args.words, rng)
    t0 = time.perf_counter()
    quiet(DI.init_reading, raw, os.path.join(tmp, "c", "reading") + "/", (32, 160, 1), 10)
    torch.cuda.synchronize()
    t_dev = time.perf_counter() - t0
    plan, _ = DI.conversion_plan(DI.list_pngs(raw), DI.parse_words_txt(DI.default_transcription_file(raw)), (32, 160, 1), 10)
    out = os.path.join(tmp, "c", "pil")
    for b in range(1, 11):
        os.makedirs(os.path.join(out, str(b)))

    def one(e):
        with Image.open(e[0]) as im:
            im.convert("L").resize((e[4][1], e[4][0]), Image.BILINEAR).save(os.path.join(out, str(e[3]), e[1] + ".png"))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=16) as ex:
        list(ex.map(one, plan))
    t_pil = time.perf_counter() - t0
    lines.append("converter, %d synthetic words (%d threads for PNG decode / encode): %.2f s; PIL Image.resize on 16 threads over the same files: %.2f s"
                 % (len(plan), DI.worker_count(), t_dev, t_pil))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--words", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    NA.configure(device=dev, seed=0)
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        m_rc, m_pf = batches(args, dev, lines, tmp)
        lines.append("")
        m_step = step_time(args, dev, lines)
        bound = max(2.0 * m_pf, 0.01 * m_step)
        lines.append("acceptance: a raw-corpus batch (%.4f ms) <= max(2 x yardstick = %.4f ms, 1 %% of the step = %.4f ms) = %.4f ms: %s"
                     % (m_rc, 2.0 * m_pf, 0.01 * m_step, bound, "met" if m_rc <= bound else "NOT met"))
        lines.append("")
        converter(args, dev, lines, tmp)
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
