"""sg_wino_gemm per layer class at B = 128: the one-tile kernel (sg_debug_set_wino_persist(0, 0)) against the persistent tile loop (2, 0),
four alternating rounds of 10 launches each (HIP events).  python tools/probe_wino_persist.py > profiles/persist_probe_classes.txt"""
import math, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scrabble_gan_amd import ops
from scrabble_gan_amd._lib import call, lib
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(3)
L = lib()
for (B, H, W, K, N) in ((128, 16, 80, 512, 512), (128, 8, 40, 1024, 1024), (128, 16, 80, 64, 512), (128, 16, 160, 128, 128), (128, 8, 80, 256, 256),
                        (128, 8, 40, 512, 1024), (128, 4, 20, 1024, 1024), (128, 32, 160, 64, 128), (16, 16, 80, 512, 512), (16, 4, 20, 1024, 1024)):
    tile = 4
    T = B * (H // tile) * (W // tile); Tp = -(-T // 128) * 128
    V = torch.randn(36 * Tp * K, device=dev, generator=g); Mt = torch.empty(36 * Tp * N, device=dev)
    u = torch.randn(36 * N * K, device=dev, generator=g) / math.sqrt(K)
    s = ops._stream()
    res = {0: [], 2: []}
    for rep in range(4):
        for mode in (0, 2):
            L.sg_debug_set_wino_persist(mode, 0)
            for _ in range(2):
                call("sg_wino_gemm", V.data_ptr(), u.data_ptr(), Mt.data_ptr(), B, H, W, K, N, tile, s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                call("sg_wino_gemm", V.data_ptr(), u.data_ptr(), Mt.data_ptr(), B, H, W, K, N, tile, s)
            e1.record(); torch.cuda.synchronize()
            res[mode].append(e0.elapsed_time(e1) / 10)
    tiles = 36 * (Tp // 128) * (N // 128)
    fl = 2.0 * 36 * Tp * K * N / 1e9
    a, b = sorted(res[0])[1], sorted(res[2])[1]
    print("%4d x %2dx%3d %4d->%4d  tiles %6d  one-tile %7.3f ms %6.1f TF/s [%s]  persistent %7.3f ms %6.1f TF/s [%s]  ratio %.3f" % (
        B, H, W, K, N, tiles, a, fl / a, " ".join("%.3f" % v for v in res[0]), b, fl / b, " ".join("%.3f" % v for v in res[2]), b / a), flush=True)
    del V, Mt, u
