"""Cost of the device image resize (functional.resize_bilinear_u8, csrc/ftx_resize.hip) for the NuScenes frame, 1600x900 -> 400x225,
one frame and a batch of four, against what it replaces: Pillow's `Image.resize(size, Image.BILINEAR)` on the host (one thread) plus the
upload of the result.  Per case: the device time of one call (HIP events around one warmed call, median), the time per call of a
back-to-back stream of calls (HIP events around the whole stream: what a loader that does not wait pays), kernel launches per call
(torch profiler), Pillow's median and best host time and the median time of the upload.  The outputs are compared first: equal bytes.

    python tools/bench_resize.py [--iters 200]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fusiontransformer_amd import functional as spf  # noqa: E402

SRC, SIZE = (1600, 900), (400, 225)


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if "resize_" in e.name and "kernel" in e.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    from PIL import Image
    import PIL
    rng = np.random.default_rng(0)
    host = rng.integers(0, 256, (4, SRC[1], SRC[0], 3), dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    print(f"device: {torch.cuda.get_device_name(0)}; Pillow {PIL.__version__}; torch threads {torch.get_num_threads()}; iters {args.iters}")
    print(f"{SRC[0]}x{SRC[1]} -> {SIZE[0]}x{SIZE[1]}, uint8 RGB")
    for n in (1, 4):
        src = dev[0] if n == 1 else dev
        run = lambda: spf.resize_bilinear_u8(src, SIZE)  # noqa: E731
        want = np.stack([np.asarray(Image.fromarray(host[i]).resize(SIZE, Image.BILINEAR)) for i in range(n)])
        got = run().cpu().numpy().reshape(want.shape)
        assert np.array_equal(got, want), "device output differs from Pillow"
        for _ in range(20):
            run()
        torch.cuda.synchronize()
        single = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            single.append(a.elapsed_time(b) * 1e3)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            run()
        b.record()
        b.synchronize()
        stream_us = a.elapsed_time(b) * 1e3 / args.iters
        n_launch = launches(run)
        pil, up = [], []
        for _ in range(max(20, args.iters // 10)):
            t0 = time.perf_counter()
            outs = [np.asarray(Image.fromarray(host[i]).resize(SIZE, Image.BILINEAR)) for i in range(n)]
            t1 = time.perf_counter()
            torch.from_numpy(np.stack(outs)).cuda()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            pil.append((t1 - t0) * 1e6)
            up.append((t2 - t1) * 1e6)
        print(f"frames={n}  device, one call {statistics.median(single):7.1f} us (min {min(single):.1f})  back-to-back {stream_us:7.1f} us/call  "
              f"launches {n_launch}  |  Pillow host {statistics.median(pil):9.1f} us (best {min(pil):.1f})  + upload {statistics.median(up):7.1f} us")


if __name__ == "__main__":
    main()
