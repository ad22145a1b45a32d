"""Per-frame cost of the device colour jitter + conversion (functional.color_jitter_to_chw, csrc/ftx_image.hip) against Pillow's CPU
chain for the same draws.  Frames: a full 370x1226 KITTI frame and a 302x480 bottom-crop view of it (row pitch 3 * 1226); 0, 3 and 4
ops.  Prints one line per case: median HIP-event time per frame, kernel launches per frame (torch profiler), Pillow's median time.

    python tools/bench_image_aug.py [--iters 200]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fusiontransformer_amd import functional as spf  # noqa: E402

CHAINS = {
    0: [],
    3: [("saturation", 0.83), ("contrast", 1.21), ("brightness", 0.92)],
    4: [("hue", 0.04), ("brightness", 1.17), ("contrast", 0.71), ("saturation", 1.33)],
}
NORM = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])


def pil_chain(img_u8, draws):
    from PIL import Image, ImageEnhance
    img = Image.fromarray(np.ascontiguousarray(img_u8))
    for op, f in draws:
        if op == "brightness":
            img = ImageEnhance.Brightness(img).enhance(f)
        elif op == "contrast":
            img = ImageEnhance.Contrast(img).enhance(f)
        elif op == "saturation":
            img = ImageEnhance.Color(img).enhance(f)
        else:
            h, s, v = img.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            np_h += np.uint8(int(f * 255) % 256)
            img = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    x = np.array(img, dtype=np.float32) / 255.
    x = np.ascontiguousarray(np.fliplr(x))
    x = (x - np.asarray(NORM[0], np.float32)) / np.asarray(NORM[1], np.float32)
    return np.moveaxis(x, -1, 0)


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if "jitter_pass_kernel" in e.name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    full = rng.integers(0, 256, (370, 1226, 3), dtype=np.uint8)
    dev = torch.from_numpy(full).cuda()
    frames = {"370x1226": (dev, full), "302x480 crop view": (dev[68:370, 373:853], full[68:370, 373:853])}
    print(f"device: {torch.cuda.get_device_name(0)}; iters {args.iters}; median per frame")
    for fname, (src, host) in frames.items():
        for k, draws in CHAINS.items():
            run = lambda: spf.color_jitter_to_chw(src, draws, True, NORM)  # noqa: E731
            for _ in range(10):
                run()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.iters):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                run()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b) * 1e3)
            n_launch = launches(run)
            pil = []
            for _ in range(max(3, args.iters // 20)):
                t0 = time.perf_counter()
                pil_chain(host, draws)
                pil.append((time.perf_counter() - t0) * 1e6)
            print(f"{fname:18s} ops={k}  device {statistics.median(times):8.1f} us  launches {n_launch}  "
                  f"Pillow+numpy CPU {statistics.median(pil):9.1f} us")


if __name__ == "__main__":
    main()
