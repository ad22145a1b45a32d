"""The spatial transformers' localisation nets on torch's library and on the fused kernels of csrc/ftx_stn_loc.hip, re-measured in ONE
run by part 2 of profiles/stn_kernels.txt: HIP events around 10 calls after 3 warm-up calls, through the Python wrappers (autograd and
the host's enqueue included), b = 2.  Also the wall clock of each path's first use (its first forward and its first forward + backward
in this process).  One run, no repeat: no spread is claimed.

    python tools/bench_stn_loc.py [--out profiles/stn_loc_kernels.txt] [--skip-library]

Floors: the arithmetic of the two convolutions (forward: 2 flop per tap and conv output; forward + backward: three times that where
the input needs a gradient, twice otherwise) at 157.3 TFLOP/s, the fp32 vector / matrix peak of one MI355X."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK = 157.3e12


def conv_flop(b, c, ih, iw):
    """Forward flop of Conv2d(c, 8, 7) then Conv2d(8, 90, 5) behind a 2 x 2 pool, on a (b, c, ih, iw) input."""
    oh, ow = ih - 6, iw - 6
    ph, pw = oh // 2, ow // 2
    return 2.0 * b * (8 * c * 49 * oh * ow + 90 * 8 * 25 * (ph - 4) * (pw - 4))


def timed(fn, calls=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stn_loc_kernels.txt"))
    ap.add_argument("--skip-library", action="store_true", help="measure the fused path only (the library rows read 'not measured')")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stn_loc: needs a GPU (there is no fallback)")
    from fusiontransformer_amd.models.transformers import SpatialTransformer
    torch.manual_seed(0)
    up, down = SpatialTransformer(96).cuda(), SpatialTransformer(3).cuda()
    with torch.no_grad():
        for st in (up, down):
            st.fc_loc[2].weight.normal_(0, 0.02)
    x_up = torch.randn((2, 96, 384, 384), device="cuda")
    x_down = torch.randn((2, 3, 370, 1226), device="cuda")
    g = torch.randn((2, 2, 3), device="cuda")

    def fwd(mod, x):
        with torch.no_grad():
            return mod.theta(x)

    def fwd_bwd(mod, x, need_x):
        xx = x.detach().requires_grad_(need_x)
        (mod.theta(xx) * g).sum().backward()
        mod.zero_grad(set_to_none=True)

    lines = ["The localisation nets of the spatial transformers on one %s, fp32, b = 2: torch's library beside the fused kernels of" % torch.cuda.get_device_name(0),
             "csrc/ftx_stn_loc.hip (SpatialTransformer.set_loc_impl), measured in one process by tools/bench_stn_loc.py.  HIP events around 10",
             "calls after 3 warm-up calls through the Python wrappers; first use = wall clock of the path's first call in this process, device",
             "synchronised.  Floor = the convolutions' arithmetic at 157.3 TFLOP/s.  One run, no repeat: no spread is claimed.", ""]
    rows = {}
    impls = ["ftx"] if args.skip_library else ["library", "ftx"]
    for impl in impls:
        up.set_loc_impl(impl)
        down.set_loc_impl(impl)
        first = [wall(lambda: fwd(down, x_down)), wall(lambda: fwd(up, x_up)), wall(lambda: fwd_bwd(up, x_up, True)), wall(lambda: fwd_bwd(down, x_down, False))]
        lines.append("%-8s first use: stn_down.theta forward %.3f s, up_stn.theta forward %.3f s, up_stn.theta forward+backward %.3f s, "
                     "stn_down.theta forward+backward %.3f s" % ((impl,) + tuple(first)))
        rows[impl] = [timed(lambda: fwd(up, x_up)), timed(lambda: fwd_bwd(up, x_up, True)), timed(lambda: fwd(down, x_down)),
                      timed(lambda: fwd_bwd(down, x_down, False))]
    if args.skip_library:
        lines.append("library  not measured")
    lines.append("")
    f_up, f_down = conv_flop(2, 96, 384, 384), conv_flop(2, 3, 370, 1226)
    names = [("up_stn.theta forward (2x96x384x384)", f_up), ("up_stn.theta forward+backward", 3 * f_up),
             ("stn_down.theta forward (2x3x370x1226)", f_down), ("stn_down.theta forward+backward (the image takes no gradient)", 2 * f_down)]
    for i, (name, flop) in enumerate(names):
        lib = "%.1f us" % rows["library"][i] if "library" in rows else "not measured"
        ratio = "  library / ftx = %.2f" % (rows["library"][i] / rows["ftx"][i]) if "library" in rows else ""
        lines.append("%s: library %s, ftx %.1f us, floor %.1f us%s" % (name, lib, rows["ftx"][i], flop / PEAK * 1e6, ratio))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
