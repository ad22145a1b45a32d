"""Micro-benchmark of the fused attention kernels at the ViT's shape (578 tokens, 12 heads) over the built tilings.
usage (GPU box): python tools/bench_attn.py [--batches 1,2,4,8] [--iters 50]
--bf16: the fp32 kernels and the bf16-operand kernels (ftx_attn_fwd_bf16 / ftx_attn_bwd_bf16) from the same process, each point timed
--repeats times (median and min-max spread printed), with max |bf16 - fp32| of out and grad_qkv at the same tiling.
--split: the same comparison for the fp32-accurate kernels on the bf16 MFMA (ftx_attn_fwd_split / ftx_attn_bwd_split), at every tiling
the split family builds (ftx_attn_split_tiling_built; a direction it does not build at a tiling is left out, "-")."""
import argparse, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fusiontransformer_amd import functional as spf

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,2,4,8")
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--tokens", type=int, default=578)
ap.add_argument("--heads", type=int, default=12)
ap.add_argument("--bf16", action="store_true", help="compare the fp32 and the bf16-operand kernels")
ap.add_argument("--split", action="store_true", help="compare the fp32 and the split (three bf16 pieces) kernels")
ap.add_argument("--repeats", type=int, default=5, help="--bf16 / --split: timed repeats per point")
args = ap.parse_args()
L = spf._lib.load()
T, H = args.tokens, args.heads
CFGS = [(0, 0), (4, 2), (2, 2), (2, 4), (1, 2), (1, 4), (1, 8)]


def timeit(fn):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3




def bench_pair(other):
    """The fp32 kernels and the `other` family ("bf16" or "split") side by side, one process, one run."""
    import statistics
    entries = {"fp32": (L.ftx_attn_fwd_tiled, L.ftx_attn_bwd_tiled), "bf16": (L.ftx_attn_fwd_bf16, L.ftx_attn_bwd_bf16),
               "split": (L.ftx_attn_fwd_split, L.ftx_attn_bwd_split)}
    # (forward, backward) built for `other` at an explicit tiling; the fp32 kernels are timed where `other` is
    built = lambda qw, sp: tuple(other != "split" or qw == 0 or bool(L.ftx_attn_split_tiling_built(qw, sp, d)) for d in (0, 1))
    cell = lambda t, flop: "%9s %11s %9s" % ("-", "-", "-") if not t else "%9.1f %5.1f-%5.1f %9.1f" % (
        statistics.median(t), min(t), max(t), flop / statistics.median(t) / 1e6)
    print("%5s %8s %5s | %9s %11s %9s | %9s %11s %9s | %9s | max |%s - fp32|: out, grad"
          % ("batch", "(qw,spl)", "prec", "fwd us", "spread", "TFLOP/s", "bwd us", "spread", "TFLOP/s", "f+b us", other))
    for B in [int(x) for x in args.batches.split(",")]:
        g = torch.Generator(device="cuda"); g.manual_seed(B)
        qkv = torch.randn(B, T, 3, H, 64, device="cuda", generator=g)
        go = torch.randn(B, T, H * 64, device="cuda", generator=g)
        ws_bytes = int(L.ftx_attn_bwd_workspace_bytes(B, T, H)); ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        flop_f = 4.0 * B * H * T * T * 64
        for qw, sp in CFGS:
            res = {}
            do_f, do_b = built(qw, sp)
            if not (do_f or do_b):
                continue
            for prec in ("fp32", other):
                fwd, bwd = entries[prec]
                out = torch.empty(B, T, H * 64, device="cuda"); lse = torch.empty(B, H, T, device="cuda"); gq = torch.empty_like(qkv)
                f = lambda: fwd(qkv.data_ptr(), B, T, H, 64, 0.125, out.data_ptr(), lse.data_ptr(), qw, sp, spf.stream())
                bw = lambda: bwd(qkv.data_ptr(), out.data_ptr(), go.data_ptr(), lse.data_ptr(), B, T, H, 64, 0.125, gq.data_ptr(), ws.data_ptr(), ws_bytes, qw, sp, spf.stream())
                if do_f:
                    tf = [timeit(f) for _ in range(args.repeats)]
                else:       # the backward needs out and lse: the automatic forward, untimed
                    tf = []
                    fwd(qkv.data_ptr(), B, T, H, 64, 0.125, out.data_ptr(), lse.data_ptr(), 0, 0, spf.stream())
                tb = [timeit(bw) for _ in range(args.repeats)] if do_b else []
                res[prec] = (out, gq)
                d = ""
                if prec != "fp32":
                    d = "%.2e" % (out - res["fp32"][0]).abs().max().item() if do_f else "-"
                    d += " %.2e" % (gq - res["fp32"][1]).abs().max().item() if do_b else " -"
                print("%5d %8s %5s | %s | %s | %9s | %s"
                      % (B, "auto" if qw == 0 else "(%d,%d)" % (qw, sp), prec, cell(tf, flop_f), cell(tb, 2.5 * flop_f),
                         "%.1f" % (statistics.median(tf) + statistics.median(tb)) if tf and tb else "-", d), flush=True)


if args.bf16 or args.split:
    bench_pair("split" if args.split else "bf16")
    sys.exit(0)

print("%5s %8s | %9s %9s | %9s %9s | max |d| vs (4,2): out, grad" % ("batch", "(qw,spl)", "fwd us", "TFLOP/s", "bwd us", "TFLOP/s"))
for B in [int(x) for x in args.batches.split(",")]:
    g = torch.Generator(device="cuda"); g.manual_seed(B)
    qkv = torch.randn(B, T, 3, H, 64, device="cuda", generator=g)
    go = torch.randn(B, T, H * 64, device="cuda", generator=g)
    out = torch.empty(B, T, H * 64, device="cuda"); lse = torch.empty(B, H, T, device="cuda")
    gq = torch.empty_like(qkv)
    ws_bytes = int(L.ftx_attn_bwd_workspace_bytes(B, T, H)); ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    flop_f = 4.0 * B * H * T * T * 64
    ref = None
    for qw, sp in CFGS:
        f = lambda: L.ftx_attn_fwd_tiled(qkv.data_ptr(), B, T, H, 64, 0.125, out.data_ptr(), lse.data_ptr(), qw, sp, spf.stream())
        bw = lambda: L.ftx_attn_bwd_tiled(qkv.data_ptr(), out.data_ptr(), go.data_ptr(), lse.data_ptr(), B, T, H, 64, 0.125, gq.data_ptr(), ws.data_ptr(), ws_bytes, qw, sp, spf.stream())
        tf = timeit(f); tb = timeit(bw)
        if (qw, sp) == (4, 2):
            ref = (out.clone(), gq.clone())
        d = "" if ref is None else "%.2e %.2e" % ((out - ref[0]).abs().max().item(), (gq - ref[1]).abs().max().item())
        print("%5d %8s | %9.1f %9.1f | %9.1f %9.1f | %s" % (B, "auto" if qw == 0 else "(%d,%d)" % (qw, sp), tf, flop_f / tf / 1e6, tb, 2.5 * flop_f / tb / 1e6, d))
