"""Times the bf16 ViT Linears (qkv, proj, fc1, fc2) per direction at batch 1, 4 and 8 (M = 578 x batch), in one process:

  (a) library  the library bf16 path as models/transformers._LinearFn runs it: casts of x, w and dy to bf16, the bf16 GEMM, the widening
               of its bf16 result to fp32, the bias add; fc1's forward adds nn.GELU, fc2's dX adds the GELU backward (fc1's dY)
  (b) mm_f32   torch.mm(bf16, bf16, out_dtype=torch.float32) on pre-cast operands (not timed: the casts), where this torch serves it
  (c) rows     the LiDAR branch's ftx_rows_gemm_bf16 (forward / dX) and dense ftx_spconv_pairs_wgrad_bf16 (dW)
  (d) dense    the new ftx_dense_gemm_bf16 (with its bias / GELU / DGELU epilogue) and ftx_dense_wgrad_bf16

Each result is checked against float64 on the bf16-rounded operands: paths (b)-(d) must meet the fp32-output bound
(chain * 2^-24 * sum |a b|); the library path must meet the same bound widened by its bf16 output rounding (2^-8 relative to the
result and to sum |a b|).  A result
that misses its bound is printed as WRONG and no time is reported for it.  roof = max(flops / 2.5 PF, bytes / 8 TB/s) with the fp32
operand and output bytes; "roof%" = roof / measured.

usage: python tools/bench_vit_linear.py [--batches 1 4 8] [--reps 50]"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fusiontransformer_amd import functional as spf  # noqa: E402

LINEARS = {"qkv": (768, 2304), "proj": (768, 768), "fc1": (768, 3072), "fc2": (3072, 768)}
U = 2.0 ** -24


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) * 1000.0 / reps)
    return sorted(best)[1]


def r64(t):
    return t.to(torch.bfloat16).double()


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / 2.0 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2.0 * torch.pi) ** 0.5


def ratio(out, ref, bound):
    return float(((out.double() - ref).abs() / bound.clamp_min(1e-300)).max())


def has_mm_out_dtype():
    a = torch.ones(64, 64, device="cuda", dtype=torch.bfloat16)
    try:
        return torch.mm(a, a, out_dtype=torch.float32).dtype == torch.float32
    except Exception:
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    mm_ok = has_mm_out_dtype()
    print(f"# torch {torch.__version__}, device {torch.cuda.get_device_name()}, mm(out_dtype=float32) on bf16: {'yes' if mm_ok else 'no'}")
    print(f"{'batch':>5} {'linear':>5} {'dir':>4} {'path':>8} {'us':>9} {'TFLOP/s':>8} {'roof%':>6} {'err/bound':>9}")
    totals = {}
    for batch in args.batches:
        m = 578 * batch
        for name, (k, n) in LINEARS.items():
            g = torch.Generator(device="cuda").manual_seed(batch * 100 + k + n)
            x = torch.randn(m, k, device="cuda", generator=g)
            w = torch.randn(n, k, device="cuda", generator=g) * 0.02
            b = torch.randn(n, device="cuda", generator=g) * 0.1
            dy = torch.randn(m, n, device="cuda", generator=g) * 0.1
            pre_fc1 = torch.randn(m, k, device="cuda", generator=g)   # fc2's input pre-activation (fc1's output), for the DGELU form
            x64, w64, dy64 = r64(x), r64(w), r64(dy)
            gelu_out = name == "fc1"
            dgelu_in = name == "fc2"

            # float64 references on the rounded operands and the fp32-output bounds
            s = x64 @ w64.t() + b.double()
            sb = (k + 2) * U * (x64.abs() @ w64.abs().t() + b.double().abs())
            if gelu_out:
                fref, fbound = gelu64(s), dgelu64(s).abs() * sb + 8 * U * (s.abs() + 1e-30)
            else:
                fref, fbound = s, sb
            d = dy64 @ w64
            db = (n + 2) * U * (dy64.abs() @ w64.abs())
            if dgelu_in:
                dg = dgelu64(pre_fc1.double())
                dref, dbound = d * dg, db * dg.abs() + 8 * U * d.abs() * (1 + pre_fc1.double().abs()) + 1e-30
            else:
                dref, dbound = d, db
            wref = dy64.t() @ x64
            wbound = (m + 72) * U * (dy64.abs().t() @ x64.abs())

            xb, wb, dyb = x.bfloat16(), w.bfloat16(), dy.bfloat16()
            wbt = wb.t().contiguous()

            def lib_fwd():
                y = (x.to(torch.bfloat16) @ w.to(torch.bfloat16).t()).float().add_(b)
                return F.gelu(y) if gelu_out else y

            def lib_dx():
                dx = (dy.to(torch.bfloat16) @ w.to(torch.bfloat16)).float()
                return torch.ops.aten.gelu_backward(dx, pre_fc1) if dgelu_in else dx

            def lib_dw():
                return (dy.to(torch.bfloat16).t() @ x.to(torch.bfloat16)).float()

            def mm_fwd():
                y = torch.mm(xb, wbt, out_dtype=torch.float32).add_(b)
                return F.gelu(y) if gelu_out else y

            def mm_dx():
                dx = torch.mm(dyb, wb, out_dtype=torch.float32)
                return torch.ops.aten.gelu_backward(dx, pre_fc1) if dgelu_in else dx

            def mm_dw():
                return torch.mm(dyb.t(), xb, out_dtype=torch.float32)

            def rows_fwd():
                y = spf._rows_gemm(x, w, 1, b, n, True)
                return F.gelu(y) if gelu_out else y

            def rows_dx():
                dx = spf._rows_gemm(dy, w, 0, None, k, True)
                return torch.ops.aten.gelu_backward(dx, pre_fc1) if dgelu_in else dx

            def rows_dw():
                return spf._rows_wgrad(dy, x, True)

            def dense_fwd():
                if gelu_out:
                    return spf._dense_gemm(x, w, 0, spf.EPI_BIAS_GELU, bias=b, with_pre=True)[0]
                return spf._dense_gemm(x, w, 0, spf.EPI_BIAS, bias=b)[0]

            def dense_dx():
                if dgelu_in:
                    return spf._dense_gemm(dy, w, 1, spf.EPI_DGELU, pre_in=pre_fc1)[0]
                return spf._dense_gemm(dy, w, 1, spf.EPI_NONE)[0]

            def dense_dw():
                return spf._dense_wgrad(dy, x)

            flops = 2.0 * m * n * k
            dirs = {
                "fwd": (fref, fbound, 4.0 * (m * k + n * k + m * n * (2 if gelu_out else 1)),
                        [("library", lib_fwd), ("mm_f32", mm_fwd), ("rows", rows_fwd), ("dense", dense_fwd)]),
                "dX": (dref, dbound, 4.0 * (m * n + n * k + m * k * (2 if dgelu_in else 1)),
                       [("library", lib_dx), ("mm_f32", mm_dx), ("rows", rows_dx), ("dense", dense_dx)]),
                "dW": (wref, wbound, 4.0 * (m * n + m * k + n * k),
                       [("library", lib_dw), ("mm_f32", mm_dw), ("rows", rows_dw), ("dense", dense_dw)]),
            }
            roof_flops = flops / 2.5e15
            chains = {"fwd": k + 2, "dX": n + 2, "dW": m + 72}
            for dname, (ref, bound, nbytes, paths) in dirs.items():
                chain = chains[dname]
                roof_us = max(roof_flops, nbytes / 8e12) * 1e6
                for pname, fn in paths:
                    if pname == "mm_f32" and not mm_ok:
                        continue
                    try:
                        out = fn()
                    except Exception as err:   # a path that does not take this shape
                        print(f"{batch:>5} {name:>5} {dname:>4} {pname:>8}  n/a ({type(err).__name__}: {str(err)[:60]})")
                        continue
                    torch.cuda.synchronize()
                    # the library path's bf16 result: one more rounding of 2^-9 relative to the unbiased product, whose size sum |a b| bounds
                    r = ratio(out, ref, bound + (2.0 ** -8 * (ref.abs() + bound / (chain * U)) if pname == "library" else 0))
                    if not r <= 1.0:
                        print(f"{batch:>5} {name:>5} {dname:>4} {pname:>8} {'WRONG':>9} {'':>8} {'':>6} {r:9.3g}")
                        continue
                    us = timed(fn, args.reps)
                    totals[(batch, pname)] = totals.get((batch, pname), 0.0) + us
                    print(f"{batch:>5} {name:>5} {dname:>4} {pname:>8} {us:9.1f} {flops / us / 1e6:8.1f} {100 * roof_us / us:6.1f} {r:9.3g}")
            del x, w, dy, x64, w64, dy64, ref
            torch.cuda.empty_cache()
    print("# per block (qkv + proj + fc1 + fc2, fwd + dX + dW), us:")
    for batch in args.batches:
        row = "  ".join(f"{p}={totals[(batch, p)]:.1f}" for p in ("library", "mm_f32", "rows", "dense") if (batch, p) in totals)
        print(f"# batch {batch}: {row}")


if __name__ == "__main__":
    main()
