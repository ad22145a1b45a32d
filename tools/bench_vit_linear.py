"""Times the bf16 ViT Linears (qkv, proj, fc1, fc2) per direction at batch 1, 4 and 8 (M = 578 x batch), in one process:

  (a) library  the library bf16 path as models/transformers._LinearFn runs it: casts of x, w and dy to bf16, the bf16 GEMM, the widening
               of its bf16 result to fp32, the bias add; fc1's forward adds nn.GELU, fc2's dX adds the GELU backward (fc1's dY)
  (b) mm_f32   torch.mm(bf16, bf16, out_dtype=torch.float32) on pre-cast operands (not timed: the casts), where this torch serves it
  (c) rows     the LiDAR branch's ftx_rows_gemm_bf16 (forward / dX) and dense ftx_spconv_pairs_wgrad_bf16 (dW)
  (d) dense    the new ftx_dense_gemm_bf16 (with its bias / GELU / DGELU epilogue) and ftx_dense_wgrad_bf16
  (e) fp32     the fp32 library path as _LinearFn(..., False) runs it: torch.addmm / mm in fp32, plus the separate GELU (fc1's forward) and
               gelu_backward (fc2's dX) kernels
  (f) split    ftx_dense_gemm_split / ftx_dense_wgrad_split (vit_linear_impl="ftx_split"): three bf16 pieces per fp32 operand, six products
               summed in fp32, the same fused epilogues

Paths (e) and (f) claim fp32 semantics, so they are checked against float64 on the UNROUNDED operands, per element, with the bound
(L + 2) * 2^-24 * sum |a b| for fp32 and (6 L + 8) * 2^-24 * sum |a b| for split (tests/test_vit_linear_split_gpu.py derives it), and their
whole-output error E = rms(out - S) / rms(S) of the GEMM without bias or GELU is printed in the last column (measured separately, not timed).

--trunk IMPL times the 12-block ViT trunk, forward + backward at batch 4 as captured HIP graphs, under vit_linear_impl=IMPL (set_bf16 off):
median of five timed samples after warm-up, by HIP events.

Each other result is checked against float64 on the bf16-rounded operands: paths (b)-(d) must meet the fp32-output bound
(chain * 2^-24 * sum |a b|); the library path must meet the same bound widened by its bf16 output rounding (2^-8 relative to the
result and to sum |a b|).  A result
that misses its bound is printed as WRONG and no time is reported for it.  roof = max(flops / 2.5 PF, bytes / 8 TB/s) with the fp32
operand and output bytes; "roof%" = roof / measured.

usage: python tools/bench_vit_linear.py [--batches 1 4 8] [--reps 50] [--paths library dense fp32 split] [--trunk library|ftx_split]"""
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


PATHS = ("library", "mm_f32", "rows", "dense", "fp32", "split")


def rel_rms(out, ref):
    return float((out.double() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())


def time_trunk(impl, batch=4, samples=5, iters=5):
    """12-block trunk, forward + backward, graphs on: ms per iteration, the median of `samples` samples of `iters` iterations each."""
    from fusiontransformer_amd.models.transformers import image_2d_distilled_transformer
    torch.manual_seed(0)
    vit = image_2d_distilled_transformer(pretrained=False, remove_tokens_outputs=True)
    vit.set_attention_impl("ftx")
    vit.set_linear_impl(impl)
    vit.graph_taps = [len(vit.blocks) - 1]
    for p in vit.norm.parameters():
        p.requires_grad_(False)   # forward_blocks never applies the final norm
    vit = vit.cuda().train()
    x = torch.randn(batch, 3, 384, 384, device="cuda")
    tap = str(len(vit.blocks) - 1)
    go = None

    def step():
        nonlocal go
        out = vit.forward_blocks(x)[tap]
        if go is None:
            go = torch.randn_like(out)
        out.backward(go)

    spf.LAUNCH_LOG = []
    try:
        step()
        torch.cuda.synchronize()
        kinds = [k for k, *_ in spf.LAUNCH_LOG]
    finally:
        spf.LAUNCH_LOG = None
    for _ in range(5):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / iters)
    times.sort()
    print(f"# trunk: 12 blocks, batch {batch}, forward + backward, vit_linear_impl={impl}, graphs {vit.graph_state()}: "
          f"median {times[len(times) // 2]:.3f} ms (min {times[0]:.3f}, max {times[-1]:.3f}); capturing step launched "
          f"{kinds.count('vit_gemm_split')} vit_gemm_split, {kinds.count('vit_wgrad_split')} vit_wgrad_split")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--paths", nargs="+", default=list(PATHS), choices=PATHS)
    ap.add_argument("--trunk", choices=("library", "ftx_split"), default=None)
    args = ap.parse_args()
    if args.trunk:
        print(f"# torch {torch.__version__}, device {torch.cuda.get_device_name()}")
        time_trunk(args.trunk)
        return
    mm_ok = has_mm_out_dtype()
    print(f"# torch {torch.__version__}, device {torch.cuda.get_device_name()}, mm(out_dtype=float32) on bf16: {'yes' if mm_ok else 'no'}")
    print(f"{'batch':>5} {'linear':>5} {'dir':>4} {'path':>8} {'us':>9} {'TFLOP/s':>8} {'roof%':>6} {'err/bound':>9} {'E':>9}")
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

            # paths "fp32" and "split": float64 on the unrounded operands; unit = 2^-24 * sum |a b| (+ |bias|), scaled by the path's chain
            xu, wu, dyu = x.double(), w.double(), dy.double()
            su = xu @ wu.t() + b.double()
            sbu = U * (xu.abs() @ wu.abs().t() + b.double().abs())
            du = dyu @ wu
            dbu = U * (dyu.abs() @ wu.abs())
            wrefu = dyu.t() @ xu
            wbu = U * (dyu.abs().t() @ xu.abs())

            def unrounded(dname, c):
                """(reference, bound) of direction dname for a path whose accumulation constant is c(L) = factor on the unit."""
                if dname == "fwd":
                    sb_ = c(k) * sbu
                    return (gelu64(su), dgelu64(su).abs() * sb_ + 8 * U * (su.abs() + 1e-30)) if gelu_out else (su, sb_)
                if dname == "dX":
                    db_ = c(n) * dbu
                    if dgelu_in:
                        dg_ = dgelu64(pre_fc1.double())
                        return du * dg_, db_ * dg_.abs() + 8 * U * du.abs() * (1 + pre_fc1.double().abs()) + 1e-30
                    return du, db_
                return wrefu, c(m + 72) * wbu

            chain_of = {"fp32": lambda L: L + 2, "split": lambda L: 6 * L + 8}
            bare = {   # the GEMM alone (no bias, no GELU) of each direction, for E
                "fp32": {"fwd": lambda: x @ w.t(), "dX": lambda: dy @ w, "dW": lambda: dy.t() @ x},
                "split": {"fwd": lambda: spf._dense_gemm(x, w, 0, spf.EPI_NONE, mode="split")[0],
                          "dX": lambda: spf._dense_gemm(dy, w, 1, spf.EPI_NONE, mode="split")[0], "dW": lambda: spf._dense_wgrad(dy, x, "split")},
            }
            bare_ref = {"fwd": su - b.double(), "dX": du, "dW": wrefu}

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

            def fp32_fwd():
                y = torch.addmm(b, x, w.t())
                return F.gelu(y) if gelu_out else y

            def fp32_dx():
                dx = dy @ w
                return torch.ops.aten.gelu_backward(dx, pre_fc1) if dgelu_in else dx

            def fp32_dw():
                return dy.t() @ x

            def split_fwd():
                if gelu_out:
                    return spf._dense_gemm(x, w, 0, spf.EPI_BIAS_GELU, bias=b, with_pre=True, mode="split")[0]
                return spf._dense_gemm(x, w, 0, spf.EPI_BIAS, bias=b, mode="split")[0]

            def split_dx():
                if dgelu_in:
                    return spf._dense_gemm(dy, w, 1, spf.EPI_DGELU, pre_in=pre_fc1, mode="split")[0]
                return spf._dense_gemm(dy, w, 1, spf.EPI_NONE, mode="split")[0]

            def split_dw():
                return spf._dense_wgrad(dy, x, "split")

            flops = 2.0 * m * n * k
            dirs = {
                "fwd": (fref, fbound, 4.0 * (m * k + n * k + m * n * (2 if gelu_out else 1)),
                        [("library", lib_fwd), ("mm_f32", mm_fwd), ("rows", rows_fwd), ("dense", dense_fwd), ("fp32", fp32_fwd), ("split", split_fwd)]),
                "dX": (dref, dbound, 4.0 * (m * n + n * k + m * k * (2 if dgelu_in else 1)),
                       [("library", lib_dx), ("mm_f32", mm_dx), ("rows", rows_dx), ("dense", dense_dx), ("fp32", fp32_dx), ("split", split_dx)]),
                "dW": (wref, wbound, 4.0 * (m * n + m * k + n * k),
                       [("library", lib_dw), ("mm_f32", mm_dw), ("rows", rows_dw), ("dense", dense_dw), ("fp32", fp32_dw), ("split", split_dw)]),
            }
            roof_flops = flops / 2.5e15
            chains = {"fwd": k + 2, "dX": n + 2, "dW": m + 72}
            for dname, (ref, bound, nbytes, paths) in dirs.items():
                chain = chains[dname]
                roof_us = max(roof_flops, nbytes / 8e12) * 1e6
                for pname, fn in paths:
                    if pname not in args.paths or (pname == "mm_f32" and not mm_ok):
                        continue
                    try:
                        out = fn()
                    except Exception as err:   # a path that does not take this shape
                        print(f"{batch:>5} {name:>5} {dname:>4} {pname:>8}  n/a ({type(err).__name__}: {str(err)[:60]})")
                        continue
                    torch.cuda.synchronize()
                    # the library path's bf16 result: one more rounding of 2^-9 relative to the unbiased product, whose size sum |a b| bounds
                    e_col = ""
                    if pname in chain_of:
                        r = ratio(out, *unrounded(dname, chain_of[pname]))
                        e_col = f"{rel_rms(bare[pname][dname](), bare_ref[dname]):9.3g}"
                    else:
                        r = ratio(out, ref, bound + (2.0 ** -8 * (ref.abs() + bound / (chain * U)) if pname == "library" else 0))
                    if not r <= 1.0:
                        print(f"{batch:>5} {name:>5} {dname:>4} {pname:>8} {'WRONG':>9} {'':>8} {'':>6} {r:9.3g}")
                        continue
                    us = timed(fn, args.reps)
                    totals[(batch, pname)] = totals.get((batch, pname), 0.0) + us
                    print(f"{batch:>5} {name:>5} {dname:>4} {pname:>8} {us:9.1f} {flops / us / 1e6:8.1f} {100 * roof_us / us:6.1f} {r:9.3g} {e_col}")
            del x, w, dy, x64, w64, dy64, ref
            torch.cuda.empty_cache()
    print("# per block (qkv + proj + fc1 + fc2, fwd + dX + dW), us:")
    for batch in args.batches:
        row = "  ".join(f"{p}={totals[(batch, p)]:.1f}" for p in PATHS if (batch, p) in totals)
        print(f"# batch {batch}: {row}")


if __name__ == "__main__":
    main()
