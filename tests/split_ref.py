"""Torch emulation of the three-piece operand split of the ftx_dense_*_split kernels (include/ftx.h states the contract), for any
device: the pieces, a GEMM from any subset of the nine piece products with float64 or fp32-chunked accumulation, and gate G2.

    h = bf16(x),  m = bf16(x - h),  l = bf16((x - h) - m)      round-to-nearest-even, the subtractions in fp32 (exact)

A product is named by two letters, the first the piece of the left operand: "hm" = h(a) * m(b)."""
import torch

SIX = ("mm", "hl", "lh", "hm", "mh", "hh")     # what the kernels sum; the five corrections smallest first, then hh
FIVE = ("hl", "lh", "hm", "mh", "hh")          # mm left out
THREE = ("hm", "mh", "hh")
NINE = ("ll", "ml", "lm") + SIX


def split3(x):
    """fp32 x -> (h, m, l), fp32 tensors whose values are bf16 numbers.  h not finite: m = l = 0."""
    assert x.dtype == torch.float32
    h = x.to(torch.bfloat16).float()
    r = torch.where(torch.isfinite(h), x - h, torch.zeros_like(x))
    m = r.to(torch.bfloat16).float()
    l = (r - m).to(torch.bfloat16).float()
    return h, m, l


def _pieces(x):
    return dict(zip("hml", split3(x)))


def gemm(a, b_kn, products=SIX, accumulate="float64", chunk=16, two_accumulators=True):
    """a (m, k) @ b_kn (k, n) from the named piece products.

    accumulate="float64": every product summed in float64 (no accumulation error: what an ideal kernel of those products returns).
    accumulate="fp32":    the reduction in chunks of `chunk`; a chunk's sum of one product is formed exactly (float64) and rounded once
                          into an fp32 accumulator, products in the order given.  two_accumulators: "hh" goes to an accumulator of its
                          own and the others to a second one, added once at the end (the kernels' form); otherwise one sequential chain.
    Returns float64 (accumulate="float64") or fp32."""
    pa, pb = _pieces(a), _pieces(b_kn)
    if accumulate == "float64":
        out = torch.zeros(a.shape[0], b_kn.shape[1], dtype=torch.float64, device=a.device)
        for p in products:
            out += pa[p[0]].double() @ pb[p[1]].double()
        return out
    assert accumulate == "fp32"
    main = torch.zeros(a.shape[0], b_kn.shape[1], dtype=torch.float32, device=a.device)
    corr = torch.zeros_like(main)
    for c0 in range(0, a.shape[1], chunk):
        for p in products:
            part = pa[p[0]][:, c0:c0 + chunk].double() @ pb[p[1]][c0:c0 + chunk].double()
            if two_accumulators and p != "hh":
                corr = (corr.double() + part).float()
            else:
                main = (main.double() + part).float()
    return main + corr


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def g2_figures(out, a, b_kn, add=None):
    """(E, T) of gate G2 for out ~ a @ b_kn (+ add, a bias row):  E = rms(out - S) / rms(S),  T = rms(S5 - S) / rms(S),  S the float64
    GEMM on the unrounded fp32 operands, S5 the five products without mm summed in float64."""
    s = a.double() @ b_kn.double()
    s5 = gemm(a, b_kn, FIVE)
    if add is not None:
        s, s5 = s + add.double(), s5 + add.double()
    return rms(out.double() - s) / rms(s), rms(s5 - s) / rms(s)


def g2_passes(out, a, b_kn, add=None):
    """Gate G2: E <= T / 2.  An implementation that drops any product of mm's size cannot beat T however it accumulates; the emulated
    six-product scheme sits at E / T = 0.11 .. 0.22."""
    e, t = g2_figures(out, a, b_kn, add)
    return e <= t / 2
