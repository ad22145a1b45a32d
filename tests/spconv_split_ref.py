"""The three-piece split sparse convolution (csrc/ftx_spconv_split.hip; include/ftx.h states the contract) on top of
tests/split_ref.py, for any device: the family's weight-gradient tile length, emulations of the pair GEMM + reduce and of the weight
gradient from any subset of the piece products, and the two gates of its tests.  Both gates compare with float64 on the UNROUNDED
operands.

G1, per element:   |got - S| <= (6 m_g + m_r + 8) * 2^-24 * R
    R the same computation on |operands|; m_g the GEMM chain (c_in for the pair GEMM, the scatter form and dense rows; tile length +
    tiles of the offset + 16 for the weight gradient), six piece products per step; m_r the reduce chain (kvol over the offsets, 0
    for the scatter form, dense rows and the weight gradient, which have no reduce; + 1 with a bias).  The dense split family's G1 with the chains of tests/test_spconv_regimes_gpu.py: derived
    from the rounding steps of the contract, not measured.
G2:                E <= T / 2,  E = rms(got - S) / rms(S),  T = rms(S5 - S) / rms(S)
    S5 the five products without mm summed in float64 (tests/split_ref.py g2_passes).  Asserted from 4 096 output elements on."""
import numpy as np
import torch

from tests import spconv_regimes as S
from tests import split_ref as R
from tests.norm_ref import U, conv_ref, ratio, wgrad_ref

G2_MIN_ELEMENTS = 4096
BF16_ONLY = ("hh",)     # with pieces {"h": bf16(x)} alone: the bf16 family's operands


def split_tile_len(lib, n_pairs, ca, cg, kvol):
    """csrc/ftx_spconv_common.h spconv_wgrad_tile_len<SpconvSplit>() (table and step: csrc/ftx_spconv_split.hip), checked against the
    library's workspace query.  Host only."""
    mi, wmg, ni, wng = S.wgrad_config(ca, cg)
    mn_tiles = S.cdiv(ca, 32 * mi * wmg) * S.cdiv(cg, 32 * ni * wng)
    slots = 256 * int(lib.ftx_spconv_wgrad_split_table_blocks(mi, wmg, ni, wng))
    length = 256
    for rounds in range(1, 65):
        tiles = max((slots * rounds * 15 // 16) // mn_tiles - (kvol + 1) // 2, 1)
        length = S.cdiv(S.cdiv(n_pairs, tiles), 64) * 64
        if length <= 4096:
            break
    length = max(length, 256)
    tiles = int(lib.ftx_spconv_pairs_wgrad_split_workspace_bytes(n_pairs, ca, cg, kvol)) // (4 * ca * cg)
    assert tiles == S.cdiv(n_pairs, length) + kvol, (n_pairs, ca, cg, kvol, tiles, length)
    return length


def host_pair_list(g, sizes, n_src, n_dst):
    """tests/test_spconv_regimes_gpu.py pair_list() without the device copies: (src, dst, koff), distinct destination rows per offset."""
    koff = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    src = torch.randint(0, n_src, (int(koff[-1]),), generator=g)
    dst = torch.empty_like(src)
    for k, c in enumerate(sizes):
        s = int(koff[k])
        if c:
            dst[s:s + c] = torch.randperm(n_dst, generator=g)[:c]
    return src, dst, koff


def pieces(x):
    return dict(zip("hml", R.split3(x)))


# ---------------------------------------------------------------- float64 sums of piece products
def conv_products(A, W, src, dst, koff, n_dst, products):
    """The convolution from the named piece products, every product summed in float64."""
    pa, pw = pieces(A), pieces(W)
    out = torch.zeros(n_dst, W.shape[2], dtype=torch.float64)
    for p in products:
        out += conv_ref(pa[p[0]].double(), pw[p[1]].double(), src, dst, koff, n_dst)
    return out


def wgrad_products(A, ia, G, ig, koff, products):
    pa, pg = pieces(A), pieces(G)
    out = torch.zeros(koff.shape[0] - 1, A.shape[1], G.shape[1], dtype=torch.float64)
    for p in products:
        out += wgrad_ref(pa[p[0]].double(), ia, pg[p[1]].double(), ig, koff)
    return out


# ---------------------------------------------------------------- fp32-chunked emulations of the kernels
def conv_emulated(A, W, src, dst, koff, n_dst, products=R.SIX, rounded=False):
    """Pair GEMM + reduce as the kernels run it: per pair row the products in 16-wide k-steps into two fp32 accumulators
    (split_ref.gemm), then the fp32 sum over the offsets in ascending order.  rounded=True: the bf16 family instead (operands rounded
    to bf16, one accumulator)."""
    out = torch.zeros(n_dst, W.shape[2], dtype=torch.float32)
    for k in range(W.shape[0]):
        s, e = int(koff[k]), int(koff[k + 1])
        if e == s:
            continue
        a = A[src[s:e]]
        if rounded:
            rows = R.gemm(a.bfloat16().float(), W[k].bfloat16().float(), BF16_ONLY, accumulate="fp32")
        else:
            rows = R.gemm(a, W[k], products, accumulate="fp32")
        out.index_add_(0, dst[s:e], rows)      # distinct rows per offset: one fp32 add per element and offset
    return out


def wgrad_emulated(A, ia, G, ig, koff, tile_len, products=R.SIX, rounded=False):
    """Weight gradient as the kernels run it: tiles of `tile_len` pairs of one offset, the pair index in 16-wide k-steps into two
    fp32 accumulators, the tiles of an offset added in fp32 in tile order."""
    kvol = koff.shape[0] - 1
    out = torch.zeros(kvol, A.shape[1], G.shape[1], dtype=torch.float32)
    for k in range(kvol):
        s, e = int(koff[k]), int(koff[k + 1])
        for t0 in range(s, e, tile_len):
            a, g = A[ia[t0:min(t0 + tile_len, e)]].T.contiguous(), G[ig[t0:min(t0 + tile_len, e)]]
            if rounded:
                out[k] += R.gemm(a.bfloat16().float(), g.bfloat16().float(), BF16_ONLY, accumulate="fp32")
            else:
                out[k] += R.gemm(a, g, products, accumulate="fp32")
    return out


# ---------------------------------------------------------------- the gates
def conv_gate(A, W, src, dst, koff, n_dst, reduce_chain=None):
    """(S, bound) of G1 for a convolution over a pair list; reduce_chain defaults to kvol."""
    A64, W64 = A.double(), W.double()
    m_r = W.shape[0] if reduce_chain is None else reduce_chain
    ref = conv_ref(A64, W64, src, dst, koff, n_dst)
    bound = (6 * W.shape[1] + m_r + 8) * U * conv_ref(A64.abs(), W64.abs(), src, dst, koff, n_dst)
    return ref, bound


def wgrad_gate(A, ia, G, ig, koff, tile_len):
    """(S, bound) of G1 for the weight gradient at this family's tile length."""
    A64, G64 = A.double(), G.double()
    kvol = koff.shape[0] - 1
    tiles = (koff[1:] - koff[:-1] + tile_len - 1) // tile_len
    m_g = (tile_len + tiles + 16).double().view(kvol, 1, 1)
    ref = wgrad_ref(A64, ia, G64, ig, koff)
    bound = (6 * m_g + 8) * U * wgrad_ref(A64.abs(), ia, G64.abs(), ig, koff)
    return ref, bound


def wgrad_mutants_resolved(A, ia, G, ig, koff):
    """The two mutants of tests/norm_ref.py wgrad_mutants -- one pair's contribution removed; that pair credited to the neighbouring
    offset (with one offset: given the next pair's G row) -- planted in the pair that G1 resolves best instead of in the middle of the
    largest offset.  The bound of an element of dW[k] grows with the pairs of offset k: at full size the centre offset holds 81 k
    pairs and (6 (L + tiles + 16) + 8) * 2^-24 * sum |a||g| is about 11-18 there, the size of ONE pair's largest product, so the gate
    cannot tell a pair of average size in that offset from rounding (the fp32 family's bound, six times tighter, can).  The pair taken
    is the one with the largest (max |a| * max |g|) / (pairs of its offset)."""
    kvol = koff.shape[0] - 1
    cnt = koff[1:] - koff[:-1]
    k_of = torch.repeat_interleave(torch.arange(kvol), cnt)
    score = A.abs().amax(1)[ia] * G.abs().amax(1)[ig] / cnt[k_of].double()
    if kvol == 1:
        score[-1] = 0          # the second mutant reads the next pair
    p = int(torch.argmax(score))
    k = int(k_of[p])
    kn = k + 1 if k + 1 < kvol else k - 1
    outer = torch.outer(A[ia[p]], G[ig[p]])
    if kvol == 1:
        return [[((k,), -outer)], [((k,), torch.outer(A[ia[p]], G[ig[p + 1]]) - outer)]]
    return [[((k,), -outer)], [((k,), -outer), ((kn,), outer)]]


def g1_ratio(got, ref, bound):
    return ratio(got.detach().cpu(), ref, bound)


def g2_figures(got, ref, s5):
    """(E, T) of G2 from the result, S and S5."""
    rs = R.rms(ref)
    return R.rms(got.detach().cpu().double() - ref) / rs, R.rms(s5 - ref) / rs


def g2_passes(got, ref, s5):
    e, t = g2_figures(got, ref, s5)
    return e <= t / 2
