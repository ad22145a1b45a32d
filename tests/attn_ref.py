"""fp32 attention (csrc/ftx_attn.hip: attn_fwd_kernel, attn_delta_kernel, attn_bwd_kv_kernel, attn_bwd_q_kernel) against float64,
with bars that are computed from a yardstick and never written down as numbers.  Plain numpy / torch on the CPU; no GPU import.

reference(qkv, go, scale, dtype)   the timm formula (softmax(Q K^T scale) V, three explicit ops, torch autograd), in float64 (THE
                                   reference) or float32 (the YARDSTICK: what an unfused fp32 implementation of the same formula gives).
abs_gradients(qkv, go, scale)      the float64 dQ / dK formulas with every term replaced by its absolute value: the natural size of
                                   the sums behind dQ and dK.  They never vanish, while dQ and dK themselves do (exactly, at T = 1:
                                   dS = P (dP - sum P dP) = 0), so errors of dQ and dK are taken relative to these.
errors(got, ref64, absg)           per tensor (out, lse, dq, dk, dv) two numbers: a relative L2 and a max-abs over max-abs.
bar(E32, max_abs_lse)              the bar for those numbers, from E32 = errors(yardstick, ref64, absg) on the SAME inputs.
emulate(qkv, go, scale, split)     a numpy fp32 model of the kernels' arithmetic, so the bars can be exercised without a GPU.  It is not a
                                   second reference: nothing is ever compared against it.

The bar.  u = 2^-24 is the unit roundoff of fp32.

    out, dq, dk, dv:   4 * E32 + 4 * u * max(1, max|lse|)
    lse:               4 * E32 + 8 * u

* E32 is what fp32 costs on these inputs for the formula itself: it scales with T, with the peakedness of the softmax and with the
  cancellation in dP - delta, which no constant could follow.
* The factor 4 allows for a different order of the same fp32 sums: the kernels sum the head dim in MFMA k-chains, the keys in 32-key
  tiles with a running-maximum rescale, and the key (query) groups in a pairwise tree; the yardstick sums whatever way the CPU BLAS
  does.  Rounding errors of two orders of an n-term sum are independent and of the same size, so their difference is within ~sqrt(2) of
  either; 4 leaves room for that and for the spread between tensors, and nothing more: a kernel that rounds an operand to bf16 or
  xf32, uses a cheaper exp, or accumulates in less than fp32 is 100 to 10000 times over E32 (tests/test_attn_fp32_host.py shows each).
* The additive term counts roundings of the exponent path that the unfused formula does not have.  The kernels work in the exp2 domain
  and the backward rebuilds P = exp2(S' - lse * log2e) from the stored lse, where S' is a differently rounded product than the forward's
  (the forward and dQ fold sl2 = scale * log2e into Q, dK / dV fold it into K).  With |S'| ~ |lse * log2e| =: x near the row maximum,
  four roundings each move the exponent by at most u * x:   (1) sl2 folded into Q or K (every product of the chain carries the
  factor's rounding),  (2) lse = (m + log2 l) * LN2 in the forward,  (3) lse * LOG2E in the backward,  (4) the subtraction S' - lse2
  (its result is small, but its operands were rounded at size x).  An exponent error e changes exp2 by e * ln2 relative, and
  x * ln2 = |lse|, so together at most 4 * u * |lse| relative error on P, and through P on dV, dS, dQ, dK; the forward's out carries the
  same term through (1) alone and is given the same allowance.  max(1, .) keeps the bar positive where E32 is exactly 0 (T = 1: the
  yardstick's softmax of one score is exactly 1 and its dS exactly 0).
* lse itself is (m + log2 l) * LN2: two roundings the yardstick's logsumexp also has, plus log2f, the product by LN2, the folded sl2
  and the exp2 of the row sum: 8 roundings of size u relative to max(1, |lse|), which is how the lse error is normalised.

Inputs (make_inputs): seeded Gaussians with Q and K multiplied by 1 ("gauss", nearly flat softmax), 3 ("peaked", |lse| up to ~50) or
30 ("large", |lse| up to ~5000).  In these three every 8th query (tokens 5, 13, ...) is then divided by 16: real tokens do not all
have one norm, and a launch should hold sharp and nearly flat softmax rows side by side -- within one wave, where the rescale branch
is taken for all 32 queries if any of them needs it.  The quiet rows keep lse near ln T in every kind, which is where a fault of
size exp(-lse) shows (a zero key let through the mask adds exactly that to the row sum and nothing else); on rows with lse > 17 such a
fault is below fp32 rounding and no bar can see it.  Two constructed cases: "ascending" (key t = t * c times a fixed direction on which every query
has a positive component: every key tile raises the running maximum, so the rescale runs in every iteration) and "late_max" (the
dominant key of every query is the last valid token: it sits in the ragged tile, and for most (T, split) in a key group other than 0,
so the (m, l, O) merge has to carry it).

The bf16-operand kernels (attn_fwd_bf16_kernel, attn_delta_bf16_kernel, attn_bwd_kv_bf16_kernel, attn_bwd_q_bf16_kernel) are held to
their precision contract (csrc/ftx_attn.hip, "Precision contract") by the same method.

rounded(a)                         bf16 round-to-nearest-even, as float64: what the kernels make of Q, K, V and dO.
reference(rounded(qkv), rounded(go), scale)      THE reference of the bf16 kernels: float64 on the rounded operands, nothing else rounded.
yardstick_bf16(qkv, go, scale)     the contract stated unfused in float64: rounded operands; P = softmax(S) rounded to bf16 as the operand
                                   of P V and P^T dO; delta = rowsum(out * bf16(dO)); dS = P (dP - delta) scale formed from the unrounded P
                                   and rounded to bf16 as the operand of dS K and dS^T Q.  Its lse is the reference's.
bar_bf16(E_yard, E32_lse, max_abs_lse)           the bars, from E_yard = errors(yardstick_bf16, ...) and the float32 yardstick's lse error.
emulate_bf16(qkv, go, scale, split)              the numpy model of the bf16 kernels: emulate's tile loop with the contract's roundings.

    out, dq, dk, dv:   4 * E_yard + 4 * u * max(1, max|lse|)          (u = 2^-24 still: the accumulators and the exponent path are fp32)
    lse:               4 * E32 + 8 * u                                 (the fp32 bar, E32 on the rounded operands)

* E_yard is what the contract's two operand roundings (P, dS; relative size 2^-9 each) cost on these inputs: ~1e-3 of a gradient on
  flat softmax rows, less where P is nearly 0 or 1 (such values round exactly or nearly so), nothing at T = 1 (P = 1).
* The factor 4 carries over, for the same reason.  The kernels do not round the element the yardstick rounds: the forward rounds the
  unnormalised exp2(s - m_running) and divides the fp32 sum by l afterwards (rescales by exp2(m_old - m_new) and 1 / l in between act
  on the fp32 accumulator and keep a rounding's relative size), the yardstick rounds the normalised P; the backward rounds an fp32 P
  rebuilt from lse and a dS formed in fp32.  Each is a rounding of relative size <= 2^-9 of the same element at another position of
  its mantissa, so the two sets of rounding errors are independent and of one size, and the error of a sum over them is within
  ~sqrt(2) of the yardstick's: the situation of two orders of one fp32 sum above.  Where the kernel happens to round the same value
  (dS, which differs from the yardstick's by fp32 rounding only) its error equals the yardstick's, a ratio of 0.25.  4 leaves no room
  for a missing or extra key, a lost tile or an operand rounded twice: tests/test_attn_bf16_host.py shows each.
* The additive fp32 term stays.  The exponent path is the fp32 kernels': scores in the exp2 domain, P rebuilt in the backward as
  exp2(S * sl2 - lse * log2e) with |S * sl2| ~ |lse * log2e| = x; the four roundings of size u * x are (1) the product S * sl2 (the
  scale is no longer folded into an operand, it multiplies the fp32 score), (2), (3), (4) as above: 4 * u * |lse| relative on P.  On the
  sharp rows of the "large" inputs (|lse| ~ 5000) the softmax is saturated, P is 0 or 1 and rounds exactly, and this term is their
  whole error (E_yard of those inputs comes from their quiet rows); at T = 1 E_yard is exactly 0 and the term keeps the bar
  positive.
* lse gets the fp32 bar.  By the contract the scores are exact fp32 sums of exact products (bf16 x bf16 fits fp32), and m, l and lse
  come from the unrounded exponentials: the kernel's lse is an fp32 evaluation of the reference's own formula on the same operands,
  with the roundings counted above for fp32.  The yardstick's lse is float64 (E_yard["lse"] = 0), so E32 comes from
  reference(rounded(qkv), rounded(go), scale, float32).  This is the tensor that pins the operand rounding: operands truncated instead
  of rounded, the scale folded into Q before rounding, or a row sum over the rounded P move lse by 2^-9-sized amounts: tens to
  thousands of bars.
"""
import numpy as np
import torch

U = 2.0 ** -24
HD = 64
TENSORS = ("out", "lse", "dq", "dk", "dv")
F32 = np.float32
LOG2E = F32(1.4426950408889634)
LN2 = F32(0.6931471805599453)

KINDS = {"gauss": 1.0, "peaked": 3.0, "large": 30.0}
QUIET = slice(5, None, 8)      # every 8th query, from token 5

# The accuracy cases of the GPU tests (tests/test_attn_fp32_gpu.py, tests/test_attn_bf16_gpu.py): (kind, T, scale).
EDGES = [1, 31, 32, 33, 64, 127, 128, 129, 257, 578]     # below one 32-token tile, its edges, the 4-wave block's edges, the ViT's T
ACCURACY = ([(kind, T, 0.125) for kind in ("gauss", "peaked") for T in EDGES] +
            [(kind, 129, 0.1) for kind in ("gauss", "peaked")] +                      # a scale that is not a power of two
            # 290: the last token lies in key tile 9, i.e. in a key group other than 0 under every split (at 257 it is tile 8: group 0)
            [(kind, T, 0.125) for kind in ("ascending", "late_max") for T in (70, 257, 290)])
LARGE_T = [100, 578]


# ---------------------------------------------------------------- inputs
def make_inputs(kind, B, T, H, seed=0):
    """qkv (B, T, 3, H, 64) and grad_out (B, T, H * 64), float32, from a generator seeded by (seed, kind, B, T, H)."""
    rng = np.random.default_rng([seed, sorted(list(KINDS) + ["ascending", "late_max"]).index(kind), B, T, H])
    qkv = rng.standard_normal((B, T, 3, H, HD))
    go = rng.standard_normal((B, T, H * HD))
    if kind in KINDS:
        qkv[:, :, :2] *= KINDS[kind]
        qkv[:, QUIET, 0] /= 16.0          # the quiet queries (module docstring)
    else:
        d = rng.standard_normal((B, 1, H, HD))
        d /= np.linalg.norm(d, axis=-1, keepdims=True)          # a fixed direction per (batch, head)
        q = qkv[:, :, 0]
        along = (q * d).sum(-1, keepdims=True)
        if kind == "ascending":
            # q.d in [0.5, ~4); key t = t * c * d with c = 64 / T: scores rise with t up to 8 * q.d at scale 1/8, and a query
            # weighs the last T / (8 q.d) keys or so: several tiles at every T used
            q += (0.5 + np.abs(rng.standard_normal(along.shape)) - along) * d
            qkv[:, :, 1] = np.arange(T).reshape(1, T, 1, 1) * (64.0 / T) * d
        else:
            # q.d >= 4, last key = 16 d: its score is >= 8 at scale 1/8, the other keys' scores are ~N(0, 1)
            q += (4.0 + np.abs(rng.standard_normal(along.shape)) - along) * d
            qkv[:, T - 1, 1] = 16.0 * d[:, 0]
    return qkv.astype(F32), go.astype(F32)


# ---------------------------------------------------------------- reference and yardstick
def _t(a, dtype):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dtype)


def reference(qkv, go, scale, dtype=torch.float64):
    """timm's Attention.forward as three explicit ops, and its autograd backward, in `dtype` on the CPU: out (B, T, H * 64),
    lse (B, H, T), grad_qkv (B, T, 3, H, 64), returned as float64 tensors."""
    B, T, _, H, D = qkv.shape
    r = _t(qkv, dtype).clone().requires_grad_(True)
    q, k, v = r.permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * scale
    lse = torch.logsumexp(s, dim=-1)
    out = (s.softmax(dim=-1) @ v).transpose(1, 2).reshape(B, T, H * D)
    out.backward(_t(go, dtype))
    return out.detach().double(), lse.detach().double(), r.grad.double()


def rounded(a):
    """bf16 round-to-nearest-even of a float32 array or tensor, as a float64 tensor."""
    return _t(a, torch.float32).to(torch.bfloat16).double()


def yardstick_bf16(qkv, go, scale):
    """The bf16 kernels' precision contract as explicit float64 ops on the CPU (module docstring): out, lse, grad_qkv, shaped as
    reference's."""
    B, T, _, H, D = qkv.shape
    rb = lambda a: a.to(torch.bfloat16).double()          # the rounding of an MFMA operand
    q, k, v = rounded(qkv).permute(2, 0, 3, 1, 4)
    g = rounded(go).reshape(B, T, H, D).transpose(1, 2)
    s = (q @ k.transpose(-2, -1)) * scale
    lse = torch.logsumexp(s, dim=-1)
    p = s.softmax(dim=-1)
    out = rb(p) @ v
    delta = (out * g).sum(-1, keepdim=True)
    ds = rb(p * (g @ v.transpose(-2, -1) - delta) * scale)
    grad = torch.stack([ds @ k, ds.transpose(-2, -1) @ q, rb(p).transpose(-2, -1) @ g], 0).permute(1, 3, 0, 2, 4)
    return out.transpose(1, 2).reshape(B, T, H * D), lse, grad.contiguous()


def abs_gradients(qkv, go, scale):
    """(dQabs, dKabs), each (B, T, H, 64) float64: dPabs = |dO| |V|^T, dSabs = P (dPabs + sum_k P dPabs) scale, dQabs = dSabs |K|,
    dKabs = dSabs^T |Q|."""
    B, T, _, H, D = qkv.shape
    q, k, v = _t(qkv, torch.float64).permute(2, 0, 3, 1, 4)
    g = _t(go, torch.float64).reshape(B, T, H, D).transpose(1, 2)
    p = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
    dp = g.abs() @ v.abs().transpose(-2, -1)
    ds = p * (dp + (p * dp).sum(-1, keepdim=True)) * scale
    return (ds @ k.abs()).transpose(1, 2).contiguous(), (ds.transpose(-2, -1) @ q.abs()).transpose(1, 2).contiguous()


# ---------------------------------------------------------------- errors and bars
def _pair(diff, norm):
    return float(diff.norm() / norm.norm()), float(diff.abs().max() / norm.abs().max())


def errors(got, ref64, absg):
    """{tensor: (relative L2, max-abs over max-abs)} of got = (out, lse, grad_qkv) against ref64 = the same from reference(float64).
    out and dv are normalised by the reference tensor, dq and dk by absg = abs_gradients(...), lse elementwise by max(1, |lse|)
    (its "L2" is the root mean square of those elementwise errors)."""
    out, lse, g = (_t(x, torch.float64) for x in got)
    rout, rlse, rg = ref64
    e = (lse - rlse).abs() / rlse.abs().clamp_min(1.0)
    return {"out": _pair(out - rout, rout),
            "lse": (float(e.square().mean().sqrt()), float(e.max())),
            "dq": _pair(g[:, :, 0] - rg[:, :, 0], absg[0]),
            "dk": _pair(g[:, :, 1] - rg[:, :, 1], absg[1]),
            "dv": _pair(g[:, :, 2] - rg[:, :, 2], rg[:, :, 2])}


def bar(E32, max_abs_lse):
    """The bars for errors(...) of a fused fp32 kernel, from the yardstick's errors on the same inputs (derivation: module docstring)."""
    extra = 4 * U * max(1.0, float(max_abs_lse))
    return {n: tuple(4 * e + (8 * U if n == "lse" else extra) for e in E32[n]) for n in TENSORS}


def bar_bf16(E_yard, E32_lse, max_abs_lse):
    """The bars for errors(...) of the bf16-operand kernels against reference(rounded(qkv), rounded(go), scale): out, dq, dk, dv from
    E_yard = errors(yardstick_bf16(...), ...), lse from E32_lse = errors(float32 reference on the rounded operands, ...)["lse"]
    (derivation: module docstring)."""
    extra = 4 * U * max(1.0, float(max_abs_lse))
    return {n: tuple(4 * e + 8 * U for e in E32_lse) if n == "lse" else tuple(4 * e + extra for e in E_yard[n]) for n in TENSORS}


def ratios(E, bars):
    """{tensor: (L2 error / its bar, max-abs error / its bar)}."""
    return {n: tuple(e / b for e, b in zip(E[n], bars[n])) for n in TENSORS}


def worst(r):
    return max(max(v) for v in r.values())


class Case:
    """Inputs with everything the bars need, computed once: the float64 reference, the float32 yardstick's errors, the bars."""

    def __init__(self, kind, B, T, H, scale, seed=0):
        self.kind, self.shape, self.scale = kind, (B, T, H), scale
        self.qkv, self.go = make_inputs(kind, B, T, H, seed)
        self.ref64 = reference(self.qkv, self.go, scale, torch.float64)
        self.absg = abs_gradients(self.qkv, self.go, scale)
        self.max_lse = float(self.ref64[1].abs().max())
        self.E32 = errors(reference(self.qkv, self.go, scale, torch.float32), self.ref64, self.absg)
        self.bars = bar(self.E32, self.max_lse)

    def ratios(self, got):
        """(ratios to the bars, errors) of got = (out, lse, grad_qkv)."""
        E = errors(got, self.ref64, self.absg)
        return ratios(E, self.bars), E


class CaseBf16:
    """Case for the bf16-operand kernels.  qkv, go: the unrounded float32 inputs (what the kernels are given); ref64 and absg: float64 on
    the rounded operands; E_yard: the bf16 yardstick's errors; E32: the float32 reference's (on the rounded operands); E_bar: the errors
    the bars are built from (E_yard with E32's lse), which is what format_row prints beside the measured ones."""

    def __init__(self, kind, B, T, H, scale, seed=0):
        self.kind, self.shape, self.scale = kind, (B, T, H), scale
        self.qkv, self.go = make_inputs(kind, B, T, H, seed)
        rq, rg = rounded(self.qkv), rounded(self.go)
        self.ref64 = reference(rq, rg, scale, torch.float64)
        self.absg = abs_gradients(rq, rg, scale)
        self.max_lse = float(self.ref64[1].abs().max())
        self.E_yard = errors(yardstick_bf16(self.qkv, self.go, scale), self.ref64, self.absg)
        self.E32 = errors(reference(rq, rg, scale, torch.float32), self.ref64, self.absg)
        self.E_bar = dict(self.E_yard, lse=self.E32["lse"])
        self.bars = bar_bf16(self.E_yard, self.E32["lse"], self.max_lse)

    def ratios(self, got):
        """(ratios to the bars, errors) of got = (out, lse, grad_qkv)."""
        E = errors(got, self.ref64, self.absg)
        return ratios(E, self.bars), E


def format_row(label, E32, E, r):
    """One line of profiles/attn_fp32_accuracy.txt: per tensor the yardstick's error, the measured error and its ratio to the bar
    (the max-abs figures; the L2 ones are smaller throughout)."""
    return label + "".join(f" | {n} {E32[n][1]:.1e} {E[n][1]:.1e} {max(r[n]):.2f}" for n in TENSORS)


# ---------------------------------------------------------------- the kernels' arithmetic in numpy fp32
FAULTS = ("drop_last_key", "extra_zero_key", "delta_of_next_head", "p_bf16", "qk_10_bits", "ds_without_scale", "dv_misses_a_tile",
          "lse_of_next_query")
FAULTS_BF16 = ("drop_last_key", "extra_zero_key", "delta_of_next_head", "dv_misses_a_tile", "lse_of_next_query",
               "operands_truncated", "scale_folded_into_q", "rowsum_of_rounded_p")


def _bf16(a):
    """round-to-nearest-even to 8 mantissa bits, as float32"""
    b = np.ascontiguousarray(a, F32).view(np.uint32)
    return ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F32)


def _trunc16(a):
    """truncation to 8 mantissa bits (bf16 by dropping the low half), as float32"""
    return (np.ascontiguousarray(a, F32).view(np.uint32) & 0xFFFF0000).view(F32)


def _trunc10(a):
    """truncation to 10 mantissa bits (xf32 / tf32 operand), as float32"""
    return (np.ascontiguousarray(a, F32).view(np.uint32) & 0xFFFFE000).view(F32)


def _tree(parts, merge):
    """The fixed pairwise tree of the kernels over the groups' partial results: 0<-1, 2<-3, ..., then 0<-2, ..."""
    parts, s = list(parts), 1
    while s < len(parts):
        for g in range(0, len(parts) - s, 2 * s):
            parts[g] = merge(parts[g], parts[g + s])
        s *= 2
    return parts[0]


def _merge_mlo(a, b):
    (m0, l0, o0), (m1, l1, o1) = a, b
    mt = np.maximum(m0, m1)
    with np.errstate(invalid="ignore"):
        a0 = np.where(np.isneginf(m0), F32(0), np.exp2(m0 - mt)).astype(F32)
        a1 = np.where(np.isneginf(m1), F32(0), np.exp2(m1 - mt)).astype(F32)
    return mt, l0 * a0 + l1 * a1, o0 * a0[..., None] + o1 * a1[..., None]


def emulate(qkv, go, scale, split=1, fault=None, bwd_split=None):
    """The fp32 kernels step by step in numpy float32, per (batch, head) slice: 32-key tiles, the exp2 domain with sl2 = scale * log2e
    folded into Q, running maximum and rescale, the pairwise (m, l, O) merge of `split` key groups, lse = (m + log2 l) * LN2, delta =
    rowsum(O * dO), the backward's P = exp2(S' - lse * LOG2E) with K scaled for dK / dV and Q scaled for dQ, the gradient tiles summed
    per group and then in the same tree.  What it does not model: the order of the sums inside one 32 x 32 x 64 product (numpy's BLAS
    stands in for the MFMA k-chain) and v_exp_f32 / v_log_f32 (numpy's exp2 / log2, correctly rounded, stand in).
    `bwd_split`: the query / key groups of the backward where they differ from the forward's key groups (the automatic choice).
    `fault` (one of FAULTS) plants one defect, for tests/test_attn_fp32_host.py to show that the bars reject it.
    Returns out, lse, grad_qkv as float32 arrays."""
    assert fault is None or fault in FAULTS, fault
    return _emulate(qkv, go, scale, split, fault, bwd_split, False)


def emulate_bf16(qkv, go, scale, split=1, fault=None, bwd_split=None):
    """The bf16-operand kernels in the same tile loop, with their precision contract: Q, K, V and dO rounded to bf16 (the products of
    such operands are exact in fp32, the sums are fp32), sl2 applied to the fp32 score, m / l / lse from the unrounded exponentials, P
    rounded as the operand of P V and P^T dO, dS = P (dP - delta) scale formed in fp32 from the unrounded P and rounded as the operand of
    dS^T Q and dS K, delta = rowsum(O * bf16(dO)).  `fault` (one of FAULTS_BF16): the structural faults of emulate, or a breach of the
    contract: "operands_truncated" (Q, K, V, dO cut to bf16 instead of rounded to nearest even), "scale_folded_into_q" (sl2 multiplied
    into Q -- K in the dK / dV pass -- before the rounding), "rowsum_of_rounded_p" (l sums the bf16 P).
    Returns out, lse, grad_qkv as float32 arrays."""
    assert fault is None or fault in FAULTS_BF16, fault
    return _emulate(qkv, go, scale, split, fault, bwd_split, True)


def _emulate(qkv, go, scale, split, fault, bwd_split, bf16):
    B, T, _, H, D = qkv.shape
    x = np.ascontiguousarray(qkv, F32).transpose(2, 0, 3, 1, 4)        # (3, B, H, T, D)
    q, k, v = x[0], x[1], x[2]
    g = np.ascontiguousarray(go, F32).reshape(B, T, H, D).transpose(0, 2, 1, 3)
    scale = F32(scale)
    sl2 = scale * LOG2E
    same = lambda a: a
    # qs, ks: the score operands where sl2 is folded in (Q in the forward and dQ, K in dK / dV); qs_src, ks_src: the other operand;
    # score(a, b^T): the scores in the exp2 domain
    if bf16:
        cut = _trunc16 if fault == "operands_truncated" else _bf16
        q, k, v, g = cut(q), cut(k), cut(v), cut(g)
        qs_src, ks_src = q, k
        if fault == "scale_folded_into_q":
            qs, ks, score = _bf16(q * sl2), _bf16(k * sl2), (lambda a, bt: a @ bt)
        else:
            qs, ks, score = q, k, (lambda a, bt: (a @ bt) * sl2)
        round_p = round_ds = _bf16                                       # as MFMA operands only
        p_of_ds = same                                                   # dS is formed from the unrounded P
        p_of_l = _bf16 if fault == "rowsum_of_rounded_p" else same
    else:
        qs_src, ks_src = (_trunc10(q), _trunc10(k)) if fault == "qk_10_bits" else (q, k)
        qs, ks, score = qs_src * sl2, ks_src * sl2, (lambda a, bt: a @ bt)
        round_p = _bf16 if fault == "p_bf16" else same
        round_ds, p_of_ds, p_of_l = same, round_p, same
    tiles = [(t0, min(t0 + 32, T)) for t0 in range(0, T, 32)]
    t_keys = T - 1 if fault == "drop_last_key" and T > 1 else T          # the forward's key mask

    # forward
    parts = []
    for grp in range(split):
        m = np.full((B, H, T), -np.inf, F32)
        l = np.zeros((B, H, T), F32)
        o = np.zeros((B, H, T, D), F32)
        for t0, t1 in tiles[grp::split]:
            kt, vt = ks_src[:, :, t0:min(t1, t_keys)], v[:, :, t0:min(t1, t_keys)]
            if fault == "extra_zero_key" and t1 == T:                    # the zero row that the tile holds past T, unmasked
                kt = np.concatenate([kt, np.zeros_like(kt[:, :, :1])], 2)
                vt = np.concatenate([vt, np.zeros_like(vt[:, :, :1])], 2)
            if kt.shape[2] == 0:
                continue
            s = score(qs, kt.transpose(0, 1, 3, 2))
            m_new = np.maximum(m, s.max(-1))
            p = np.exp2(s - m_new[..., None])
            alpha = np.exp2(m - m_new)
            l = l * alpha + p_of_l(p).sum(-1, dtype=F32)
            o = o * alpha[..., None] + round_p(p) @ vt
            m = m_new
        parts.append((m, l, o))
    m, l, o = _tree(parts, _merge_mlo)
    out = o * (F32(1) / l)[..., None]
    lse = (m + np.log2(l)) * LN2

    # backward
    split = split if bwd_split is None else bwd_split
    delta = (out * g).sum(-1, dtype=F32)
    if fault == "delta_of_next_head":
        delta = np.roll(delta, -1, axis=1)
    lse2 = lse * LOG2E
    if fault == "lse_of_next_query":
        lse2 = np.roll(lse2, -1, axis=2)
    ds_scale = F32(1) if fault == "ds_without_scale" else scale

    def p_ds(s, rows, cols):
        p = np.exp2(s - lse2[:, :, rows, None])
        dp = g[:, :, rows] @ v[:, :, cols].transpose(0, 1, 3, 2)
        return round_p(p), round_ds(p_of_ds(p) * (dp - delta[:, :, rows, None]) * ds_scale)

    add = lambda a, b: tuple(x + y for x, y in zip(a, b))
    every = slice(0, T)
    parts = []                                                              # dK, dV: groups of query tiles
    for grp in range(split):
        dv, dk = np.zeros((B, H, T, D), F32), np.zeros((B, H, T, D), F32)
        for t0, t1 in tiles[grp::split]:
            rows = slice(t0, t1)
            p, ds = p_ds(score(qs_src[:, :, rows], ks.transpose(0, 1, 3, 2)), rows, every)
            if not (fault == "dv_misses_a_tile" and t1 == T):
                dv = dv + p.transpose(0, 1, 3, 2) @ g[:, :, rows]
            dk = dk + ds.transpose(0, 1, 3, 2) @ q[:, :, rows]
        parts.append((dv, dk))
    dv, dk = _tree(parts, add)
    parts = []                                                              # dQ: groups of key tiles
    for grp in range(split):
        dq = np.zeros((B, H, T, D), F32)
        for t0, t1 in tiles[grp::split]:
            cols = slice(t0, t1)
            _, ds = p_ds(score(qs, ks_src[:, :, cols].transpose(0, 1, 3, 2)), every, cols)
            dq = dq + ds @ k[:, :, cols]
        parts.append((dq,))
    dq, = _tree(parts, add)
    grad = np.stack([dq, dk, dv], 0).transpose(1, 3, 0, 2, 4)                # (B, T, 3, H, D)
    return (np.ascontiguousarray(out.transpose(0, 2, 1, 3)).reshape(B, T, H * D), np.ascontiguousarray(lse),
            np.ascontiguousarray(grad))
