"""A numpy model of the split attention kernels (csrc/ftx_attn.hip: AttnSplit; ftx_attn_fwd_split / ftx_attn_bwd_split), so that the fp32
bars of tests/attn_ref.py can be exercised on the three-piece scheme without a GPU.  It is not a reference: nothing is ever compared
against it.  The kernels are held to attn_ref.Case(...).bars, the bars of the fp32 kernels, unchanged (tests/test_attn_split_gpu.py).

emulate_split is the tile loop of attn_ref._emulate -- 32-key tiles, the exp2 domain, running maximum and rescale, the pairwise
(m, l, O) merge of the key groups, lse = (m + log2 l) * LN2, delta = rowsum(O * dO), P rebuilt from lse, the gradient tiles summed per
group and then in the same tree -- with the precision contract of include/ftx.h in place of the fp32 products:

* every operand of a product is split into h = bf16(x), m = bf16(x - h), l = bf16((x - h) - m) (tests/split_ref.py): Q, K, V and dO,
  and P and dS where they are operands;
* a product is the six piece products mm, hl, lh, hm, mh, hh, each an fp32 matmul of bf16-valued operands (its products are exact in
  fp32), hh in one fp32 accumulator and the five corrections, smallest first, in another, added once per tile product;
* scale * log2(e) multiplies the fp32 score; dO is exact, in delta too; the softmax statistics are fp32.

What it does not model: the order of the sums inside one piece product (numpy's BLAS stands in for the MFMA k-chain) and v_exp_f32 /
v_log_f32, as attn_ref.emulate."""
import numpy as np

from tests.attn_ref import F32, LN2, LOG2E, _bf16, _merge_mlo, _tree

SIX = ("mm", "hl", "lh", "hm", "mh", "hh")          # tests/split_ref.py
FAULTS = {"five_products": "mm is left out of every product",
          "three_products": "only hm, mh and hh are summed",
          "p_one_piece": "P enters P V and P^T dO as bf16(P) alone",
          "ds_one_piece": "dS enters dS K and dS^T Q as bf16(dS) alone",
          "do_rounded": "dO is rounded to bf16, in delta too"}


def split3(x):
    """fp32 array -> (h, m, l), fp32 arrays of bf16 values: ftx::split1 elementwise (h not finite: m = l = 0)."""
    x = np.ascontiguousarray(x, F32)
    h = _bf16(x)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isfinite(h), x - h, F32(0)).astype(F32)
    m = _bf16(r)
    return h, m, _bf16(r - m)


def product(a, b, names=SIX, a_one_piece=False):
    """a @ b (batched) from the named piece products: hh in one fp32 accumulator, the others in a second, added at the end."""
    pa = dict(zip("hml", split3(a)))
    pb = dict(zip("hml", split3(b)))
    if a_one_piece:
        pa["m"] = pa["l"] = np.zeros_like(pa["h"])
    corr = None
    for n in names:
        if n != "hh":
            part = pa[n[0]] @ pb[n[1]]
            corr = part if corr is None else corr + part
    main = pa["h"] @ pb["h"]
    return main if corr is None else main + corr


def emulate_split(qkv, go, scale, split=1, fault=None, bwd_split=None):
    """out (B, T, H * 64), lse (B, H, T), grad_qkv (B, T, 3, H, 64) as float32 arrays.  `split`: the key groups of the forward, and of the
    backward's query / key groups unless `bwd_split` names those.  `fault` (a key of FAULTS) plants one breach of the contract, for
    tests/test_attn_split_host.py to show that the bars reject it."""
    assert fault is None or fault in FAULTS, fault
    B, T, _, H, D = qkv.shape
    x = np.ascontiguousarray(qkv, F32).transpose(2, 0, 3, 1, 4)        # (3, B, H, T, D)
    q, k, v = x[0], x[1], x[2]
    g = np.ascontiguousarray(go, F32).reshape(B, T, H, D).transpose(0, 2, 1, 3)
    if fault == "do_rounded":
        g = _bf16(g)
    scale = F32(scale)
    sl2 = scale * LOG2E
    names = {"five_products": SIX[1:], "three_products": SIX[3:]}.get(fault, SIX)
    prod = lambda a, b, one=False: product(a, b, names, one)
    tr = lambda a: a.transpose(0, 1, 3, 2)
    p_one, ds_one = fault == "p_one_piece", fault == "ds_one_piece"
    tiles = [(t0, min(t0 + 32, T)) for t0 in range(0, T, 32)]

    # forward
    parts = []
    for grp in range(split):
        m = np.full((B, H, T), -np.inf, F32)
        l = np.zeros((B, H, T), F32)
        o = np.zeros((B, H, T, D), F32)
        for t0, t1 in tiles[grp::split]:
            s = prod(q, tr(k[:, :, t0:t1])) * sl2
            m_new = np.maximum(m, s.max(-1))
            p = np.exp2(s - m_new[..., None])
            alpha = np.exp2(m - m_new)
            l = l * alpha + p.sum(-1, dtype=F32)
            o = o * alpha[..., None] + prod(p, v[:, :, t0:t1], p_one)
            m = m_new
        parts.append((m, l, o))
    m, l, o = _tree(parts, _merge_mlo)
    out = o * (F32(1) / l)[..., None]
    lse = (m + np.log2(l)) * LN2

    # backward
    split = split if bwd_split is None else bwd_split
    delta = (out * g).sum(-1, dtype=F32)
    lse2 = lse * LOG2E

    def p_ds(s, rows, cols):
        p = np.exp2(s - lse2[:, :, rows, None])
        dp = prod(g[:, :, rows], tr(v[:, :, cols]))
        return p, p * (dp - delta[:, :, rows, None]) * scale

    add = lambda a, b: tuple(x + y for x, y in zip(a, b))
    every = slice(0, T)
    parts = []                                                              # dK, dV: groups of query tiles
    for grp in range(split):
        dv, dk = np.zeros((B, H, T, D), F32), np.zeros((B, H, T, D), F32)
        for t0, t1 in tiles[grp::split]:
            rows = slice(t0, t1)
            p, ds = p_ds(prod(q[:, :, rows], tr(k)) * sl2, rows, every)
            dv = dv + prod(tr(p), g[:, :, rows], p_one)
            dk = dk + prod(tr(ds), q[:, :, rows], ds_one)
        parts.append((dv, dk))
    dv, dk = _tree(parts, add)
    parts = []                                                              # dQ: groups of key tiles
    for grp in range(split):
        dq = np.zeros((B, H, T, D), F32)
        for t0, t1 in tiles[grp::split]:
            cols = slice(t0, t1)
            _, ds = p_ds(prod(q, tr(k[:, :, cols])) * sl2, every, cols)
            dq = dq + prod(ds, k[:, :, cols], ds_one)
        parts.append((dq,))
    dq, = _tree(parts, add)
    grad = np.stack([dq, dk, dv], 0).transpose(1, 3, 0, 2, 4)                # (B, T, 3, H, D)
    return (np.ascontiguousarray(out.transpose(0, 2, 1, 3)).reshape(B, T, H * D), np.ascontiguousarray(lse),
            np.ascontiguousarray(grad))
