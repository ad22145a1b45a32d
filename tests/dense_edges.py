"""Edge cases of the dense MFMA GEMM families (ftx_dense_gemm_*, ftx_dense_wgrad_*, ftx_vit_patch_embed_*, ftx_vit_tap_stem_*;
csrc/ftx_dense_common.h): the case lists, the float64 references, the gates and the planted faults, for any device.  Used by
tests/test_dense_edges_host.py (CPU) and tests/test_dense_edges_gpu.py.

The value tests of the families (tests/test_vit_linear_bf16_gpu.py, tests/test_vit_linear_split_gpu.py) run at the workload's shapes;
the guard-band tests visit the edges and check no value.  The lists here put a VALUE check on every place where dense_gemm_kernel and
dense_wgrad_kernel decide something from the shape:

  GEMM_CASES    the last row tile holds 1, 31, 32, 33, 63 or 64 rows (and 65, 95, 96, 97, 127 at the 128-row tile) at each of the three
                tiles: the sub-tile borders of the wave split wm * 32 MI + 32 i + l31 and the clamp r < M ? r : M - 1; the last column
                tile holds 4, 36 or 68 columns (36 and 68 cross a 32-column sub-tile; with W stored [K][N] the clamp n + 4 <= N ? n : N - 4);
                k = 64 (one staged step of the bf16 family, two of the split family), and 128 and 192 once per tile.
  WGRAD_CASES   every split count 1 .. 8, a last split of 1, 2, 34, 65, 129, 193 and 256 rows (the row-pair zeroing r0 + 2 rp + h >= hi),
                n and k tails on both sides of the 128 tile (gcol / xcol clamp to N - 4 / K - 4), with one and with several splits.
  PATCH_CASES   the patch-embedding form at the three tiles with frame borders inside tiles, t0 = 1 and 2, an output-column tail.
  TAP_CASES     the tap-stem form at the three tiles, t0 = 0, 1, 2, co = 4, 68, 96, 132.

The tile and split rules are mirrored below (gemm_tile, wgrad_splits) to DOCUMENT each case; what the tests assert against is the
library's own host query (ftx_dense_bf16_tile / ftx_dense_split_tile).

Gates.  None is new: the bf16 family's per-element bound chain * 2^-24 * sum |a b| on bf16-rounded operands
(tests/test_vit_linear_bf16_gpu.py), the split family's G1 (6 L + 8) * 2^-24 * sum |a b| on unrounded operands and G2 E <= T / 2
(tests/test_vit_linear_split_gpu.py, tests/split_ref.py), with the chains k + 2 and ceil(m / splits) + 64 + splits and the GELU terms
as those files write them.  At k = 64 the bounds are about fifty times tighter than at the workload's k.  Two epilogues those files do
not meet get the same treatment: the patch embedding adds pos behind the bias (one more rounding of a value that |pos| joins; k + 2
still counts every addition), and the tap stem's eval BatchNorm scales the pre-activation's bound by |gamma| / sqrt(var + eps) (ReLU is
1-Lipschitz) and adds 8 * 2^-24 of the magnitudes its five fp32 roundings see (1 / sqrt, x - mean, two products, + beta)."""
import torch

from tests import split_ref as R
from tests.test_vit_linear_bf16_gpu import U, _dgelu64, _gelu64, _r64, passes, worst

FAMILIES = ("bf16", "split")
CUS, GRANULE, DW_TILE = 256, 64, 128      # kDenseCUs, kDenseGranule, kDenseDwTile
TILES = ((64, 64), (64, 128), (128, 128))
G2_MIN_ELEMS = 4096                       # G2 is an rms statistic: asserted from this many output elements on, printed below it


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------- the rules, mirrored (csrc/ftx_dense_common.hip)
def gemm_tile(m, n):
    """dense_gemm_tile: the largest of 128 x 128, 64 x 128, 64 x 64 that still gives 256 blocks; else 64 x 64."""
    for tm, tn in ((128, 128), (64, 128), (64, 64)):
        if cdiv(m, tm) * cdiv(n, tn) >= CUS:
            return tm, tn
    return 64, 64


def wgrad_splits(m, n, k):
    """dense_wgrad_split_len: (splits, split length, rows in the last split)."""
    s = min(cdiv(CUS, cdiv(n, DW_TILE) * cdiv(k, DW_TILE)), min(m // 256, 8))
    s = max(s, 1)
    length = max(cdiv(cdiv(m, s), GRANULE) * GRANULE, GRANULE)
    splits = max(cdiv(m, length), 1)
    return splits, length, m - (splits - 1) * length


def tails(m, n, tile):
    """(rows in the last row tile, columns in the last column tile; a full tile counts as its size, no column tail as 0)."""
    rt = m - (cdiv(m, tile[0]) - 1) * tile[0]
    ct = n % tile[1]
    return rt, ct


# ---------------------------------------------------------------- plain GEMM cases: (m, n, k, tile, row_tail, col_tail)
ROW_TAILS = {(64, 64): (1, 31, 32, 33, 63, 64), (64, 128): (1, 31, 32, 33, 63, 64), (128, 128): (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127)}
# Rows and columns in front of the last tile.  64 x 64: one full tile each way (nothing that small reaches 256 blocks).  64 x 128: 16
# full row tiles and 15 full column tiles, 17 x 16 = 272 blocks >= 256, while 128-row tiles give 9 x 16 = 144 < 256.  128 x 128: 15
# and 15, 16 x 16 = 256 blocks.
FRONT = {(64, 64): (64, 64), (64, 128): (1024, 1920), (128, 128): (1920, 1920)}
# the shapes the rule was checked at by hand when the lists were drawn up: (m, n) -> (tile, row tail, column tail)
CHECKED_SHAPES = {(65, 68): ((64, 64), 1, 4), (129, 132): ((64, 64), 1, 4), (1, 4): ((64, 64), 1, 4),
                  (1025, 1924): ((64, 128), 1, 4), (993, 2052): ((64, 128), 33, 4),
                  (2049, 1924): ((128, 128), 1, 4), (1953, 2052): ((128, 128), 33, 4), (1985, 2052): ((128, 128), 65, 4),
                  (2017, 1988): ((128, 128), 97, 68)}


def _gemm_cases():
    shapes = []
    for tile in TILES:
        fm, fn = FRONT[tile]
        for i, rt in enumerate(ROW_TAILS[tile]):
            wide = 36 if tile[1] == 64 else (36, 68)[i % 2]      # 68 is a tail of 4 at the 64-column tile
            for ct in (4, wide):
                shapes.append((fm + rt, fn + ct, 64))
        shapes.append((fm + tile[0], fn + tile[1], 64))          # no tail either way
        shapes += [(fm + 33, fn + 4, 128), (fm + 33, fn + 4, 192)]   # two and three staged steps (bf16), four and six (split)
    shapes += [(m, n, 64) for m, n in CHECKED_SHAPES]
    out = []
    for m, n, k in dict.fromkeys(shapes):
        tile = gemm_tile(m, n)
        out.append((m, n, k, tile) + tails(m, n, tile))
    return out


GEMM_CASES = _gemm_cases()

# ---------------------------------------------------------------- weight-gradient cases: (m, n, k, splits, rows_in_last_split)
# m -> (splits, rows in the last split) at every n, k of the lists below (one to nine 128 x 128 tiles: the cap m / 256 decides)
WGRAD_ROWS = {1: (1, 1), 2: (1, 2), 31: (1, 31), 33: (1, 33), 63: (1, 63), 65: (1, 65), 300: (1, 300), 512: (2, 256), 513: (2, 193),
              769: (3, 129), 1025: (4, 65), 1281: (5, 1), 1282: (5, 2), 1314: (5, 34), 1601: (6, 1), 2049: (7, 129), 2241: (8, 1),
              2305: (8, 65)}
WGRAD_NK = ((68, 68), (132, 260))                                         # every m
WGRAD_NK_MORE = ((4, 4), (4, 132), (260, 4), (132, 132), (260, 68))       # at WGRAD_M_MORE: unsplit, two splits, eight splits of one row
WGRAD_M_MORE = (33, 513, 2241)
WGRAD_CASES = [(m, n, k) + WGRAD_ROWS[m] for m in WGRAD_ROWS for n, k in WGRAD_NK] + \
              [(m, n, k) + WGRAD_ROWS[m] for m in WGRAD_M_MORE for n, k in WGRAD_NK_MORE]

# ---------------------------------------------------------------- form cases
# Patch embedding: patch 4, 4 channels (k = 64), image side 100: 625 patches per frame, so frame borders fall inside tiles.
# (b, side, dim, t0, tile, row_tail).  dim 768: 6 column tiles of 128; b = 5: 3125 rows, 25 x 6 = 150 < 256 at 128 rows, 49 x 6 = 294
# at 64: 64 x 128, tail 3125 - 48 * 64 = 53.  b = 9: 5625 rows, 44 x 6 = 264: 128 x 128, tail 5625 - 43 * 128 = 121.  b = 1: 64 x 64,
# tail 625 - 9 * 64 = 49.  dim 772 adds a column tail of 4 (7 column tiles; the same tiles follow).
PATCH_P, PATCH_C = 4, 4
PATCH_CASES = [(1, 100, 768, 2, (64, 64), 49), (1, 100, 772, 1, (64, 64), 49), (5, 100, 768, 1, (64, 128), 53), (5, 100, 772, 2, (64, 128), 53),
               (9, 100, 768, 2, (128, 128), 121), (9, 100, 772, 1, (128, 128), 121)]
# Tap stem: dim 64.  (b, g, t0, co, tile, row_tail).  co <= 132 is at most two column tiles, so the wider tiles need many rows:
# co = 132 reaches 64 x 128 from 8129 rows (128 x 2 blocks) and 128 x 128 from 16257; co <= 128 is one column tile and reaches
# 64 x 128 only from 16321 rows and 128 x 128 from 32641 rows.  Every tile is reached: 64 x 64 with every co, 64 x 128 with co = 132
# and co = 96, 128 x 128 with co = 132 alone (co = 96 there would take 32641 rows of tokens: the same kernel and column map as
# 64 x 128, left out for its size).
TAP_DIM = 64
TAP_CASES = [(3, 25, 0, 4, (64, 64), 11), (3, 25, 1, 68, (64, 64), 11), (3, 43, 2, 96, (64, 64), 1), (3, 25, 1, 132, (64, 64), 11),
             (13, 627, 2, 132, (64, 128), 23), (27, 625, 0, 96, (64, 128), 43), (26, 627, 1, 132, (128, 128), 46)]


# ---------------------------------------------------------------- data: the zero-mean distribution of the families' value tests
def data(m, k, n, seed, device="cpu"):
    """x (m, k) ~ N(0, 1), w (n, k) ~ 0.02 N(0, 1), b (n) ~ 0.1 N(0, 1): _data of tests/test_vit_linear_bf16_gpu.py on any device."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(m, k, device=device, generator=g)
    w = torch.randn(n, k, device=device, generator=g) * 0.02
    b = torch.randn(n, device=device, generator=g) * 0.1
    return x, w, b


def randn(shape, seed, device="cpu", scale=1.0):
    return torch.randn(*shape, device=device, generator=torch.Generator(device=device).manual_seed(seed)) * scale


def unfold(img, p):
    """(b, c, h, w) -> (b gh gw, c p p): row (frame, gy, gx), column (c, py, px), the patch embedding's A."""
    b, c, h, w = img.shape
    gh, gw = h // p, w // p
    return img.reshape(b, c, gh, p, gw, p).permute(0, 2, 4, 1, 3, 5).reshape(b * gh * gw, c * p * p).contiguous()


# ---------------------------------------------------------------- references and bounds
def operands64(family, *ts):
    """The float64 operands a family's reference multiplies: bf16-rounded for the bf16 family, as stored for the split family."""
    return tuple(_r64(t) if family == "bf16" else t.double() for t in ts)


def factor(family, chain):
    """The number of 2^-24 units of sum |a b| a family is allowed over an accumulation chain of `chain` additions."""
    return chain + 2 if family == "bf16" else 6 * chain + 8


def wgrad_factor(family, m, splits):
    chain = cdiv(m, splits) + 64 + splits
    return chain if family == "bf16" else 6 * chain + 8


def gemm_ref(family, a, b_kn):
    """(float64 sum, sum |a b|) of a (m, k) @ b_kn (k, n) on the family's reference operands."""
    a64, b64 = operands64(family, a, b_kn)
    return a64 @ b64, a64.abs() @ b64.abs()


def bias_ref(s, sa, bias, f):
    """(reference, bound) of the BIAS epilogue from the NONE epilogue's (s, sa)."""
    b64 = bias.double()
    return s + b64, f * U * (sa + b64.abs())


def gelu_ref(pre_ref, pre_bound, pre):
    """(reference, bound) of BIAS_GELU: gelu of the fp32 pre-activation `pre` (the kernel's own), its error through gelu' plus a few
    ulps of erf in fp32."""
    p64 = pre.double()
    return _gelu64(pre_ref), _dgelu64(pre_ref).abs() * pre_bound + 8 * U * (p64.abs() + _gelu64(p64).abs()) + 1e-30


def dgelu_ref(s, sa, pre_in, f):
    """(reference, bound) of DGELU: the sum times gelu'(pre_in)."""
    p64 = pre_in.double()
    d64 = _dgelu64(p64)
    return s * d64, f * U * sa * d64.abs() + 8 * U * s.abs() * (1 + p64.abs()) + 1e-30


def g2_parts(a, b_kn):
    """(S, S5) of gate G2 (tests/split_ref.py g2_figures), computed once for the outputs that share the operands."""
    return a.double() @ b_kn.double(), R.gemm(a, b_kn, R.FIVE)


def g2_figures(out, parts, add=None):
    """(E, T) = R.g2_figures(out, a, b_kn, add) from g2_parts(a, b_kn)."""
    s, s5 = parts
    if add is not None:
        s, s5 = s + add.double(), s5 + add.double()
    return R.rms(out.double() - s) / R.rms(s), R.rms(s5 - s) / R.rms(s)


def patch_ref(family, img, w, bias, pos, t0, f):
    """Patch rows of the patch embedding, (b g, dim): (reference, bound, A, add) with add the (b g, dim) bias + pos rows."""
    b = img.shape[0]
    a = unfold(img, PATCH_P)
    s, sa = gemm_ref(family, a, w.t())
    add = (bias.double().unsqueeze(0) + pos.double()[t0:]).repeat(b, 1)
    add_abs = (bias.double().abs().unsqueeze(0) + pos.double()[t0:].abs()).repeat(b, 1)
    return s + add, f * U * (sa + add_abs), a, add


def bn64(x, gamma, beta, mean, var, eps):
    return (x - mean.double()) / torch.sqrt(var.double() + eps) * gamma.double() + beta.double()


def tap_ref(family, tokens, w, bias, gamma, beta, mean, var, eps, t0, f, skip=True):
    """The tap stem, (b g, co): BatchNorm(ReLU(tokens[:, t0:] W^T + bias)) in float64 and its bound.  skip=False is fault (h)."""
    b, tg, dim = tokens.shape
    g = tg - t0
    a = (tokens[:, t0:] if skip else tokens[:, :g]).reshape(b * g, dim)
    s, sa = gemm_ref(family, a, w.t())
    pre, pre_bound = bias_ref(s, sa, bias, f)
    x = pre.clamp_min(0)
    scale = gamma.double().abs() / torch.sqrt(var.double() + eps)
    return bn64(x, gamma, beta, mean, var, eps), scale * pre_bound + 8 * U * (scale * (x + mean.double().abs()) + beta.double().abs()) + 1e-30


# ---------------------------------------------------------------- the planted faults
def mutants(kind, **t):
    """float64 references of the faults these edges can hide, name -> reference.  Operands are float64 (operands64).

    kind "gemm"  (a, b_kn, bias, col_tail):  out = a @ b_kn + bias
        c  the last 16-wide k-step is dropped
        d  output row M - 1 holds row M - 2's sums
        f  the bias of the last column tile's tail is read four columns early
    kind "dx"    (a, b_kn):  W stored [K][N], out = a @ b_kn
        c, d as above
        e  columns N-4 .. N-1 hold the sums of columns N-8 .. N-5 (the clamped address n = N - 4 one float4 early)
    kind "wgrad" (g, x, split_len):  dW = g^T x
        a  the last reduction row of the last split is dropped
        b  row `hi` of the next split (the first row behind split 0) is added twice
    kind "patch" (a, b_kn, bias, pos, g, t0):  rows (frame, patch) = a @ b_kn + bias + pos[t0 + patch]
        g  the first patch row of frame 1 takes pos of the row in front of it, the last patch of frame 0
    kind "tap"   (ref_unskipped):  h  the rows do not skip the t0 leading tokens (tap_ref(..., skip=False))"""
    out = {}
    if kind in ("gemm", "dx"):
        a, b_kn = t["a"], t["b_kn"]
        s = a @ b_kn
        add = t["bias"].unsqueeze(0) if kind == "gemm" else 0.0
        k = a.shape[1]
        out["c"] = a[:, :k - 16] @ b_kn[:k - 16] + add
        if a.shape[0] >= 2:
            d = (s + add).clone()
            d[-1] = d[-2]
            out["d"] = d
        n = b_kn.shape[1]
        if kind == "gemm" and t["col_tail"] and n >= 8:
            early = t["bias"].clone()
            early[n - t["col_tail"]:] = t["bias"][n - t["col_tail"] - 4:n - 4]
            out["f"] = s + early.unsqueeze(0)
        if kind == "dx" and n >= 8:
            e = s.clone()
            e[:, n - 4:] = s[:, n - 8:n - 4]
            out["e"] = e
    elif kind == "wgrad":
        g, x, length = t["g"], t["x"], t["split_len"]
        s = g.t() @ x
        out["a"] = s - g[-1].unsqueeze(1) * x[-1].unsqueeze(0)
        if length < g.shape[0]:
            out["b"] = s + g[length].unsqueeze(1) * x[length].unsqueeze(0)
    elif kind == "patch":
        a, b_kn, bias, pos, g, t0 = t["a"], t["b_kn"], t["bias"], t["pos"], t["g"], t["t0"]
        frames = a.shape[0] // g
        ref = a @ b_kn + bias.unsqueeze(0) + pos[t0:].repeat(frames, 1)
        if frames >= 2:
            ref[g] += pos[t0 + g - 1] - pos[t0]
            out["g"] = ref
    elif kind == "tap":
        out["h"] = t["ref_unskipped"]
    else:
        raise ValueError(kind)
    return out


def emulate(family, a, b_kn):
    """What an ideal kernel of the family sums, in float64: the product of the bf16-rounded operands, or the six piece products of
    tests/split_ref.py.  The contract rounds it once to float32 behind the epilogue's additions."""
    return _r64(a) @ _r64(b_kn) if family == "bf16" else R.gemm(a, b_kn, R.SIX)
