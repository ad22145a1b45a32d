"""Which tile shape each sparse-convolution launch reaches (tests/test_spconv_regimes.py, tests/test_spconv_regimes_gpu.py).

The pair GEMM (ftx_spconv_pairs_gemm, _scatter, ftx_rows_gemm), the reduce and the weight gradient (ftx_spconv_pairs_wgrad) of
csrc/ftx_spconv.hip pick their tiles from the sizes of their arguments (the rules: csrc/ftx_spconv_common.h).  This module restates those choices in Python, checked
against the library's own host queries (ftx_spconv_gemm_block_cols, ftx_spconv_pairs_wgrad_workspace_bytes,
ftx_spconv_wgrad_resident_blocks), and holds the table of production layers that the GPU tests run at full size."""
from __future__ import annotations

# bench.py's first resident batch, make_batch([0, 1, 2, 3]): voxels per level and pairs of the 3x3x3 submanifold map of the level
# (the strided 2x2x2 map from level s to 2s has one pair per voxel of level s)
BENCH_VOXELS = {1: 81237, 2: 43016, 4: 20197, 8: 8102, 16: 2949}
BENCH_SUBM_PAIRS = {1: 382735, 2: 219664, 4: 126675, 8: 56976, 16: 20329}
DENSE_ROWS = 81237

# Production layers at full size, each run forward, data gradient and weight gradient on the pair-list kernels.
#   map:  ("subm", level) = 3x3x3 submanifold map of the level (kvol 27), ("down", level) = 2x2x2 strided map level -> 2 level (kvol 8)
#   form: "conv" = pair GEMM + reduce; "deconv" = the transposed conv on a strided map (forward in the scatter form);
#         "down_dgrad" = the strided conv whose data gradient is the scatter form (w_transposed)
#   fwd / dgrad: columns per pair-GEMM block of the forward / data gradient; wgrad: (MI, WMG, NI, WNG), pairs per tile, reduce lanes TL
# Entries marked production=False use the production map with channels the model does not run, to reach the scatter form at 128
# columns (no production scatter launch has enough row tiles for it).
PRODUCTION = [
    dict(name="stem 4->32 L1", map=("subm", 1), form="conv", ca=4, co=32, n_pairs=382735, production=True,
         fwd=32, dgrad=32, wgrad=((1, 1, 1, 1), 256, 16)),
    dict(name="128->96 L1", map=("subm", 1), form="conv", ca=128, co=96, n_pairs=382735, production=True,
         fwd=96, dgrad=128, wgrad=((2, 2, 3, 1), 832, 16)),
    dict(name="192->128 L4", map=("subm", 4), form="conv", ca=192, co=128, n_pairs=126675, production=True,
         fwd=128, dgrad=96, wgrad=((3, 1, 2, 2), 576, 16)),
    dict(name="64->128 L8", map=("subm", 8), form="conv", ca=64, co=128, n_pairs=56976, production=True,
         fwd=128, dgrad=64, wgrad=((2, 1, 2, 2), 256, 16)),
    dict(name="128->128 L8", map=("subm", 8), form="conv", ca=128, co=128, n_pairs=56976, production=True,
         fwd=128, dgrad=128, wgrad=((2, 2, 2, 2), 256, 16)),
    dict(name="384->256 L8", map=("subm", 8), form="conv", ca=384, co=256, n_pairs=56976, production=True,
         fwd=128, dgrad=128, wgrad=((2, 2, 2, 2), 896, 4)),
    dict(name="deconv 96->96 L2->L1", map=("down", 1), form="deconv", ca=96, co=96, n_pairs=81237, production=True,
         fwd=96, dgrad=96, wgrad=((2, 2, 3, 1), 256, 16)),
    dict(name="down 128->128 L1->L2 (scatter dgrad)", map=("down", 1), form="down_dgrad", ca=128, co=128, n_pairs=81237, production=False,
         fwd=128, dgrad=128, wgrad=((2, 2, 2, 2), 256, 16)),
]

# Dense rows (functional.linear): forward (ca -> co, with bias), input gradient (co -> ca, W as stored), weight gradient in dense mode
# (A = grad_out, G = x, kvol = 1).
DENSE = [
    dict(name="linear 32->256", ca=32, co=256, rows=DENSE_ROWS, fwd=128, dgrad=32, wgrad=((2, 2, 1, 1), 256, 16)),
    dict(name="linear 96->20", ca=96, co=20, rows=DENSE_ROWS, fwd=32, dgrad=96, wgrad=((1, 1, 3, 1), 256, 16)),
]

# One channel count per M / N side of the weight-gradient tile: (MI, WMG) = (1,1), (2,1), (3,1), (2,2); channel counts that are not
# multiples of 32 put tiles partly outside the matrix
WGRAD_SIDES = {(1, 1): (20, 32), (2, 1): (36, 64), (3, 1): (96, 192), (2, 2): (100, 132)}


def cdiv(a, b):
    return -(-a // b)


def gemm_nt(co, row_tiles):
    """csrc/ftx_spconv_common.h spconv_gemm_nt(): 32-column tiles per block."""
    nt = 4 if co >= 128 else (co + 31) // 32
    if co > 128 and co % 96 == 0 and co % 128 != 0:
        nt = 3
    if nt == 4 and row_tiles * cdiv(co, 128) <= 400:
        nt = 2
    return nt


def block_cols(co, n_pairs, kvol):
    """Columns per block of a pair-list launch (kvol >= 1) or of ftx_rows_gemm (kvol = 0)."""
    return 32 * gemm_nt(co, cdiv(n_pairs, 128) + kvol)


def wgrad_config(ca, cg):
    """csrc/ftx_spconv_common.h spconv_wgrad_config(): (MI, WMG, NI, WNG) of pairs_wgrad_kernel<MI, NI, WMG, WNG>."""
    def side(c):
        if c <= 32:
            return (1, 1)
        if c <= 64:
            return (2, 1)
        if c % 96 == 0 and c % 128 != 0:
            return (3, 1)
        return (2, 2)
    m, n = side(ca), side(cg)
    if m == (3, 1) and n == (3, 1):
        m = (2, 2)
    return m + n


def wgrad_tile_len(lib, n_pairs, ca, cg, kvol):
    """csrc/ftx_spconv_common.h spconv_wgrad_tile_len<SpconvF32>(): pairs per weight-gradient tile."""
    mi, wmg, ni, wng = wgrad_config(ca, cg)
    mn_tiles = cdiv(ca, 32 * mi * wmg) * cdiv(cg, 32 * ni * wng)
    slots = 256 * int(lib.ftx_spconv_wgrad_resident_blocks(ca, cg))
    length = 256
    for rounds in range(1, 65):
        tiles = max((slots * rounds * 15 // 16) // mn_tiles - (kvol + 1) // 2, 1)
        length = cdiv(cdiv(n_pairs, tiles), 64) * 64
        if length <= 4096:
            break
    return max(length, 256)


def wgrad_reduce_lanes(tiles, kvol):
    """csrc/ftx_spconv_common.h launch_wgrad_reduce(): lanes TL of the ordered reduce over `tiles` partial tiles (either precision)."""
    big = 6 * tiles // kvol if kvol > 1 else tiles
    return 1 if big <= 4 else 4 if big <= 32 else 16


def wgrad_regime(lib, n_pairs, ca, cg, kvol):
    """(instantiation, tile length, reduce lanes TL) of one ftx_spconv_pairs_wgrad call.  The tile count comes from the library's
    workspace query (bytes / (4 ca cg) = ceil(P / tile_len) + kvol), so the restated tile length is checked against the library."""
    length = wgrad_tile_len(lib, n_pairs, ca, cg, kvol)
    tiles = int(lib.ftx_spconv_pairs_wgrad_workspace_bytes(n_pairs, ca, cg, kvol)) // (4 * ca * cg)
    assert tiles == cdiv(n_pairs, length) + kvol, (n_pairs, ca, cg, kvol, tiles, length)
    return wgrad_config(ca, cg), length, wgrad_reduce_lanes(tiles, kvol)


# Offset sizes of the tile-edge pair lists, per kvol: "L" stands for the weight-gradient tile length, "L-1" / "L+1" next to it,
# "150L" for 150 tiles and one pair (TL = 16 with kvol 27).  Empty first, last and middle offsets; one-tile offsets (written
# straight to dW[k]) and two-tile ones (reduced); 1, 31, 32, 33, 127, 128 and 129 pairs around the 32-pair steps and 128-pair
# GEMM tiles.  kvol 27 and 8 are the reduce's unrolled instantiations, 5 its generic loop.
EDGE_SIZES = {
    27: [0, 1, 31, 32, 33, 127, 128, 129, "L-1", "L", "L+1", 0, "150L", 5, 8, 11, 14, 17, 20, 23, 26, 29, 32, 35, 38, 41, 0],
    8: [0, 1, "L-1", "L", "L+1", "40L", 129, 0],
    5: [0, 31, "L", "L+1", 0],
}


def edge_sizes(lib, ca, cg, kvol, tile_len=None):
    """EDGE_SIZES[kvol] with L resolved.  The tile length depends on the total pair count, so it is iterated to a fixed point.
    tile_len: the precision's tile-length function (default: wgrad_tile_len, the fp32 kernels').  Returns (sizes, tile_len)."""
    tile_len = tile_len or wgrad_tile_len
    def resolve(v, length):
        if isinstance(v, int):
            return v
        if v == "L":
            return length
        if v.endswith("L"):
            return int(v[:-1]) * length + 1
        return length + int(v[1:])
    length = 256
    for _ in range(20):
        sizes = [resolve(v, length) for v in EDGE_SIZES[kvol]]
        new = tile_len(lib, sum(sizes), ca, cg, kvol)
        if new == length:
            return sizes, length
        length = new
    raise AssertionError("tile-edge sizes did not settle")
