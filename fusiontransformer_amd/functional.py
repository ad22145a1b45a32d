"""Host-side operator surface over libftx: the torchsparse `spf.*` functions the
reference calls (models/utils.py:19-27,44-58,71-99), the kernel-map builder and
sparse convolution hidden inside `spnn.Conv3d` (models/spvcnn.py:26-30), the
fused BatchNorm(+residual)(+ReLU), and the fused nearest-upsample + lift gather
of `Net2DBillinear.get_img_feats` (models/image_models_billinear.py:113-124).

Same names and argument meaning as the reference's imports; tensors live on
the GPU, index tensors are int32 (torchsparse returns int64 and immediately
`.int()`s them, utils.py:22,51)."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, req, stream

I32, I64, F32 = torch.int32, torch.int64, torch.float32


def _empty(shape, dtype, like):
    return torch.empty(shape, dtype=dtype, device=like.device)


# Kernel workspaces (BatchNorm / weight-gradient partials, sort and scan temporaries) live in ONE growing buffer per (device, stream):
# a workspace is only touched by the kernels of the call that receives it, and calls on one stream execute in order, so the next
# call may reuse the bytes.  This takes two allocator round trips and a size query through ctypes out of every such call (~150 per
# training step).  While a stream is being captured into a HIP graph the buffer must not be baked in (it can be re-grown later), so
# capture falls back to a fresh allocation from the graph's pool.
_SCRATCH = {}
_WS_BYTES = {}


def _ws_bytes(fn_name, *args):
    key = (fn_name,) + args
    v = _WS_BYTES.get(key)
    if v is None:
        v = _WS_BYTES[key] = int(getattr(_lib.load(), fn_name)(*args))
        if len(_WS_BYTES) > 4096:
            _WS_BYTES.clear()
    return v


def _carve(like, *nbytes):
    """Raw device pointers of consecutive 256-byte aligned regions of the stream's scratch buffer: the temporaries of ONE call
    (pair rows, partial statistics, an intermediate gradient, kernel workspaces) that never leave it."""
    if torch.cuda.is_current_stream_capturing():
        # Under capture `_scratch` hands out a fresh allocation from the graph's private pool; this function returns raw addresses and
        # drops the tensor, so a later allocation of the same capture could be given the same block while kernels recorded earlier
        # still use it.  The callers (the Conv3d + BatchNorm node) also rely on the library's per-stream ticket counters, which must
        # not be baked into a graph that replays beside eager launches.  Neither is supported: fail instead of corrupting data.
        raise RuntimeError("fusiontransformer_amd: the fused Conv3d + BatchNorm node cannot be captured into a HIP graph "
                           "(its temporaries are carved from the stream's scratch buffer); run the LiDAR branch eagerly")
    offs, total = [], 0
    for n in nbytes:
        offs.append(total)
        total += (int(n) + 255) & ~255
    base = _scratch(max(total, 256), like).data_ptr()
    return [base + o for o in offs]


def _scratch(nbytes, like):
    dev = like.device
    if torch.cuda.is_current_stream_capturing():
        return torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    key = (dev.index, stream())
    buf = _SCRATCH.get(key)
    if buf is None or buf.shape[0] < nbytes:
        buf = _SCRATCH[key] = torch.empty((max(int(nbytes * 1.25), 1 << 22),), dtype=torch.uint8, device=dev)
    return buf


# The statistics kernels (BatchNorm, the convolution's reduce-with-statistics pass) keep a few ticket counters per (device, stream)
# (include/ftx.h, ftx_stream_scratch_*).  The caller owns that buffer: it is a torch allocation attached to the stream at its first use.
_TICKETS = {}


def _stream_scratch(st=None):
    """Make sure the current stream has its ticket buffer attached (a dict lookup after the first call); returns the raw stream."""
    if st is None:
        st = stream()
    key = (torch.cuda.current_device(), st)
    if key not in _TICKETS and not torch.cuda.is_current_stream_capturing():
        L = _lib.load()
        n = int(L.ftx_stream_scratch_bytes())
        buf = torch.empty((n,), dtype=torch.uint8, device=torch.device("cuda", key[0]))
        check(L.ftx_stream_scratch_attach(st, buf.data_ptr(), n), "ftx_stream_scratch_attach")
        _TICKETS[key] = buf
    return st


def reset_stream_scratch():
    """Clear the ticket counters of the current stream (after a kernel of the library died mid-flight on it)."""
    check(_lib.load().ftx_stream_scratch_reset(stream()), "ftx_stream_scratch_reset")


def release_stream_scratch():
    """Detach (and free) the ticket buffers of every stream this process attached one to."""
    L = _lib.load()
    for (dev, st) in list(_TICKETS):
        with torch.cuda.device(dev):
            check(L.ftx_stream_scratch_release(st), "ftx_stream_scratch_release")
        del _TICKETS[(dev, st)]


# ---------------------------------------------------------------- integer side
def sphash(coords: torch.Tensor, offsets: torch.Tensor | None = None) -> torch.Tensor:
    """spf.sphash: (N,4) int32 -> (N,) int64, or with (K,3) offsets -> (K,N)."""
    L = _lib.load()
    req(coords, I32, "sphash coords", 2)
    if coords.shape[1] != 4:
        raise ValueError("sphash: coords must be (N,4)")
    n = coords.shape[0]
    if offsets is None:
        out = _empty((n,), I64, coords)
        check(L.ftx_hash(ptr(coords), n, ptr(out), stream()), "ftx_hash")
        return out
    req(offsets, I32, "sphash offsets", 2)
    k = offsets.shape[0]
    out = _empty((k, n), I64, coords)
    check(L.ftx_hash_kernel(ptr(coords), n, ptr(offsets), k, ptr(out), stream()), "ftx_hash_kernel")
    return out


def floor_coords(pc: torch.Tensor, stride: int) -> torch.Tensor:
    """cat([floor(pc[:, :3] / s).int() * s, pc[:, -1].int()]) (models/utils.py:44-48)."""
    L = _lib.load()
    req(pc, F32, "floor_coords pc", 2)
    if pc.shape[1] != 4:
        raise ValueError("floor_coords: pc must be (N,4)")
    out = _empty(pc.shape, I32, pc)
    check(L.ftx_floor_coords(ptr(pc), pc.shape[0], int(stride), ptr(out), stream()), "ftx_floor_coords")
    return out


class HashTable:
    """Open-addressing table (64-bit keys -> int32 row) resident in HBM."""

    def __init__(self, keys: torch.Tensor):
        L = _lib.load()
        req(keys, I64, "HashTable keys", 1)
        self.n = keys.shape[0]
        self.capacity = int(L.ftx_hashtable_capacity(self.n))
        self.keys = _empty((self.capacity,), I64, keys)
        self.vals = _empty((self.capacity,), I32, keys)
        check(L.ftx_hashtable_build(ptr(keys), self.n, ptr(self.keys), ptr(self.vals), self.capacity, stream()), "ftx_hashtable_build")

    def query(self, q: torch.Tensor) -> torch.Tensor:
        L = _lib.load()
        req(q, I64, "HashTable query")
        out = _empty(q.shape, I32, q)
        check(L.ftx_hashtable_query(ptr(q), q.numel(), ptr(self.keys), ptr(self.vals), self.capacity, ptr(out), stream()), "ftx_hashtable_query")
        return out


def sphashquery(hash_query: torch.Tensor, hash_target: torch.Tensor) -> torch.Tensor:
    """spf.sphashquery: row of each query hash in hash_target, -1 if absent (int32)."""
    return HashTable(hash_target).query(hash_query)


def spcount(idx: torch.Tensor, n: int) -> torch.Tensor:
    L = _lib.load()
    req(idx, I32, "spcount idx", 1)
    out = _empty((int(n),), I32, idx)
    check(L.ftx_count(ptr(idx), idx.shape[0], ptr(out), int(n), stream()), "ftx_count")
    return out


def unique_sorted(keys: torch.Tensor):
    """torch.unique(keys) (ascending) plus the row of the first occurrence of each.

    Returns (uniq (n,), first_index (n,), n_unique (1,) int32 ON DEVICE); rows
    past n_unique are unspecified.  No host sync here."""
    L = _lib.load()
    req(keys, I64, "unique_sorted keys", 1)
    n = keys.shape[0]
    uniq = _empty((n,), I64, keys)
    first = _empty((n,), I32, keys)
    cnt = torch.zeros((1,), dtype=I32, device=keys.device)
    ws_bytes = _ws_bytes("ftx_unique_workspace_bytes", n)
    ws = _scratch(ws_bytes, keys)
    check(L.ftx_unique_sorted(ptr(keys), n, ptr(uniq), ptr(first), ptr(cnt), ptr(ws), ws_bytes, stream()), "ftx_unique_sorted")
    return uniq, first, cnt


def levels_unique(points: torch.Tensor, strides):
    """Every U-Net level's voxel set from the floored point coordinates in ONE pass (ftx_levels_unique): for each stride s the sorted
    unique hashes of floor_div(p, s) * s and the point row of each one's first occurrence, back to back, plus `level_off`
    (len(strides) + 1,) int32 ON THE DEVICE -- where each level's run starts.  One sort, no host sync here."""
    L = _lib.load()
    req(points, I32, "levels_unique points", 2)
    if points.shape[1] != 4:
        raise ValueError("levels_unique: points must be (N,4)")
    st = np.ascontiguousarray(np.asarray(strides, dtype=np.int32))
    nl, n = int(st.shape[0]), points.shape[0]
    if not (1 <= nl <= 8) or (st < 1).any():
        raise ValueError("levels_unique: 1..8 strides, each >= 1")
    uniq = _empty((nl * n,), I64, points)
    first = _empty((nl * n,), I32, points)
    level_off = _empty((nl + 1,), I32, points)
    sorted_keys = _empty((nl, n), I64, points)        # row l: level l's (tag | hash) keys, ascending
    order = _empty((nl, n), I32, points)              # row l: the points sorted by their voxel of level l (stable)
    ws_bytes = _ws_bytes("ftx_levels_workspace_bytes", n, nl)
    ws = _scratch(ws_bytes, points)
    check(L.ftx_levels_unique(ptr(points), n, st.ctypes.data, nl, ptr(uniq), ptr(first), ptr(level_off), ptr(sorted_keys), ptr(order), ptr(ws), ws_bytes,
                              stream()), "ftx_levels_unique")
    return uniq, first, level_off, sorted_keys, order


def level_segments(sorted_keys_row: torch.Tensor, order_row: torch.Tensor, hashes: torch.Tensor, level: int) -> "Segments":
    """The sorted segments of spvoxelize at one level from levels_unique's sort (no second sort): == Segments(idx_query, n_vox)."""
    L = _lib.load()
    req(sorted_keys_row, I64, "level_segments sorted keys", 1)
    req(order_row, I32, "level_segments order", 1)
    req(hashes, I64, "level_segments hashes", 1)
    m = hashes.shape[0]
    seg_off = _empty((m + 1,), I32, hashes)
    check(L.ftx_level_segments(ptr(sorted_keys_row), sorted_keys_row.shape[0], ptr(hashes), m, int(level), ptr(seg_off), stream()), "ftx_level_segments")
    return Segments.from_parts(order_row, seg_off, m)


def level_coords(points: torch.Tensor, first_index: torch.Tensor, stride: int) -> torch.Tensor:
    """Coordinates of one level: floor_div(points[first_index], stride) * stride, rows in the level's (hash) order."""
    L = _lib.load()
    req(points, I32, "level_coords points", 2)
    req(first_index, I32, "level_coords first_index", 1)
    out = _empty((first_index.shape[0], 4), I32, points)
    check(L.ftx_level_coords(ptr(points), ptr(first_index), first_index.shape[0], int(stride), ptr(out), stream()), "ftx_level_coords")
    return out


def sorted_rank(sorted_keys: torch.Tensor, n_sorted: torch.Tensor, queries: torch.Tensor) -> torch.Tensor:
    """Position of every query in sorted_keys[:n_sorted] (ascending, unique), -1 when absent; n_sorted is a (1,) int32 DEVICE tensor,
    so `unique_sorted` + `sorted_rank` give numpy.unique(return_index, return_inverse) without a host read."""
    L = _lib.load()
    req(sorted_keys, I64, "sorted_rank sorted", 1)
    req(n_sorted, I32, "sorted_rank n_sorted", 1)
    req(queries, I64, "sorted_rank queries", 1)
    rank = _empty((queries.shape[0],), I32, queries)
    check(L.ftx_sorted_rank(ptr(sorted_keys), ptr(n_sorted), sorted_keys.shape[0], ptr(queries), queries.shape[0], ptr(rank), stream()), "ftx_sorted_rank")
    return rank


def rotate_points(points: torch.Tensor, rot) -> torch.Tensor:
    """points (N,3) float32 @ rot (3,3) float32 (host array) with the rounding of numpy's `points.dot(rot)` (libftx)."""
    L = _lib.load()
    req(points, F32, "rotate_points points", 2)
    if points.shape[1] != 3:
        raise ValueError("rotate_points: points must be (N, 3)")
    r = np.ascontiguousarray(np.asarray(rot, dtype=np.float32).reshape(9))
    out = _empty(tuple(points.shape), F32, points)
    check(L.ftx_rotate_points(ptr(points), points.shape[0], r.ctypes.data_as(ctypes.c_void_p), ptr(out), stream()), "ftx_rotate_points")
    return out


def downsample_coords(coords: torch.Tensor, ratio: int) -> torch.Tensor:
    L = _lib.load()
    req(coords, I32, "downsample coords", 2)
    out = torch.empty_like(coords)
    check(L.ftx_downsample_coords(ptr(coords), coords.shape[0], int(ratio), ptr(out), stream()), "ftx_downsample_coords")
    return out


def gather_coords(src: torch.Tensor, index: torch.Tensor) -> torch.Tensor:
    L = _lib.load()
    req(src, I32, "gather_coords src", 2)
    req(index, I32, "gather_coords index", 1)
    out = _empty((index.shape[0], 4), I32, src)
    check(L.ftx_gather_coords(ptr(src), ptr(index), index.shape[0], ptr(out), stream()), "ftx_gather_coords")
    return out


def kernel_offsets(kernel_size: int, tensor_stride: int = 1) -> np.ndarray:
    """torchsparse KernelRegion(kernel_size, tensor_stride).get_kernel_offset():
    odd kernels enumerate x fastest, even kernels z fastest."""
    single = (np.arange(-kernel_size // 2 + 1, kernel_size // 2 + 1) * tensor_stride).tolist()
    if kernel_size % 2 == 1:
        offs = [[x, y, z] for z in single for y in single for x in single]
    else:
        offs = [[x, y, z] for x in single for y in single for z in single]
    return np.array(offs, dtype=np.int32)


def kernel_map_build(out_coords: torch.Tensor, offsets: torch.Tensor, table: HashTable) -> torch.Tensor:
    """nbr (K, N_out) int32: row of out_coords[o]+offsets[k] among the table's keys, or -1."""
    L = _lib.load()
    req(out_coords, I32, "kernel_map out_coords", 2)
    req(offsets, I32, "kernel_map offsets", 2)
    n_out, k = out_coords.shape[0], offsets.shape[0]
    nbr = _empty((k, n_out), I32, out_coords)
    check(L.ftx_kernel_map_build(ptr(out_coords), n_out, ptr(offsets), k, ptr(table.keys), ptr(table.vals), table.capacity, ptr(nbr), stream()),
          "ftx_kernel_map_build")
    return nbr


def kernel_map_count(nbr: torch.Tensor):
    """Step 1 of the pair list: returns (pos scratch (K,N_out), koff (K+1,) int32 on the device).
    koff[-1] is the number of pairs; the caller reads it back (one host sync) to size the arrays."""
    L = _lib.load()
    req(nbr, I32, "kernel_map_count nbr", 2)
    k, n_out = nbr.shape
    pos = torch.empty_like(nbr)
    koff = _empty((k + 1,), I32, nbr)
    ws_bytes = _ws_bytes("ftx_kernel_map_count_workspace_bytes", n_out, k)
    ws = _scratch(ws_bytes, nbr)
    check(L.ftx_kernel_map_count(ptr(nbr), n_out, k, ptr(pos), ptr(koff), ptr(ws), ws_bytes, stream()), "ftx_kernel_map_count")
    return pos, koff


def kernel_map_pairs(nbr: torch.Tensor, pos: torch.Tensor, n_in: int, n_pairs: int):
    """Step 2: (pos (K,N_out), pos_t (K,N_in), pair_in (P,), pair_out (P,))."""
    L = _lib.load()
    k, n_out = nbr.shape
    pos_t = _empty((k, int(n_in)), I32, nbr)
    pair_in = _empty((int(n_pairs),), I32, nbr)
    pair_out = _empty((int(n_pairs),), I32, nbr)
    check(L.ftx_kernel_map_pairs(ptr(nbr), n_out, int(n_in), k, ptr(pos), ptr(pos_t), ptr(pair_in), ptr(pair_out), int(n_pairs), stream()),
          "ftx_kernel_map_pairs")
    return pos, pos_t, pair_in, pair_out


def calc_ti_weights(pc: torch.Tensor, idx_query: torch.Tensor, scale: int = 1) -> torch.Tensor:
    """spf.calc_ti_weights, already in the point-major (N,8) layout of utils.py:82-83."""
    L = _lib.load()
    req(pc, F32, "calc_ti_weights pc", 2)
    req(idx_query, I32, "calc_ti_weights idx", 2)
    n = pc.shape[0]
    if pc.shape[1] != 4 or idx_query.shape != (n, 8):
        raise ValueError("calc_ti_weights: pc must be (N,4) and idx (N,8)")
    w = _empty((n, 8), F32, pc)
    check(L.ftx_trilinear_weights(ptr(pc), ptr(idx_query), n, int(scale), ptr(w), stream()), "ftx_trilinear_weights")
    return w


# ---------------------------------------------------------------- voxelize / devoxelize
class Segments:
    """Entries sorted by destination row (ftx_segment_build): `order`, `seg_off`, `m` rows."""
    __slots__ = ("order", "seg_off", "m")

    @classmethod
    def from_parts(cls, order, seg_off, m):
        self = cls.__new__(cls)
        self.order, self.seg_off, self.m = order, seg_off, int(m)
        return self

    def __init__(self, keys: torch.Tensor, m: int):
        L = _lib.load()
        keys = req(keys.contiguous().view(-1), I32, "segment keys", 1)
        n = keys.shape[0]
        self.m = int(m)
        self.order = _empty((n,), I32, keys)
        self.seg_off = _empty((self.m + 1,), I32, keys)
        ws_bytes = _ws_bytes("ftx_segment_workspace_bytes", n, self.m)
        ws = _scratch(ws_bytes, keys)
        check(L.ftx_segment_build(ptr(keys), n, self.m, ptr(self.order), ptr(self.seg_off), ptr(ws), ws_bytes, stream()), "ftx_segment_build")


def voxelize_segments(idx: torch.Tensor, m: int) -> Segments:
    """Points sorted by their voxel: makes the scatter-mean of spvoxelize a gather-reduce."""
    return Segments(idx, m)


def devoxelize_segments(idx: torch.Tensor, weights: torch.Tensor, m: int) -> Segments:
    """(point, corner) entries sorted by voxel, zero-weight corners dropped: makes the scatter-add of
    spdevoxelize's backward a gather-reduce."""
    keys = torch.where(weights != 0, idx, torch.full_like(idx, -1))
    return Segments(keys, m)


class _Voxelize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, idx, counts, seg):
        L = _lib.load()
        feats = req(feats.contiguous(), F32, "spvoxelize feats", 2)
        req(idx, I32, "spvoxelize idx", 1)
        req(counts, I32, "spvoxelize counts", 1)
        n, c = feats.shape
        if idx.shape[0] != n:
            raise ValueError("spvoxelize: idx length != rows of feats")
        m = counts.shape[0]
        out = _empty((m, c), F32, feats)
        if seg is not None and c % 4 == 0:
            if seg.m != m or seg.order.shape[0] != n:
                raise ValueError("spvoxelize: segments do not match idx / counts")
            check(L.ftx_voxelize_fwd_sorted(ptr(feats), ptr(seg.order), ptr(seg.seg_off), n, c, m, ptr(out), stream()), "ftx_voxelize_fwd_sorted")
        else:
            check(L.ftx_voxelize_fwd(ptr(feats), ptr(idx), ptr(counts), n, c, m, ptr(out), stream()), "ftx_voxelize_fwd")
        ctx.save_for_backward(idx, counts)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, grad_out):
        L = _lib.load()
        idx, counts = ctx.saved_tensors
        grad_out = req(grad_out.contiguous(), F32, "spvoxelize grad", 2)
        m, c = grad_out.shape
        gf = _empty((ctx.n, c), F32, grad_out)
        check(L.ftx_voxelize_bwd(ptr(grad_out), ptr(idx), ptr(counts), ctx.n, c, m, ptr(gf), stream()), "ftx_voxelize_bwd")
        return gf, None, None, None


def spvoxelize(feats, idx, counts, seg=None):
    """spf.spvoxelize (scatter-mean of point rows into voxel rows); `seg` = voxelize_segments(idx, m)
    selects the atomic-free sorted form."""
    return _Voxelize.apply(feats, idx, counts, seg)


class _Devoxelize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, idx, weights, seg):
        L = _lib.load()
        feats = req(feats.contiguous(), F32, "spdevoxelize feats", 2)
        req(idx, I32, "spdevoxelize idx", 2)
        req(weights, F32, "spdevoxelize weights", 2)
        m, c = feats.shape
        n = idx.shape[0]
        if idx.shape != (n, 8) or weights.shape != (n, 8):
            raise ValueError("spdevoxelize: idx and weights must be (N,8)")
        out = _empty((n, c), F32, feats)
        check(L.ftx_devoxelize_fwd(ptr(feats), ptr(idx), ptr(weights), n, c, m, ptr(out), stream()), "ftx_devoxelize_fwd")
        ctx.save_for_backward(idx, weights)
        ctx.m, ctx.seg = m, seg
        return out

    @staticmethod
    def backward(ctx, grad_out):
        L = _lib.load()
        idx, weights = ctx.saved_tensors
        grad_out = req(grad_out.contiguous(), F32, "spdevoxelize grad", 2)
        n, c = grad_out.shape
        gf = _empty((ctx.m, c), F32, grad_out)
        seg = ctx.seg
        if seg is not None:
            if seg.m != ctx.m or seg.order.shape[0] != n * 8:
                raise ValueError("spdevoxelize: segments do not match idx")
            check(L.ftx_devoxelize_bwd_sorted(ptr(grad_out), ptr(weights), ptr(seg.order), ptr(seg.seg_off), n, c, ctx.m, ptr(gf), stream()),
                  "ftx_devoxelize_bwd_sorted")
        else:
            check(L.ftx_devoxelize_bwd(ptr(grad_out), ptr(idx), ptr(weights), n, c, ctx.m, ptr(gf), stream()), "ftx_devoxelize_bwd")
        return gf, None, None, None


def spdevoxelize(feats, idx, weights, seg=None):
    """spf.spdevoxelize (8-corner weighted gather of voxel rows onto points); `seg` =
    devoxelize_segments(idx, weights, m) makes the backward atomic-free.  Differentiable in feats only: the trilinear weights are data
    of the point cloud, and weights that ask for a gradient are refused."""
    _refuse_grad(weights, "spdevoxelize", "weights", "they are computed from the point coordinates, detach them")
    return _Devoxelize.apply(feats, idx, weights, seg)


# ---------------------------------------------------------------- sparse convolution
# When set to a list, every sparse-conv launch appends (kind, start_event, end_event,
# shape dict): HIP events recorded on the launch stream, read back by bench.py after the step.
LAUNCH_LOG = None


def _log_launch(kind, meta, launch):
    if LAUNCH_LOG is None:
        return launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = launch()
    e1.record()
    LAUNCH_LOG.append((kind, e0, e1, meta))
    return out


# The operand modes of the pair GEMM, the dense rows and the weight gradient, as the layer record of the executors numbers them
# (include/ftx.h).  "fp32": the exact fp32 MFMA (csrc/ftx_spconv.hip).  "bf16": the operands rounded to bf16 (csrc/ftx_spconv_bf16.hip).
# "split": every operand split into three bf16 pieces, six piece products summed in fp32 -- fp32-class results on the bf16 MFMA
# (csrc/ftx_spconv_split.hip).  Accumulation and storage are fp32 in all three.  False == 0 and True == 1, so bf16=False / bf16=True
# index the tables below as they always did.
FP32, BF16, SPLIT = 0, 1, 2
OPERANDS = {"fp32": FP32, "bf16": BF16, "split": SPLIT}


def operand_mode(bf16=False, operands=None):
    """The mode (FP32, BF16 or SPLIT) that the public pair `bf16=`, `operands=` names.  operands=None: bf16=False / True mean what
    they always meant.  operands="fp32" | "bf16" | "split" names the mode itself; bf16=True next to another mode is a contradiction
    and refused.  `bf16` is a flag, not a mode number: anything but False / True (0 / 1) is refused, so `bf16=2` never means split.
    Inside this module a resolved mode travels in the launchers' and autograd nodes' `bf16` argument and is never resolved again."""
    if operands is None:
        if bf16 not in (False, True):
            raise ValueError(f"bf16 must be False or True, got {bf16!r}")
        return int(bf16)
    if operands not in OPERANDS:
        raise ValueError(f"operands must be 'fp32', 'bf16' or 'split', got {operands!r}")
    if bf16 and OPERANDS[operands] != BF16:
        raise ValueError(f"bf16=True contradicts operands={operands!r}")
    return OPERANDS[operands]


# (C entry, launch-log kind) per mode
_PAIRS_GEMM = {FP32: ("ftx_spconv_pairs_gemm", "spconv_pairs_gemm"), BF16: ("ftx_spconv_pairs_gemm_bf16", "spconv_pairs_gemm_bf16"),
               SPLIT: ("ftx_spconv_pairs_gemm_split", "spconv_pairs_gemm_split")}
_PAIRS_GEMM_SCATTER = {FP32: "ftx_spconv_pairs_gemm_scatter", BF16: "ftx_spconv_pairs_gemm_scatter_bf16", SPLIT: "ftx_spconv_pairs_gemm_scatter_split"}
_PAIRS_WGRAD = {FP32: ("ftx_spconv_pairs_wgrad", "ftx_spconv_pairs_wgrad_workspace_bytes", "spconv_pairs_wgrad"),
                BF16: ("ftx_spconv_pairs_wgrad_bf16", "ftx_spconv_pairs_wgrad_bf16_workspace_bytes", "spconv_pairs_wgrad_bf16"),
                SPLIT: ("ftx_spconv_pairs_wgrad_split", "ftx_spconv_pairs_wgrad_split_workspace_bytes", "spconv_pairs_wgrad_split")}
_ROWS_GEMM = {FP32: "ftx_rows_gemm", BF16: "ftx_rows_gemm_bf16", SPLIT: "ftx_rows_gemm_split"}


# The launchers: the ONE call site of each convolution / BatchNorm entry point and of its launch-log metadata.  Pointers are raw device
# addresses; results and temporaries go where the caller says (sparse_conv and batch_norm allocate tensors, so they can be captured
# into a HIP graph; conv_bn_train carves its temporaries from the stream's scratch buffer).
def _launch_pairs_gemm(a, rows_a, gather, w, w_transposed, koff, n_pairs, ca, co, kvol, tmp, n_out, st, bf16):
    """tmp[p] = A[gather[p]] @ W[k(p)]; n_out (the rows of the reduce that follows) is for the log only.  Returns the log metadata."""
    L = _lib.load()
    gemm, kind = _PAIRS_GEMM[bf16]
    meta = dict(pairs=n_pairs, n_out=n_out, ca=ca, co=co, kvol=kvol)
    _log_launch(kind, meta, lambda: check(getattr(L, gemm)(a, rows_a, gather, w, w_transposed, koff, n_pairs, ca, co, kvol, tmp, st), gemm))
    return meta


def _launch_pairs(a, rows_a, gather, w, w_transposed, pos, koff, n_pairs, ca, co, kvol, tmp, out, n_out, st, bf16, part=0, nb=0):
    """tmp[p] = A[gather[p]] @ W[k(p)], then out = the reduce of tmp over the offsets through `pos`.  part != 0: the reduce also leaves
    the BatchNorm statistics of `out` there (nb partial rows + the totals row, float64; `st` then has its tickets attached)."""
    L = _lib.load()
    meta = _launch_pairs_gemm(a, rows_a, gather, w, w_transposed, koff, n_pairs, ca, co, kvol, tmp, n_out, st, bf16)
    if part:
        _log_launch("spconv_reduce", meta, lambda: check(L.ftx_spconv_reduce_stats(tmp, pos, n_out, co, kvol, out, part, nb, st), "ftx_spconv_reduce_stats"))
    else:
        _log_launch("spconv_reduce", meta, lambda: check(L.ftx_spconv_reduce(tmp, pos, n_out, co, kvol, out, st), "ftx_spconv_reduce"))


def _launch_direct(a, rows_a, gather, scatter, w, w_transposed, koff, n_pairs, ca, co, kvol, out, n_out, st, bf16):
    """out[scatter[p]] = A[gather[p]] @ W[k(p)]: the pair GEMM with the scatter epilogue."""
    L = _lib.load()
    gemm = _PAIRS_GEMM_SCATTER[bf16]
    _log_launch(_PAIRS_GEMM[bf16][1], dict(pairs=n_pairs, n_out=n_out, ca=ca, co=co, kvol=kvol, direct=True), lambda: check(getattr(L, gemm)(
        a, rows_a, gather, scatter, w, w_transposed, koff, n_pairs, ca, co, kvol, out, n_out, st), gemm))


def _launch_ostat(a, rows_a, nbr, n_out, w, w_transposed, flip, ca, co, kvol, out, part, nb, st, pairs):
    """out[o] = sum_k A[nbr[k, o]] @ W[k]; part != 0: also the BatchNorm statistics, as _launch_pairs.  `pairs` is for the log only."""
    L = _lib.load()
    _log_launch("spconv_ostat", dict(pairs=pairs, n_out=n_out, ca=ca, co=co, kvol=kvol, direct=True), lambda: check(L.ftx_spconv_ostat(
        a, rows_a, nbr, n_out, w, w_transposed, flip, ca, co, kvol, out, part, nb, st), "ftx_spconv_ostat"))


def _launch_wgrad(a, rows_a, idx_a, g, rows_g, idx_g, koff, n_pairs, ca, cg, kvol, dw, ws, ws_bytes, st, bf16):
    """dw[k] = sum over the pairs p of offset k of A[idx_a[p]]^T G[idx_g[p]]."""
    L = _lib.load()
    fn, _, kind = _PAIRS_WGRAD[bf16]
    _log_launch(kind, dict(pairs=n_pairs, n_out=rows_g, ca=ca, co=cg, kvol=kvol), lambda: check(getattr(L, fn)(
        a, rows_a, idx_a, g, rows_g, idx_g, koff, n_pairs, ca, cg, kvol, dw, ws, ws_bytes, st), fn))


def _launch_bn_fwd(x, residual, gamma, beta, running_mean, running_var, momentum, eps, n, c, relu, y, mean, invstd, st, ws=0, ws_bytes=0, totals=0):
    """y = relu?(BN(x) (+ residual)).  totals = 0: a statistics pass and the apply pass both read x (workspace `ws`); otherwise the
    address of the column totals that the convolution left while it wrote x, and x is read once."""
    L = _lib.load()
    args = (x, residual, gamma, beta, running_mean, running_var, float(momentum), float(eps), n, c, int(relu), y, mean, invstd)
    if totals:
        _log_launch("bn_fwd", dict(n=n, c=c, reads=1 + (residual != 0), writes=1), lambda: check(L.ftx_bn_train_fwd_totals(*args, totals, st), "ftx_bn_train_fwd_totals"))
    else:
        _log_launch("bn_fwd", dict(n=n, c=c, reads=2 + (residual != 0), writes=1), lambda: check(L.ftx_bn_train_fwd(*args, ws, ws_bytes, st), "ftx_bn_train_fwd"))


def _launch_bn_bwd(gy, x, y, gamma, beta, mean, invstd, n, c, relu, gx, gres, ggamma, gbeta, ws, ws_bytes, st):
    """Two passes (statistics, apply), each reading gy and x (and y for the ReLU mask when a residual went into it: otherwise the mask is
    recomputed from x; beta = 0 reads y in that case too); one or two row matrices written (gres = 0: there was no residual)."""
    L = _lib.load()
    has_res = gres != 0
    _log_launch("bn_bwd", dict(n=n, c=c, reads=2 * (2 + (1 if (relu and has_res) else 0)), writes=1 + (1 if has_res else 0)), lambda: check(
        L.ftx_bn_train_bwd(gy, x, y, gamma, beta, mean, invstd, n, c, int(relu), gx, gres, ggamma, gbeta, ws, ws_bytes, st), "ftx_bn_train_bwd"))


def _spconv_apply(A, W, gather, pos, koff, n_pairs, n_rows_out, co, w_transposed, bf16=False, operands=None, mode=None):
    """reduce(pairs_gemm(A[gather] @ W[k]), pos) -> (n_rows_out, co)."""
    rows_a, ca = A.shape
    tmp = _empty((n_pairs, co), F32, A)
    out = _empty((n_rows_out, co), F32, A)
    _launch_pairs(ptr(A), rows_a, ptr(gather), ptr(W), int(w_transposed), ptr(pos), ptr(koff), n_pairs, ca, co, koff.shape[0] - 1, ptr(tmp), ptr(out),
                  n_rows_out, stream(), operand_mode(bf16, operands) if mode is None else mode)
    return out


def _spconv_direct(A, W, gather, scatter, koff, n_pairs, n_rows_out, co, w_transposed, bf16=False, operands=None, mode=None):
    """out[scatter[p]] = A[gather[p]] @ W[k(p)] in ONE launch, for maps whose destination side is a bijection of the pair list."""
    rows_a, ca = A.shape
    if n_pairs != n_rows_out:
        raise ValueError("direct sparse conv: the pair list must cover every destination row exactly once")
    out = _empty((n_rows_out, co), F32, A)
    _launch_direct(ptr(A), rows_a, ptr(gather), ptr(scatter), ptr(W), int(w_transposed), ptr(koff), n_pairs, ca, co, koff.shape[0] - 1, ptr(out),
                   n_rows_out, stream(), operand_mode(bf16, operands) if mode is None else mode)
    return out


_OSTAT_OK = {}
_OSTAT_MAX_ROWS = 64 * 4096      # one block per 64 output rows, at most 4096 partial rows in the statistics hand-over


def ostat_supported(ca, co, kvol, w_transposed=False, rows=0):
    """Does the one-launch output-stationary kernel (ftx_spconv_ostat) take this layer?  (ca in {4, 32, 64}, co in {32, 64},
    at most 262 144 output rows; anything else runs on the pair-list kernels)"""
    key = (int(ca), int(co), int(kvol), bool(w_transposed))
    v = _OSTAT_OK.get(key)
    if v is None:
        v = _OSTAT_OK[key] = bool(_lib.load().ftx_spconv_ostat_supported(key[0], key[1], key[2], int(key[3])))
    return v and rows <= _OSTAT_MAX_ROWS


def ostat_preferred(ca, co, kvol, w_transposed=False, rows=0):
    """Where the output-stationary kernel is FASTER than pair GEMM + reduce on MI355X (tools/bench_spconv.py, profiles/r03_spconv_layer_micro.txt):
    forward convolutions with c_in <= 32 and c_out = 32 -- the stem, the 32 -> 32 layers of levels 1 and 2, the strided 32 -> 32 layers.
    It is bound by instruction issue (~23 instructions per pair), so 64-channel layers and the transposed-W data-gradient form lose
    (csrc/ftx_spconv_ostat.hip).  No data gradient is therefore ever sent to it: _conv_route asks for forward convolutions only, and the
    mirrored form (w_transposed = 1, flip = 1) is reached through _spconv_ostat alone."""
    return ostat_supported(ca, co, kvol, w_transposed, rows) and not w_transposed and co == 32 and ca <= 32


def _spconv_ostat(A, W, nbr, n_rows_out, co, w_transposed, flip, part=0, nb=0, pairs=0):
    """out[o] = sum_k A[nbr[k, o]] @ W[k] in ONE launch (no pair rows, no reduce pass); `part`: also the BatchNorm statistics."""
    rows_a, ca = A.shape
    kvol = nbr.shape[0]
    if nbr.shape[1] != n_rows_out:
        raise ValueError("ostat sparse conv: the neighbour table does not match the output rows")
    out = _empty((n_rows_out, co), F32, A)
    _launch_ostat(ptr(A), rows_a, ptr(nbr), n_rows_out, ptr(W), int(w_transposed), int(flip), ca, co, kvol, ptr(out), part, nb,
                  _stream_scratch() if part else stream(), pairs)
    return out


def _spconv_wgrad(A, idx_a, G, idx_g, koff, n_pairs, bf16=False, operands=None, mode=None):
    mode = operand_mode(bf16, operands) if mode is None else mode      # mode: already resolved (the autograd nodes)
    rows_a, ca = A.shape
    rows_g, cg = G.shape
    kvol = koff.shape[0] - 1
    dW = _empty((kvol, ca, cg), F32, A)
    ws_bytes = _ws_bytes(_PAIRS_WGRAD[mode][1], n_pairs, ca, cg, kvol)
    ws = _scratch(ws_bytes, A)
    _launch_wgrad(ptr(A), rows_a, ptr(idx_a), ptr(G), rows_g, ptr(idx_g), ptr(koff), n_pairs, ca, cg, kvol, ptr(dW), ptr(ws), ws_bytes, stream(), mode)
    return dW


def _conv_shapes(feats, kernel, km, transposed):
    kvol, ca, co = kernel.shape
    n_in, n_out = (km.n_out, km.n_in) if transposed else (km.n_in, km.n_out)
    if feats.shape != (n_in, ca) or km.kvol != kvol:
        raise ValueError(f"conv3d: shape mismatch feats {tuple(feats.shape)} kernel {tuple(kernel.shape)} map ({km.kvol},{n_in}->{n_out})")
    return kvol, ca, co, n_in, n_out


def _map_sides(km, transposed):
    """(src, src_pos, dst, dst_pos): per pair the row the convolution reads (`src`) and the row it writes (`dst`), and per side the
    (kvol, rows) table of each row's pairs.  The forward gathers `src` and scatters to `dst` / reduces through `dst_pos`; the data
    gradient gathers `dst` and scatters to `src` / reduces through `src_pos`.  `transposed` swaps the two sides of the map."""
    if transposed:
        return km.pair_out, km.pos, km.pair_in, km.pos_t
    return km.pair_in, km.pos_t, km.pair_out, km.pos


_EMPTY, _DIRECT, _OSTAT, _PAIRS = "empty", "direct", "ostat", "pairs"


def _conv_route(km, transposed, ca, co, kvol, rows, bf16, grad=False):
    """How sparse_conv and conv_bn_train compute the (rows, co) result of a ca -> co GEMM over the map's pairs: a layer's forward, or
    (grad=True) its data gradient.  _DIRECT: one launch with the scatter epilogue, where every row written is the destination of
    exactly one pair (the strided 2^3 map seen from its fine side: forward of the transposed conv, data gradient of the strided one).
    _OSTAT: the output-stationary kernel on the neighbour table, for the thin forward layers of the fp32 and the split mode (the kernel
    is exact fp32, which meets the split mode's fp32-class contract; `bf16` is the operand mode).  _PAIRS: pair GEMM + reduce.
    _EMPTY: no pair or no row -- the forward takes the pair list without the statistics-producing forms, the gradient is a zero fill."""
    if grad:
        if rows == 0 or km.n_pairs == 0:
            return _EMPTY
        return _DIRECT if (not transposed and km.fine_bijective) else _PAIRS
    if transposed and km.fine_bijective:
        return _DIRECT
    if rows == 0 or km.n_pairs == 0:
        return _EMPTY
    if bf16 != BF16 and not transposed and ostat_preferred(ca, co, kvol, rows=rows):
        return _OSTAT
    return _PAIRS


def _conv_forward(feats, kernel, km, transposed, bf16=False):
    """`bf16`: the operand mode.  BF16: the output-stationary kernel is exact fp32 only, so every layer takes the pair list."""
    kvol, ca, co, n_in, n_out = _conv_shapes(feats, kernel, km, transposed)
    route = _conv_route(km, transposed, ca, co, kvol, n_out, bf16)
    src, _, dst, dst_pos = _map_sides(km, transposed)
    if route == _DIRECT:
        return _spconv_direct(feats, kernel, src, dst, km.koff, km.n_pairs, n_out, co, 0, mode=bf16)
    if route == _OSTAT:
        return _spconv_ostat(feats, kernel, km.nbr, n_out, co, 0, 0, pairs=km.n_pairs)
    return _spconv_apply(feats, kernel, src, dst_pos, km.koff, km.n_pairs, n_out, co, 0, mode=bf16)


def _conv_backward(feats, kernel, km, transposed, grad_out, need_feats, need_kernel, bf16=False):
    kvol, ca, co = kernel.shape
    n_feats = feats.shape[0]
    g_feats = g_kernel = None
    src, src_pos, dst, _ = _map_sides(km, transposed)
    if need_feats:
        route = _conv_route(km, transposed, co, ca, kvol, n_feats, bf16, grad=True)
        if route == _EMPTY:
            g_feats = torch.zeros((n_feats, ca), dtype=F32, device=feats.device)
        elif route == _DIRECT:
            g_feats = _spconv_direct(grad_out, kernel, dst, src, km.koff, km.n_pairs, n_feats, ca, 1, mode=bf16)
        else:
            g_feats = _spconv_apply(grad_out, kernel, dst, src_pos, km.koff, km.n_pairs, n_feats, ca, 1, mode=bf16)
    if need_kernel:
        g_kernel = _spconv_wgrad(feats, src, grad_out, dst, km.koff, km.n_pairs, mode=bf16)
    return g_feats, g_kernel


class _SparseConv(torch.autograd.Function):
    """out[o] = sum over pairs (k, i->o) of feats[i] @ kernel[k].

    `km` is a KernelMap (pair list); `transposed` swaps the roles of its two sides: the
    transposed conv of models/spvcnn.py:42-46 reuses the paired strided conv's map."""

    @staticmethod
    def forward(ctx, feats, kernel, km, transposed, bf16=False):
        feats = req(feats.contiguous(), F32, "conv3d feats", 2)
        kernel = req(kernel.contiguous(), F32, "conv3d kernel", 3)
        out = _conv_forward(feats, kernel, km, transposed, bf16)
        ctx.save_for_backward(feats, kernel)
        ctx.km, ctx.transposed, ctx.bf16 = km, transposed, bf16
        return out

    @staticmethod
    def backward(ctx, grad_out):
        feats, kernel = ctx.saved_tensors
        grad_out = req(grad_out.contiguous(), F32, "conv3d grad", 2)
        g_feats, g_kernel = _conv_backward(feats, kernel, ctx.km, ctx.transposed, grad_out, ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.bf16)
        return g_feats, g_kernel, None, None, None


def sparse_conv(feats, kernel, km, transposed=False, bf16=False, operands=None):
    """bf16=True (operands="bf16"): forward, data gradient and weight gradient on bf16-rounded operands with fp32 accumulation.
    operands="split": the three on three-piece split operands, fp32-class results on the bf16 MFMA; layers the output-stationary kernel
    takes in fp32 mode keep it (it is exact fp32).  The contracts are stated in include/ftx.h."""
    return _SparseConv.apply(feats, kernel, km, transposed, operand_mode(bf16, operands))


# ---------------------------------------------------------------- dense rows (skinny GEMMs)
def _rows_gemm(A, W, w_transposed, bias, co, bf16=False):
    L = _lib.load()
    n, ca = A.shape
    out = _empty((n, co), F32, A)
    fn = _ROWS_GEMM[bf16]                      # a resolved mode, as in the launchers above
    check(getattr(L, fn)(ptr(A), n, ptr(W), int(w_transposed), ptr(bias), ca, co, ptr(out), stream()), fn)
    return out


def _rows_wgrad(A, G, bf16=False):
    """A (n, ca)^T @ G (n, cg) -> (ca, cg)."""
    L = _lib.load()
    fn, ws_fn, _ = _PAIRS_WGRAD[bf16]
    n, ca = A.shape
    cg = G.shape[1]
    dW = _empty((1, ca, cg), F32, A)
    ws_bytes = _ws_bytes(ws_fn, n, ca, cg, 1)
    ws = _scratch(ws_bytes, A)
    check(getattr(L, fn)(ptr(A), n, 0, ptr(G), n, 0, 0, n, ca, cg, 1, ptr(dW), ptr(ws), ws_bytes, stream()), fn + "(dense)")
    return dW[0]


def _rows_ok(*channels):
    return all(c >= 4 and c % 4 == 0 for c in channels)


class _RowsLinear(torch.autograd.Function):
    """F.linear on (N, C) rows: out = x @ weight^T + bias, weight (co, ca) as nn.Linear stores it."""

    @staticmethod
    def forward(ctx, x, weight, bias, bf16=False):
        x = req(x.contiguous(), F32, "linear x", 2)
        weight = req(weight.contiguous(), F32, "linear weight", 2)
        co, ca = weight.shape
        if x.shape[1] != ca:
            raise ValueError("linear: shape mismatch")
        _channel_operands(x, co, "linear", optional=("bias",), bias=bias)
        ctx.save_for_backward(x, weight)
        ctx.has_bias, ctx.bf16 = bias is not None, bf16
        return _rows_gemm(x, weight, 1, bias, co, bf16)

    @staticmethod
    def backward(ctx, go):
        x, weight = ctx.saved_tensors
        go = req(go.contiguous(), F32, "linear grad", 2)
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _rows_gemm(go, weight, 0, None, weight.shape[1], ctx.bf16)
        if ctx.needs_input_grad[1]:
            gw = _rows_wgrad(go, x, ctx.bf16)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = colsum(go) if go.shape[1] % 4 == 0 else go.sum(0)
        return gx, gw, gb, None


class _RowsMatmul(torch.autograd.Function):
    """x (N, ca) @ kernel (ca, co): the kernel_size = 1 spnn.Conv3d."""

    @staticmethod
    def forward(ctx, x, kernel, bf16=False):
        x = req(x.contiguous(), F32, "matmul x", 2)
        kernel = req(kernel.contiguous(), F32, "matmul kernel", 2)
        if x.shape[1] != kernel.shape[0]:
            raise ValueError("matmul: shape mismatch")
        ctx.save_for_backward(x, kernel)
        ctx.bf16 = bf16
        return _rows_gemm(x, kernel, 0, None, kernel.shape[1], bf16)

    @staticmethod
    def backward(ctx, go):
        x, kernel = ctx.saved_tensors
        go = req(go.contiguous(), F32, "matmul grad", 2)
        gx = _rows_gemm(go, kernel, 1, None, kernel.shape[0], ctx.bf16) if ctx.needs_input_grad[0] else None
        gk = _rows_wgrad(x, go, ctx.bf16) if ctx.needs_input_grad[1] else None
        return gx, gk, None


def _bf16_round(t):
    """t rounded to bf16 (round-to-nearest-even), held in fp32."""
    return t.bfloat16().float()


class _LibraryMatmulBf16(torch.autograd.Function):
    """x @ w (+ bias) as a library GEMM on bf16-rounded operands with fp32 results, for the shapes the tile kernel does not take: the
    contract of the bf16 kernels (forward: x and w rounded; data gradient: grad and w; weight gradient: grad and x; bias in fp32)."""

    @staticmethod
    def forward(ctx, x, w, bias):
        xr, wr = _bf16_round(x), _bf16_round(w)
        ctx.save_for_backward(xr, wr)
        ctx.has_bias = bias is not None
        out = torch.matmul(xr, wr)
        return out + bias if bias is not None else out

    @staticmethod
    def backward(ctx, go):
        xr, wr = ctx.saved_tensors
        gr = _bf16_round(go)
        gx = torch.matmul(gr, wr.t()) if ctx.needs_input_grad[0] else None
        gw = torch.matmul(xr.reshape(-1, xr.shape[-1]).t(), gr.reshape(-1, gr.shape[-1])) if ctx.needs_input_grad[1] else None
        gb = go.reshape(-1, go.shape[-1]).sum(0) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return gx, gw, gb


def linear(x, weight, bias=None, bf16=False, operands=None):
    """nn.Linear on point / voxel rows.  Skinny shapes (tens of thousands of rows, <= 384 channels)
    run on libftx's tile kernel; anything else is a plain library GEMM.  bf16=True (operands="bf16"): x, weight (and in the backward
    the output gradient) rounded to bf16 as GEMM operands, fp32 accumulation, on every shape.  operands="split": the tile kernel on
    three-piece split operands (fp32-class results); a shape the tile kernel does not take runs the plain fp32 library GEMM."""
    mode = operand_mode(bf16, operands)
    if x.dim() == 2 and _rows_ok(x.shape[1], weight.shape[0]) and max(weight.shape) <= 512:
        return _RowsLinear.apply(x, weight, bias, mode)
    if mode == BF16:
        return _LibraryMatmulBf16.apply(x, weight.t(), bias)
    return torch.nn.functional.linear(x, weight, bias)


def rows_matmul(x, kernel, bf16=False, operands=None):
    """x (N, ca) @ kernel (ca, co); `bf16` / `operands` as in linear()."""
    mode = operand_mode(bf16, operands)
    if x.dim() == 2 and _rows_ok(*kernel.shape) and max(kernel.shape) <= 512:
        return _RowsMatmul.apply(x, kernel, mode)
    if mode == BF16:
        return _LibraryMatmulBf16.apply(x, kernel, None)
    return torch.matmul(x, kernel)


# ---------------------------------------------------------------- BatchNorm (+residual)(+ReLU)
def _bn_operands(residual, gamma, beta, n, c, who, params):
    """Operand checks of the training-mode BatchNorm nodes; returns the contiguous residual."""
    if residual is not None:
        residual = req(residual.contiguous(), F32, "bn residual", 2)
        if residual.shape != (n, c):
            raise ValueError(who + ": residual shape mismatch")
    for t, nm in ((gamma, "gamma"), (beta, "beta")):
        req(t, F32, "bn " + nm, 1)
        if t.shape[0] != c:
            raise ValueError(f"{who}: {params}")
    return residual


def _channel_operands(like, c, who, optional=(), **named):
    """Per-channel float32 vectors that reach a kernel as raw pointers (a bias, BatchNorm parameters, running statistics): each a
    CUDA tensor on `like`'s device, contiguous, 1-d, `c` long; the names in `optional` may be None.  Checked before anything is launched."""
    for nm, t in named.items():
        if t is None and nm in optional:
            continue
        req(t, F32, f"{who} {nm}", 1)
        if t.shape[0] != c:
            raise ValueError(f"{who} {nm}: expected ({c},), got {tuple(t.shape)}")
        if t.device != like.device:
            raise ValueError(f"{who} {nm}: lives on another device than the rows it is applied to")


def _refuse_grad(t, who, name, hint):
    """An input the node has no gradient for must not ask for one: autograd would hand back None without a word."""
    if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"{who}: no gradient is produced for {name} ({hint})")


_RUNNING = ("running_mean", "running_var")      # the training kernels take NULL for "no update" (include/ftx.h)


class _BatchNormTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, gamma, beta, running_mean, running_var, momentum, eps, relu, remask):
        x = req(x.contiguous(), F32, "bn x", 2)
        n, c = x.shape
        residual = _bn_operands(residual, gamma, beta, n, c, "bn", "parameter length != channels")
        _channel_operands(x, c, "bn", optional=_RUNNING, running_mean=running_mean, running_var=running_var)    # written in place
        y = torch.empty_like(x)
        mean = _empty((c,), F32, x)
        invstd = _empty((c,), F32, x)
        ws_bytes = _ws_bytes("ftx_bn_workspace_bytes", n, c)
        ws = _scratch(ws_bytes, x)
        _launch_bn_fwd(ptr(x), ptr(residual), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), momentum, eps, n, c, relu, ptr(y), ptr(mean),
                       ptr(invstd), _stream_scratch(), ptr(ws), ws_bytes)
        ctx.save_for_backward(x, y, gamma, beta, mean, invstd)
        ctx.relu = int(relu)
        ctx.has_res = residual is not None
        ctx.remask = bool(remask)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, y, gamma, beta, mean, invstd = ctx.saved_tensors
        gy = req(gy.contiguous(), F32, "bn grad", 2)
        n, c = x.shape
        gx = torch.empty_like(x)
        gres = torch.empty_like(x) if ctx.has_res else None
        ggamma = _empty((c,), F32, x)
        gbeta = _empty((c,), F32, x)
        ws_bytes = _ws_bytes("ftx_bn_workspace_bytes", n, c)
        ws = _scratch(ws_bytes, x)
        _launch_bn_bwd(ptr(gy), ptr(x), ptr(y), ptr(gamma), ptr(beta) if ctx.remask else 0, ptr(mean), ptr(invstd), n, c, ctx.relu, ptr(gx), ptr(gres),
                       ptr(ggamma), ptr(gbeta), ptr(ws), ws_bytes, _stream_scratch())
        return gx, gres, ggamma, gbeta, None, None, None, None, None, None


class _BatchNormEval(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, gamma, beta, running_mean, running_var, eps, relu):
        L = _lib.load()
        x = req(x.contiguous(), F32, "bn x", 2)
        n, c = x.shape
        residual = _bn_operands(residual, gamma, beta, n, c, "bn", "parameter length != channels")
        _channel_operands(x, c, "bn", running_mean=running_mean, running_var=running_var)
        y = torch.empty_like(x)
        check(L.ftx_bn_eval_fwd(ptr(x), ptr(residual), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), float(eps), n, c, int(relu),
                                ptr(y), stream()), "ftx_bn_eval_fwd")
        # x and running_mean are read by d gamma alone: kept only for a gamma that asks (the executors and model.eval() under no_grad never do)
        need_gamma = ctx.needs_input_grad[2]
        ctx.save_for_backward(y, gamma, running_var, x if need_gamma else None, running_mean if need_gamma else None)
        ctx.eps, ctx.relu, ctx.has_res = float(eps), int(relu), residual is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        # Eval-mode gradients are elementwise (torch device ops); the parameter gradients are column sums (ftx_colsum: float64, fixed order).
        y, gamma, running_var, x, running_mean = ctx.saved_tensors
        dy = gy * (y > 0) if ctx.relu else gy
        invstd = torch.rsqrt(running_var + ctx.eps)
        scale = gamma * invstd
        gx = dy * scale
        sums = colsum if gy.shape[1] % 4 == 0 else (lambda t: t.sum(0))
        ggamma = sums(dy * ((x - running_mean) * invstd)) if ctx.needs_input_grad[2] else None
        gbeta = sums(dy) if ctx.needs_input_grad[3] else None
        return gx, (dy if ctx.has_res else None), ggamma, gbeta, None, None, None, None


class _ConvBNTrain(torch.autograd.Function):
    """spnn.Conv3d -> spnn.BatchNorm (training statistics) (-> + residual) (-> ReLU) as ONE autograd node
    (models/spvcnn.py:22-35,38-50,53-79).  The reduce pass of the convolution produces the BatchNorm's batch statistics while
    it writes the convolution output (ftx_spconv_reduce_stats: the last block to finish leaves the column totals), so that output is read
    once, by the one apply launch (ftx_bn_train_fwd_totals), instead of twice;
    one node instead of two also halves the host work per layer, and everything that does not outlive the call -- the pair rows `tmp`,
    the partial statistics, the BatchNorm input gradient between the two halves of the backward, the kernel workspaces -- lives in the
    stream's scratch buffer instead of six allocator round trips per layer and direction.  Route and launchers are sparse_conv's."""

    @staticmethod
    def forward(ctx, feats, kernel, km, transposed, residual, gamma, beta, running_mean, running_var, momentum, eps, relu, bf16, remask):
        feats = req(feats.contiguous(), F32, "conv3d feats", 2)
        kernel = req(kernel.contiguous(), F32, "conv3d kernel", 3)
        kvol, ca, co, n_in, n_out = _conv_shapes(feats, kernel, km, transposed)
        residual = _bn_operands(residual, gamma, beta, n_out, co, "conv_bn", "BatchNorm parameter length != output channels")
        _channel_operands(feats, co, "conv_bn", optional=_RUNNING, running_mean=running_mean, running_var=running_var)    # written in place
        stats = _empty((2, co), F32, feats)              # row 0: batch mean, row 1: 1 / sqrt(var + eps)
        x = _empty((n_out, co), F32, feats)
        y = torch.empty_like(x)
        st = _stream_scratch()
        route = _conv_route(km, transposed, ca, co, kvol, n_out, bf16)
        src, _, dst, dst_pos = _map_sides(km, transposed)
        tmp_bytes = 0 if route in (_DIRECT, _OSTAT) else 4 * km.n_pairs * co
        if route in (_OSTAT, _PAIRS):   # the convolution leaves the statistics (nb partial rows + the totals row, float64), then the apply pass
            nb = _ws_bytes("ftx_spconv_ostat_blocks", n_out) if route == _OSTAT else _ws_bytes("ftx_spconv_reduce_stats_blocks", n_out, co)
            tmp, part = _carve(feats, tmp_bytes, 16 * (nb + 1) * co)
            ws = ws_bytes = 0
            totals = part + 16 * nb * co
        else:                           # scatter epilogue or empty map: the plain convolution, then the BatchNorm's own statistics pass
            ws_bytes = _ws_bytes("ftx_bn_workspace_bytes", n_out, co)
            tmp, ws = _carve(feats, tmp_bytes, ws_bytes)
            part = nb = totals = 0
        if route == _DIRECT:
            _launch_direct(ptr(feats), n_in, ptr(src), ptr(dst), ptr(kernel), 0, ptr(km.koff), km.n_pairs, ca, co, kvol, ptr(x), n_out, st, bf16)
        elif route == _OSTAT:
            _launch_ostat(ptr(feats), n_in, ptr(km.nbr), n_out, ptr(kernel), 0, 0, ca, co, kvol, ptr(x), part, nb, st, km.n_pairs)
        else:
            _launch_pairs(ptr(feats), n_in, ptr(src), ptr(kernel), 0, ptr(dst_pos), ptr(km.koff), km.n_pairs, ca, co, kvol, tmp, ptr(x), n_out, st, bf16,
                          part, nb)
        _launch_bn_fwd(ptr(x), ptr(residual), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), momentum, eps, n_out, co, relu, ptr(y),
                       stats.data_ptr(), stats.data_ptr() + 4 * co, st, ws, ws_bytes, totals)
        ctx.save_for_backward(feats, kernel, x, y, gamma, beta, stats)
        ctx.km, ctx.transposed, ctx.relu, ctx.has_res, ctx.bf16, ctx.remask = km, transposed, int(relu), residual is not None, bf16, bool(remask)
        return y

    @staticmethod
    def backward(ctx, gy):
        feats, kernel, x, y, gamma, beta, stats = ctx.saved_tensors
        km, transposed, bf16 = ctx.km, ctx.transposed, ctx.bf16
        gy = req(gy.contiguous(), F32, "conv_bn grad", 2)
        n, co = x.shape
        kvol, ca, _ = kernel.shape
        n_feats = feats.shape[0]
        need_feats, need_kernel = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        st = _stream_scratch()
        gparams = _empty((2, co), F32, x)               # row 0: d gamma, row 1: d beta
        gres = torch.empty_like(x) if ctx.has_res else None
        src, src_pos, dst, _ = _map_sides(km, transposed)
        route = _conv_route(km, transposed, co, ca, kvol, n_feats, bf16, grad=True) if need_feats else None
        bn_ws_bytes = _ws_bytes("ftx_bn_workspace_bytes", n, co)
        wg_bytes = _ws_bytes(_PAIRS_WGRAD[bf16][1], km.n_pairs, ca, co, kvol) if (need_kernel and km.n_pairs > 0) else 0
        bn_ws, gx, tmp, wg_ws = _carve(x, bn_ws_bytes, 4 * n * co, 4 * km.n_pairs * ca if route == _PAIRS else 0, wg_bytes)
        # BatchNorm half: gx = d loss / d (convolution output) stays in the scratch buffer, it is consumed by the two calls below
        _launch_bn_bwd(ptr(gy), ptr(x), ptr(y), ptr(gamma), ptr(beta) if ctx.remask else 0, stats.data_ptr(), stats.data_ptr() + 4 * co, n, co, ctx.relu,
                       gx, ptr(gres), gparams.data_ptr(), gparams.data_ptr() + 4 * co, bn_ws, bn_ws_bytes, st)
        g_feats = g_kernel = None
        if need_feats:
            g_feats = _empty((n_feats, ca), F32, x)
            if route == _EMPTY:
                g_feats.zero_()
            elif route == _DIRECT:
                _launch_direct(gx, n, ptr(dst), ptr(src), ptr(kernel), 1, ptr(km.koff), km.n_pairs, co, ca, kvol, ptr(g_feats), n_feats, st, bf16)
            else:
                _launch_pairs(gx, n, ptr(dst), ptr(kernel), 1, ptr(src_pos), ptr(km.koff), km.n_pairs, co, ca, kvol, tmp, ptr(g_feats), n_feats, st, bf16)
        if need_kernel:
            g_kernel = _empty((kvol, ca, co), F32, x)
            _launch_wgrad(ptr(feats), n_feats, ptr(src), gx, n, ptr(dst), ptr(km.koff), km.n_pairs, ca, co, kvol, ptr(g_kernel), wg_ws, wg_bytes, st, bf16)
        return g_feats, g_kernel, None, None, gres, gparams[0], gparams[1], None, None, None, None, None, None, None


def conv_bn_train(feats, kernel, km, transposed, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, residual=None, relu=False,
                  bf16=False, remask=True, operands=None):
    """Conv3d -> BatchNorm(training) (+ residual) (+ ReLU) in one autograd node; see _ConvBNTrain.  bf16=True (operands="bf16"): the
    convolution's forward, data gradient and weight gradient on bf16-rounded operands (as sparse_conv(bf16=True)); operands="split":
    on three-piece split operands (as sparse_conv(operands="split")).  BatchNorm stays fp32.  remask: as in batch_norm."""
    return _ConvBNTrain.apply(feats, kernel, km, transposed, residual, gamma, beta, running_mean, running_var, momentum, eps, relu,
                              operand_mode(bf16, operands), bool(remask))


def batch_norm(x, gamma, beta, running_mean, running_var, training, momentum=0.1, eps=1e-5, residual=None, relu=False, remask=True):
    """y = relu?(BN(x) (+ residual)) over the rows of x (N,C).  remask (training): the backward recomputes the ReLU mask of a
    residual-free BatchNorm from x instead of reading it from y (ftx_bn_train_bwd given beta); False reads y."""
    if training:
        return _BatchNormTrain.apply(x, residual, gamma, beta, running_mean, running_var, momentum, eps, relu, bool(remask))
    return _BatchNormEval.apply(x, residual, gamma, beta, running_mean, running_var, eps, relu)


# ---------------------------------------------------------------- eval-mode Conv3d -> BatchNorm in two launches, row helpers of the executor
def spconv_reduce_bn_eval(tmp, pos, n_out, gamma, beta, running_mean, running_var, eps=1e-5, residual=None, relu=False):
    """relu?(BNeval(sum_k tmp[pos[k, o]]) (+ residual[o])) in ONE launch (ftx_spconv_reduce_bn_eval): bit-identical to ftx_spconv_reduce
    followed by ftx_bn_eval_fwd.  tmp (P, co) pair rows, pos (kvol, n_out) int32 with kvol 8 or 27.  No autograd: eval mode only."""
    L = _lib.load()
    tmp = req(tmp, F32, "reduce_bn_eval tmp", 2)
    req(pos, I32, "reduce_bn_eval pos", 2)
    co, kvol = tmp.shape[1], pos.shape[0]
    if pos.shape[1] != n_out:
        raise ValueError("reduce_bn_eval: the position table does not match the output rows")
    for t, nm in ((gamma, "gamma"), (beta, "beta"), (running_mean, "running_mean"), (running_var, "running_var")):
        req(t, F32, "reduce_bn_eval " + nm, 1)
        if t.shape[0] != co:
            raise ValueError("reduce_bn_eval: BatchNorm parameter length != output channels")
    if residual is not None:
        residual = req(residual.contiguous(), F32, "reduce_bn_eval residual", 2)
        if residual.shape != (n_out, co):
            raise ValueError("reduce_bn_eval: residual shape mismatch")
    out = _empty((n_out, co), F32, tmp)
    _log_launch("spconv_reduce", dict(pairs=tmp.shape[0], n_out=n_out, ca=0, co=co, kvol=kvol), lambda: check(L.ftx_spconv_reduce_bn_eval(
        ptr(tmp), ptr(pos), n_out, co, kvol, ptr(residual), ptr(gamma), ptr(beta), ptr(running_mean), ptr(running_var), float(eps), int(relu), ptr(out),
        stream()), "ftx_spconv_reduce_bn_eval"))
    return out


def conv_bn_eval(feats, kernel, km, transposed, gamma, beta, running_mean, running_var, eps=1e-5, residual=None, relu=False, bf16=False,
                 operands=None):
    """Conv3d -> BatchNorm(eval) (+ residual) (+ ReLU) without autograd.  On the pair-list route (and for an empty map) the reduce carries
    the BatchNorm in its epilogue: pair GEMM + ftx_spconv_reduce_bn_eval, two launches instead of three and one (n_out, co) round trip
    less; the other routes run sparse_conv's launch and the eval BatchNorm pass.  Bit-identical to sparse_conv + batch_norm(training=False)
    in the same operand mode (`bf16` / `operands` as in sparse_conv)."""
    mode = operand_mode(bf16, operands)
    feats = req(feats.contiguous(), F32, "conv3d feats", 2)
    kernel = req(kernel.contiguous(), F32, "conv3d kernel", 3)
    kvol, ca, co, n_in, n_out = _conv_shapes(feats, kernel, km, transposed)
    route = _conv_route(km, transposed, ca, co, kvol, n_out, mode)
    if route in (_PAIRS, _EMPTY) and kvol in (8, 27):
        src, _, _, dst_pos = _map_sides(km, transposed)
        tmp = _empty((km.n_pairs, co), F32, feats)
        _launch_pairs_gemm(ptr(feats), n_in, ptr(src), ptr(kernel), 0, ptr(km.koff), km.n_pairs, ca, co, kvol, ptr(tmp), n_out, stream(), mode)
        return spconv_reduce_bn_eval(tmp, dst_pos, n_out, gamma, beta, running_mean, running_var, eps, residual=residual, relu=relu)
    with torch.no_grad():
        return batch_norm(_conv_forward(feats, kernel, km, transposed, mode), gamma, beta, running_mean, running_var, False, eps=eps,
                          residual=residual, relu=relu)


def rows_concat(a, b):
    """torch.cat([a, b], 1) of (n, ca) and (n, cb) float32 rows (ftx_rows_concat; channel counts multiples of 4)."""
    a, b = req(a, F32, "rows_concat a", 2), req(b, F32, "rows_concat b", 2)
    if a.shape[0] != b.shape[0]:
        raise ValueError("rows_concat: row counts differ")
    out = _empty((a.shape[0], a.shape[1] + b.shape[1]), F32, a)
    check(_lib.load().ftx_rows_concat(ptr(a), a.shape[1], ptr(b), b.shape[1], a.shape[0], ptr(out), stream()), "ftx_rows_concat")
    return out


def rows_split(x, ca):
    """(x[:, :ca], x[:, ca:]) of (n, ca + cb) float32 rows as two contiguous matrices in one launch (ftx_rows_split, the backward of
    rows_concat; channel counts multiples of 4)."""
    x = req(x, F32, "rows_split x", 2)
    n, cb = x.shape[0], x.shape[1] - int(ca)
    a, b = _empty((n, int(ca)), F32, x), _empty((n, cb), F32, x)
    check(_lib.load().ftx_rows_split(ptr(x), n, int(ca), cb, ptr(a), ptr(b), stream()), "ftx_rows_split")
    return a, b


def rows_add(a, b):
    """a + b of two (n, c) float32 row matrices (ftx_rows_add; c a multiple of 4)."""
    a, b = req(a, F32, "rows_add a", 2), req(b, F32, "rows_add b", 2)
    if a.shape != b.shape:
        raise ValueError("rows_add: shapes differ")
    out = torch.empty_like(a)
    check(_lib.load().ftx_rows_add(ptr(a), ptr(b), a.shape[0], a.shape[1], ptr(out), stream()), "ftx_rows_add")
    return out


# ---------------------------------------------------------------- 2D -> 3D lift, nearest resample
def lift_segments(img_idx, point_batch, b, gh, gw, H, W) -> Segments:
    """Points sorted by the grid cell they read: turns the lift's backward into a gather-reduce."""
    L = _lib.load()
    req(img_idx, I64, "lift img_idx", 2)
    req(point_batch, I32, "lift point_batch", 1)
    n = img_idx.shape[0]
    cells = _empty((n,), I32, point_batch)
    check(L.ftx_lift_cells(ptr(img_idx), ptr(point_batch), n, int(b), int(gh), int(gw), int(H), int(W), ptr(cells), stream()), "ftx_lift_cells")
    return Segments(cells, int(b) * int(gh) * int(gw))


class _LiftGather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, img_idx, point_batch, H, W, seg):
        L = _lib.load()
        grid = req(grid.contiguous(), F32, "lift grid", 4)
        req(img_idx, I64, "lift img_idx", 2)
        req(point_batch, I32, "lift point_batch", 1)
        b, gh, gw, c = grid.shape
        n = img_idx.shape[0]
        if img_idx.shape != (n, 2) or point_batch.shape[0] != n:
            raise ValueError("lift_gather: img_idx must be (N,2), point_batch (N,)")
        out = _empty((n, c), F32, grid)
        check(L.ftx_lift_gather_fwd(ptr(grid), ptr(img_idx), ptr(point_batch), n, b, gh, gw, c, int(H), int(W), ptr(out), stream()), "ftx_lift_gather_fwd")
        ctx.save_for_backward(img_idx, point_batch)
        ctx.dims = (b, gh, gw, c, int(H), int(W))
        ctx.seg = seg
        return out

    @staticmethod
    def backward(ctx, go):
        L = _lib.load()
        img_idx, point_batch = ctx.saved_tensors
        b, gh, gw, c, H, W = ctx.dims
        go = req(go.contiguous(), F32, "lift grad", 2)
        gg = _empty((b, gh, gw, c), F32, go)
        seg = ctx.seg
        if seg is not None:
            if seg.m != b * gh * gw or seg.order.shape[0] != go.shape[0]:
                raise ValueError("lift_gather: segments do not match the grid / points")
            check(L.ftx_segment_sum(ptr(go), ptr(seg.order), ptr(seg.seg_off), go.shape[0], c, seg.m, ptr(gg), stream()), "ftx_segment_sum")
        else:
            check(L.ftx_lift_gather_bwd(ptr(go), ptr(img_idx), ptr(point_batch), go.shape[0], b, gh, gw, c, H, W, ptr(gg), stream()), "ftx_lift_gather_bwd")
        return gg, None, None, None, None, None


def lift_gather(grid, img_idx, point_batch, H, W, seg=None):
    """Per-point rows of nearest-upsample(grid -> (H,W)) without materialising the map.
    `seg` = lift_segments(...) makes the backward an atomic-free, bit-reproducible gather-reduce."""
    return _LiftGather.apply(grid, img_idx, point_batch, H, W, seg)


class _ResampleNearest(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, oh, ow):
        L = _lib.load()
        x = req(x.contiguous(), F32, "resample x", 4)
        b, c, ih, iw = x.shape
        out = _empty((b, c, int(oh), int(ow)), F32, x)
        check(L.ftx_resample_nearest_fwd(ptr(x), b, c, ih, iw, int(oh), int(ow), ptr(out), stream()), "ftx_resample_nearest_fwd")
        ctx.dims = (b, c, ih, iw, int(oh), int(ow))
        return out

    @staticmethod
    def backward(ctx, go):
        L = _lib.load()
        b, c, ih, iw, oh, ow = ctx.dims
        go = req(go.contiguous(), F32, "resample grad", 4)
        gi = _empty((b, c, ih, iw), F32, go)
        check(L.ftx_resample_nearest_bwd(ptr(go), b, c, ih, iw, oh, ow, ptr(gi), stream()), "ftx_resample_nearest_bwd")
        return gi, None, None


def resample_nearest(x, size):
    """nn.Upsample(size) (nearest) on NCHW.  The backward adds with float atomics: up to two target pixels per source pixel (any
    downsample) it is exact in any order; an upsample's gradient is right to rounding, not bit-reproducible."""
    return _ResampleNearest.apply(x, size[0], size[1])


# ---------------------------------------------------------------- affine grid sampling (spatial transformers)
def _affine_operands(src, theta, who):
    """(b, c, ih, iw, host stride array) of a strided float32 source and its (b, 2, 3) theta, checked before anything is launched."""
    if not isinstance(src, torch.Tensor) or not src.is_cuda:
        raise ValueError(f"{who} src: expected a CUDA (HIP) tensor; the product path has no CPU fallback")
    if src.dtype != F32 or src.dim() != 4:
        raise ValueError(f"{who} src: expected a 4-d float32 tensor, got {src.dtype} {tuple(src.shape)}")
    b, c, ih, iw = src.shape
    if min(b, c, ih, iw) < 1 or b > 128:
        raise ValueError(f"{who} src: empty tensor or more than 128 frames: {tuple(src.shape)}")
    # any layout whose elements are distinct (NCHW, channels-last, a slice): an expanded tensor would alias its gradient
    if any(st <= 0 and sz > 1 for st, sz in zip(src.stride(), src.shape)):
        raise ValueError(f"{who} src: strides {src.stride()} alias elements")
    req(theta, F32, who + " theta", 3)
    if theta.shape != (b, 2, 3):
        raise ValueError(f"{who} theta: expected ({b}, 2, 3), got {tuple(theta.shape)}")
    if theta.device != src.device:
        raise ValueError(f"{who}: src and theta live on different devices")
    return b, c, ih, iw, (ctypes.c_int64 * 4)(*src.stride())


def _affine_size(h, w, who):
    h, w = int(h), int(w)
    if h < 1 or w < 1 or h * w >= 2 ** 31:
        raise ValueError(f"{who}: bad target size ({h}, {w})")
    return h, w


class _AffineSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, theta, oh, ow):
        L = _lib.load()
        b, c, ih, iw, strides = _affine_operands(src, theta, "affine_sample")
        out = _empty((b, c, oh, ow), F32, src)
        check(L.ftx_affine_sample_fwd(ptr(src), strides, b, c, ih, iw, ptr(theta), oh, ow, ptr(out), stream()), "ftx_affine_sample_fwd")
        ctx.save_for_backward(src, theta)
        ctx.size = (oh, ow)
        return out

    @staticmethod
    def backward(ctx, go):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None
        L = _lib.load()
        src, theta = ctx.saved_tensors
        oh, ow = ctx.size
        b, c, ih, iw, strides = _affine_operands(src, theta, "affine_sample")
        go = req(go.contiguous(), F32, "affine_sample grad", 4)
        if go.shape != (b, c, oh, ow):
            raise ValueError("affine_sample: gradient shape differs from the output's")
        gt = _empty((b, 2, 3), F32, theta)
        ws_bytes = _ws_bytes("ftx_affine_theta_workspace_bytes", b)
        ws = _scratch(ws_bytes, theta)
        check(L.ftx_affine_sample_bwd_theta(ptr(src), strides, b, c, ih, iw, ptr(theta), ptr(go), oh, ow, ptr(gt), ptr(ws), ws_bytes, stream()),
              "ftx_affine_sample_bwd_theta")
        return None, gt, None, None


def affine_sample(src, theta, size):
    """F.grid_sample(src, F.affine_grid(theta, (b, c) + size, align_corners=False), align_corners=False) -- bilinear, zero padding --
    for src (b, c, ih, iw) of any non-aliasing strides and theta (b, 2, 3); NCHW result.  The grid is never stored.  Differentiable in
    theta only (bit-reproducible): like sample_down, this dense form is for the input image and refuses a source that needs a gradient."""
    if src.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("affine_sample: the dense form does not produce a gradient for src (affine_lift does)")
    oh, ow = _affine_size(size[0], size[1], "affine_sample")
    return _AffineSample.apply(src, theta, oh, ow)


def _affine_points(img_idx, point_batch, src, who):
    req(img_idx, I64, who + " img_idx", 2)
    req(point_batch, I32, who + " point_batch", 1)
    n = img_idx.shape[0]
    if img_idx.shape != (n, 2) or point_batch.shape[0] != n:
        raise ValueError(f"{who}: img_idx must be (N, 2), point_batch (N,)")
    if img_idx.device != src.device or point_batch.device != src.device:
        raise ValueError(f"{who}: the point indices live on another device than src")
    return n


class _AffineLift(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, theta, img_idx, point_batch, H, W):
        L = _lib.load()
        b, c, ih, iw, strides = _affine_operands(src, theta, "affine_lift")
        n = _affine_points(img_idx, point_batch, src, "affine_lift")
        out = _empty((n, c), F32, src)
        check(L.ftx_affine_lift_fwd(ptr(src), strides, b, c, ih, iw, ptr(theta), ptr(img_idx), ptr(point_batch), n, H, W, ptr(out), stream()),
              "ftx_affine_lift_fwd")
        ctx.save_for_backward(src, theta, img_idx, point_batch)
        ctx.size = (H, W)
        return out

    @staticmethod
    def backward(ctx, go):
        L = _lib.load()
        src, theta, img_idx, point_batch = ctx.saved_tensors
        H, W = ctx.size
        b, c, ih, iw, strides = _affine_operands(src, theta, "affine_lift")
        n = img_idx.shape[0]
        go = req(go.contiguous(), F32, "affine_lift grad", 2)
        if go.shape != (n, c):
            raise ValueError("affine_lift: gradient shape differs from the output's")
        want_src, want_theta = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gs = gt = seg = None
        if want_src:
            # theta is data: the sort of the points by source cell belongs to this call alone (nothing to share between taps or to prefetch)
            cells = _empty((n,), I32, point_batch)
            check(L.ftx_affine_lift_cells(ptr(theta), ptr(img_idx), ptr(point_batch), n, b, ih, iw, H, W, ptr(cells), stream()),
                  "ftx_affine_lift_cells")
            seg = Segments(cells, b * (ih + 1) * (iw + 1))
            gs = torch.empty_strided(src.shape, src.stride(), dtype=F32, device=src.device)
        ws_bytes = 0
        if want_theta:
            gt = _empty((b, 2, 3), F32, theta)
            ws_bytes = _ws_bytes("ftx_affine_theta_workspace_bytes", b)
        ws = _scratch(ws_bytes, theta) if want_theta else None
        if want_src or want_theta:
            check(L.ftx_affine_lift_bwd(ptr(src), strides, b, c, ih, iw, ptr(theta), ptr(img_idx), ptr(point_batch), ptr(go), n, H, W,
                                        ptr(seg.order) if seg is not None else 0, ptr(seg.seg_off) if seg is not None else 0,
                                        ptr(gs), ptr(gt), ptr(ws), ws_bytes, stream()), "ftx_affine_lift_bwd")
        return gs, gt, None, None, None, None


def affine_lift(src, theta, img_idx, point_batch, H, W):
    """The rows affine_sample(src, theta, (H, W))[point_batch, :, row, col] for img_idx (N, 2) int64 (row, col), bit for bit, without
    the (H, W) map: (N, c).  A point whose frame or pixel is out of range gives a zero row and takes no gradient.  Differentiable in
    src (same strides as src, every element written; the points are sorted by source cell inside the backward) and in theta; no
    float atomics, so both gradients repeat bit for bit."""
    H, W = _affine_size(H, W, "affine_lift")
    return _AffineLift.apply(src, theta, img_idx, point_batch, H, W)


# ---------------------------------------------------------------- the spatial transformers' localisation net
LOC_LAYERS = ((7, 8), (5, 90))     # the (k, co) csrc/ftx_stn_loc.hip serves: Conv2d(C, 8, 7) and Conv2d(8, 90, 5)


def _loc_operands(x, weight, bias, who):
    """(b, c, ih, iw, k, co, ph, pw, host stride array) of a strided float32 input and its contiguous Conv2d parameters, checked before
    anything is launched."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"{who} x: expected a CUDA (HIP) tensor; the product path has no CPU fallback")
    if x.dtype != F32 or x.dim() != 4:
        raise ValueError(f"{who} x: expected a 4-d float32 tensor, got {x.dtype} {tuple(x.shape)}")
    b, c, ih, iw = x.shape
    if min(b, c, ih, iw) < 1 or b > 128:
        raise ValueError(f"{who} x: empty tensor or more than 128 frames: {tuple(x.shape)}")
    if any(st <= 0 and sz > 1 for st, sz in zip(x.stride(), x.shape)):
        raise ValueError(f"{who} x: strides {x.stride()} alias elements")
    req(weight, F32, who + " weight", 4)
    co, cw, k, k2 = weight.shape
    if cw != c or k != k2 or (k, co) not in LOC_LAYERS:
        raise ValueError(f"{who} weight: expected (co, {c}, k, k) with (k, co) one of {LOC_LAYERS}, got {tuple(weight.shape)}")
    if bias is not None:
        req(bias, F32, who + " bias", 1)
        if bias.shape[0] != co:
            raise ValueError(f"{who} bias: expected ({co},), got {tuple(bias.shape)}")
    if weight.device != x.device or (bias is not None and bias.device != x.device):
        raise ValueError(f"{who}: x and the parameters live on different devices")
    ph, pw = (ih - k + 1) // 2, (iw - k + 1) // 2
    if ph < 1 or pw < 1:
        raise ValueError(f"{who}: a {ih} x {iw} input has no pooled pixel under a {k} x {k} kernel")
    return b, c, ih, iw, k, co, ph, pw, (ctypes.c_int64 * 4)(*x.stride())


class _LocConvPoolRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mean):
        L = _lib.load()
        b, c, ih, iw, k, co, ph, pw, strides = _loc_operands(x, weight, bias, "loc_conv_pool_relu")
        sel = _empty((b, co, ph, pw), torch.int8, x)
        if mean:
            out = _empty((b, co), F32, x)
            ws_bytes = _ws_bytes("ftx_loc_conv_pool_relu_fwd_workspace_bytes", b, co, ph, pw)
            ws = _scratch(ws_bytes, x)
            check(L.ftx_loc_conv_pool_relu_fwd(ptr(x), strides, b, c, ih, iw, ptr(weight), ptr(bias), k, co, 0, ptr(sel), ptr(out), ptr(ws),
                                               ws_bytes, stream()), "ftx_loc_conv_pool_relu_fwd")
        else:
            out = _empty((b, co, ph, pw), F32, x)
            check(L.ftx_loc_conv_pool_relu_fwd(ptr(x), strides, b, c, ih, iw, ptr(weight), ptr(bias), k, co, ptr(out), ptr(sel), 0, 0, 0,
                                               stream()), "ftx_loc_conv_pool_relu_fwd")
        # x, the pooled output (the mean form: the (b, co) row) and the routing bytes; the un-pooled map never existed
        ctx.save_for_backward(x, weight, bias, out, sel)
        ctx.mean = bool(mean)
        ctx.mark_non_differentiable(sel)
        return out, sel

    @staticmethod
    def backward(ctx, go, _gsel):
        L = _lib.load()
        x, weight, bias, out, sel = ctx.saved_tensors
        b, c, ih, iw, k, co, ph, pw, strides = _loc_operands(x, weight, bias, "loc_conv_pool_relu")
        if go.shape != out.shape:
            raise ValueError("loc_conv_pool_relu: gradient shape differs from the output's")
        if ctx.mean:   # d mean / d pooled = 1 / (ph pw) everywhere: a (b, co) row read with zero strides, no (b, co, ph, pw) tensor
            go = req((go * (1.0 / (ph * pw))).contiguous(), F32, "loc_conv_pool_relu grad", 2)
            gstrides = (ctypes.c_int64 * 4)(co, 1, 0, 0)
        else:
            go = req(go.contiguous(), F32, "loc_conv_pool_relu grad", 4)
            gstrides = (ctypes.c_int64 * 4)(*go.stride())
        gx = gw = gb = None
        if ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2]):
            gw, gb = torch.empty_like(weight), _empty((co,), F32, weight)
            ws_bytes = _ws_bytes("ftx_loc_conv_pool_relu_bwd_weight_workspace_bytes", b, c, ih, iw, k, co)
            ws = _scratch(ws_bytes, x)
            check(L.ftx_loc_conv_pool_relu_bwd_weight(ptr(x), strides, b, c, ih, iw, ptr(sel), ptr(go), gstrides, k, co, ptr(gw), ptr(gb),
                                                      ptr(ws), ws_bytes, stream()), "ftx_loc_conv_pool_relu_bwd_weight")
            if bias is None:
                gb = None
        if ctx.needs_input_grad[0]:   # skipped for stn_down: its x is the image
            gx = torch.empty_strided(x.shape, x.stride(), dtype=F32, device=x.device)
            check(L.ftx_loc_conv_pool_relu_bwd_data(ptr(weight), ptr(sel), ptr(go), gstrides, b, c, ih, iw, k, co, ptr(gx), strides, stream()),
                  "ftx_loc_conv_pool_relu_bwd_data")
        return gx, gw, gb, None


def loc_conv_pool_relu(x, weight, bias=None, mean=False, return_sel=False):
    """relu(max_pool2d(conv2d(x, weight, bias), 2, 2)) of a stride-1, unpadded Conv2d(C, 8, 7) or Conv2d(8, 90, 5) on csrc/ftx_stn_loc.hip:
    x (b, c, ih, iw) float32 of any non-aliasing strides, NCHW result (b, co, ph, pw); mean=True returns its spatial mean (b, co)
    instead, without the map.  Differentiable in x (same strides as x), weight and bias; exact float32, no float atomics, every output
    repeats bit for bit.  return_sel adds the int8 routing map (position 0..3 of each window's maximum, -1 where the ReLU is dead)."""
    out, sel = _LocConvPoolRelu.apply(x, weight, bias, bool(mean))
    return (out, sel) if return_sel else out


# ---------------------------------------------------------------- LayerNorm (+ the residual add in front of it)
def layer_norm_supported(x: torch.Tensor) -> bool:
    return x.is_cuda and x.dtype == F32 and x.shape[-1] % 256 == 0 and 256 <= x.shape[-1] <= 1024


def _ln_forward(x, y, weight, bias, eps, y_bias=None):
    L = _lib.load()
    shape = x.shape
    c = shape[-1]
    if y is not None and (not isinstance(y, torch.Tensor) or y.numel() != x.numel() or y.shape[-1] != c):
        raise ValueError("add_layer_norm: x and y differ in shape")
    x2 = req(x.contiguous().view(-1, c), F32, "layer_norm x", 2)
    y2 = req(y.contiguous().view(-1, c), F32, "layer_norm y", 2) if y is not None else None
    for t, nm in ((weight, "weight"), (bias, "bias"), (y_bias, "y_bias")):
        if t is None and nm == "y_bias":
            continue
        req(t, F32, "layer_norm " + nm, 1)
        if t.shape[0] != c:
            raise ValueError("layer_norm: parameter length != row length")
    if y_bias is not None and y2 is None:
        raise ValueError("add_layer_norm: y_bias without y")
    rows = x2.shape[0]
    h = torch.empty_like(x2)
    s = torch.empty_like(x2) if y2 is not None else x2
    stats = _empty((2, rows), F32, x2)               # row 0: mean, row 1: 1 / sqrt(var + eps)
    check(L.ftx_add_layernorm_fwd(ptr(x2), ptr(y2), ptr(y_bias), ptr(weight), ptr(bias), float(eps), rows, c, ptr(s) if y2 is not None else 0, ptr(h),
                                  stats.data_ptr(), stats.data_ptr() + 4 * rows, stream()), "ftx_add_layernorm_fwd")
    return s, h, stats, shape


def _ln_backward(gh, gs, s, weight, stats, with_y_bias=False):
    L = _lib.load()
    rows, c = s.shape
    gh = req(gh.contiguous().view(rows, c), F32, "layer_norm grad", 2)
    gs = req(gs.contiguous().view(rows, c), F32, "layer_norm residual grad", 2) if gs is not None else None
    gx = torch.empty_like(s)
    gparams = _empty((3 if with_y_bias else 2, c), F32, s)      # d gamma, d beta (, d y_bias)
    ws_bytes = _ws_bytes("ftx_layernorm_bwd_workspace_bytes", rows, c)
    ws = _scratch(ws_bytes, s)
    check(L.ftx_add_layernorm_bwd(ptr(gh), ptr(gs), ptr(s), ptr(weight), stats.data_ptr(), stats.data_ptr() + 4 * rows, rows, c, int(with_y_bias),
                                  ptr(gx), ptr(gparams), ptr(ws), ws_bytes, stream()), "ftx_add_layernorm_bwd")
    return gx, gparams


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        s, h, stats, shape = _ln_forward(x, None, weight, bias, eps)
        ctx.save_for_backward(s, weight, stats)
        ctx.shape = shape
        return h.view(shape)

    @staticmethod
    def backward(ctx, gh):
        s, weight, stats = ctx.saved_tensors
        gx, gparams = _ln_backward(gh, None, s, weight, stats)
        return gx.view(ctx.shape), gparams[0], gparams[1], None


class _AddLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, y_bias, weight, bias, eps):
        s, h, stats, shape = _ln_forward(x, y, weight, bias, eps, y_bias)
        ctx.save_for_backward(s, weight, stats)
        ctx.shape, ctx.with_y_bias = shape, y_bias is not None
        return s.view(shape), h.view(shape)

    @staticmethod
    def backward(ctx, gs, gh):
        s, weight, stats = ctx.saved_tensors            # autograd hands an unused output's gradient over as zeros: gs and gh are tensors
        gx, gparams = _ln_backward(gh, gs, s, weight, stats, ctx.with_y_bias)
        gx = gx.view(ctx.shape)
        return gx, gx, (gparams[2] if ctx.with_y_bias else None), gparams[0], gparams[1], None


def layer_norm(x, weight, bias, eps=1e-5):
    """nn.LayerNorm over the last dimension (256 / 512 / 768 / 1024 floats per row)."""
    return _LayerNorm.apply(x, weight, bias, eps)


def add_layer_norm(x, y, weight, bias, eps=1e-5, y_bias=None):
    """(s, LayerNorm(s)) with s = x + y in one pass; the backward returns one gradient for both addends: the residual gradient plus the
    LayerNorm's input gradient, written once.  `y_bias`: y is a Linear's output computed WITHOUT its bias, s = x + (y + y_bias); the
    bias gradient then comes out of the same backward pass (no column-sum launches for that Linear)."""
    return _AddLayerNorm.apply(x, y, y_bias, weight, bias, eps)


# ---------------------------------------------------------------- column sums (bias gradients)
def colsum(x: torch.Tensor) -> torch.Tensor:
    """x (rows, cols) float32 -> (cols,) column sums (float64 accumulation, fixed order): the bias gradient of a Linear."""
    L = _lib.load()
    x = req(x.contiguous(), F32, "colsum x", 2)
    rows, cols = x.shape
    out = _empty((cols,), F32, x)
    ws_bytes = _ws_bytes("ftx_colsum_workspace_bytes", rows, cols)
    ws = _scratch(ws_bytes, x)
    check(L.ftx_colsum(ptr(x), rows, cols, ptr(out), ptr(ws), ws_bytes, stream()), "ftx_colsum")
    return out


# ---------------------------------------------------------------- ViT self-attention
# (forward entry, its launch-log kind, backward entry, its kind) per operand mode (FP32 == False and BF16 == True, as ever)
_ATTENTION = {FP32: ("ftx_attn_fwd_tiled", "attn_fwd", "ftx_attn_bwd_tiled", "attn_bwd"),
              BF16: ("ftx_attn_fwd_bf16", "attn_fwd_bf16", "ftx_attn_bwd_bf16", "attn_bwd_bf16"),
              SPLIT: ("ftx_attn_fwd_split", "attn_fwd_split", "ftx_attn_bwd_split", "attn_bwd_split")}


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, scale, tiling=(0, 0), bf16=False):
        L = _lib.load()
        fn, kind = _ATTENTION[bf16][:2]
        qkv = req(qkv.contiguous(), F32, "attention qkv", 5)
        b, t, three, h, d = qkv.shape
        if three != 3 or d != 64:
            raise ValueError(f"attention: qkv must be (B, T, 3, heads, 64), got {tuple(qkv.shape)}")
        out = _empty((b, t, h * d), F32, qkv)
        lse = _empty((b, h, t), F32, qkv)
        qw, split = int(tiling[0]), int(tiling[1])
        _log_launch(kind, dict(b=b, t=t, h=h, d=d, products=2), lambda: check(getattr(L, fn)(
            ptr(qkv), b, t, h, d, float(scale), ptr(out), ptr(lse), qw, split, stream()), fn))
        ctx.save_for_backward(qkv, out, lse)
        ctx.scale, ctx.tiling, ctx.bf16 = float(scale), (qw, split), bf16
        return out

    @staticmethod
    def backward(ctx, go):
        L = _lib.load()
        fn, kind = _ATTENTION[ctx.bf16][2:]
        qkv, out, lse = ctx.saved_tensors
        b, t, _, h, d = qkv.shape
        go = req(go.contiguous(), F32, "attention grad", 3)
        gqkv = torch.empty_like(qkv)
        ws_bytes = int(L.ftx_attn_bwd_workspace_bytes(b, t, h))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=qkv.device)
        _log_launch(kind, dict(b=b, t=t, h=h, d=d, products=7), lambda: check(getattr(L, fn)(
            ptr(qkv), ptr(out), ptr(go), ptr(lse), b, t, h, d, ctx.scale, ptr(gqkv), ptr(ws), ws_bytes, ctx.tiling[0], ctx.tiling[1], stream()), fn))
        return gqkv, None, None, None


def attention(qkv, scale, tiling=(0, 0), bf16=False, operands=None):
    """softmax(Q K^T * scale) V for qkv (B, T, 3, heads, 64) -> (B, T, heads*64).  `tiling` = (waves per block, key groups) of the
    kernels, (0, 0) = chosen per launch (ftx_attn_fwd_tiled in include/ftx.h): a per-call argument for tests and tools.
    bf16=True: the bf16-operand kernels (ftx_attn_fwd_bf16 / ftx_attn_bwd_bf16: Q, K, V, dO, P and dS rounded to bf16 as MFMA
    operands, fp32 accumulation, softmax statistics and storage; the contract is stated in include/ftx.h).
    operands="split": the fp32-accurate kernels on the bf16 MFMA (ftx_attn_fwd_split / ftx_attn_bwd_split: every MFMA operand in three
    bf16 pieces, six piece products; contract in include/ftx.h); its tilings are those ftx_attn_split_tiling_built reports.  `bf16`,
    `operands` name the mode as for the sparse ops (operand_mode): bf16=True next to operands="split" is refused."""
    return _Attention.apply(qkv, scale, tiling, operand_mode(bf16, operands))


# ---------------------------------------------------------------- bf16-operand ViT Linears
# Epilogues of ftx_dense_gemm_bf16 (include/ftx.h FTX_EPI_*)
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU = 0, 1, 2, 3
# modes of the kernels; the mode is the C entries' suffix.  "bf16": operands rounded to bf16.  "split": every operand split into three
# bf16 pieces, six piece products summed in fp32 (fp32-class accuracy; the contract is stated in include/ftx.h).
_DENSE_MODES = ("bf16", "split")


def vit_linear_supported(x, weight):
    """True when the ftx_dense_* kernels take this Linear in both directions: fp32 CUDA tensors, in and out features multiples of 64
    (each is the reduction of one GEMM), rows at most 2^30."""
    n, k = weight.shape
    return (x.is_cuda and weight.is_cuda and x.dtype == F32 and weight.dtype == F32 and x.shape[-1] == k and k % 64 == 0 and n % 64 == 0
            and x.numel() // k <= (1 << 30))


def _dense_gemm(a, w, w_kn, epi, bias=None, pre_in=None, with_pre=False, mode="bf16"):
    """ftx_dense_gemm_bf16 (mode "bf16") or ftx_dense_gemm_split (mode "split"): a (m, kr) times W ((n, kr) for w_kn = 0, (kr, n) for
    w_kn = 1) -> (out, pre_out or None), fp32."""
    L = _lib.load()
    m, kr = a.shape
    n = w.shape[1] if w_kn else w.shape[0]
    _channel_operands(a, n, "vit " + mode + " gemm", optional=("bias",), bias=bias)
    out = _empty((m, n), F32, a)
    pre = _empty((m, n), F32, a) if with_pre else None
    _log_launch("vit_gemm_" + mode, dict(m=m, n=n, k=kr, w_kn=w_kn, epi=epi), lambda: check(getattr(L, "ftx_dense_gemm_" + mode)(
        ptr(a), ptr(w), w_kn, ptr(bias), ptr(pre_in), m, n, kr, epi, ptr(out), ptr(pre), stream()), "ftx_dense_gemm_" + mode))
    return out, pre


def _dense_wgrad(g, x, mode="bf16"):
    """ftx_dense_wgrad_bf16 / ftx_dense_wgrad_split: dW (n, k) = g (m, n)^T x (m, k)."""
    L = _lib.load()
    m, n = g.shape
    k = x.shape[1]
    dw = _empty((n, k), F32, g)
    ws_bytes = _ws_bytes(f"ftx_dense_wgrad_{mode}_workspace_bytes", m, n, k)
    ws = _scratch(ws_bytes, g)
    _log_launch("vit_wgrad_" + mode, dict(m=m, n=n, k=k), lambda: check(getattr(L, "ftx_dense_wgrad_" + mode)(
        ptr(g), ptr(x), m, n, k, ptr(dw), ptr(ws), ws_bytes, stream()), "ftx_dense_wgrad_" + mode))
    return dw


def dense_tile(mode, form, m, n, k):
    """(tile rows, tile columns, row splits) that ftx_dense_gemm_<mode> (form 0) or ftx_dense_wgrad_<mode> (form 1) picks: host only."""
    entry = f"ftx_dense_{mode}_tile"
    tm, tn, sp = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    check(getattr(_lib.load(), entry)(form, m, n, k, ctypes.byref(tm), ctypes.byref(tn), ctypes.byref(sp)), entry)
    return tm.value, tn.value, sp.value


# the per-family names the tests and callers written before dense_tile use
dense_bf16_tile = functools.partial(dense_tile, "bf16")
dense_split_tile = functools.partial(dense_tile, "split")


class _VitLinear(torch.autograd.Function):
    """y = x W^T (+ b) on ftx_dense_gemm_bf16; dX on the same kernel with W in the reduction-strided orientation, dW on
    ftx_dense_wgrad_bf16, the bias gradient on ftx_colsum.  Operands rounded to bf16 as they are staged, everything else fp32.
    mode "split": the same node on ftx_dense_gemm_split / ftx_dense_wgrad_split (three-piece operands, fp32-class results)."""

    @staticmethod
    def forward(ctx, x, w, b, mode="bf16"):
        x2 = req(x.reshape(-1, x.shape[-1]).contiguous(), F32, "vit_linear x", 2)
        w = req(w.contiguous(), F32, "vit_linear weight", 2)
        y, _ = _dense_gemm(x2, w, 0, EPI_BIAS if b is not None else EPI_NONE, bias=b, mode=mode)
        ctx.save_for_backward(x2, w)
        ctx.in_shape, ctx.has_bias, ctx.mode = x.shape, b is not None, mode
        return y.view(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        mode = ctx.mode
        dy2 = req(dy.reshape(-1, dy.shape[-1]).contiguous(), F32, "vit_linear grad", 2)
        dx = _dense_gemm(dy2, w, 1, EPI_NONE, mode=mode)[0].view(ctx.in_shape) if ctx.needs_input_grad[0] else None
        dw = _dense_wgrad(dy2, x2, mode) if ctx.needs_input_grad[1] else None
        db = colsum(dy2) if ctx.has_bias and ctx.needs_input_grad[2] else None
        return dx, dw, db, None


class _VitMlp(torch.autograd.Function):
    """fc2(gelu(fc1(x))) as one node: fc1 with the BIAS_GELU epilogue (writes the pre-activation and its GELU), fc2 with BIAS or NONE;
    backward: fc2's dX with the DGELU epilogue IS fc1's output gradient, so no GELU-backward pass runs.  mode as _VitLinear."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, mode="bf16"):
        x2 = req(x.reshape(-1, x.shape[-1]).contiguous(), F32, "vit_mlp x", 2)
        w1 = req(w1.contiguous(), F32, "vit_mlp fc1 weight", 2)
        w2 = req(w2.contiguous(), F32, "vit_mlp fc2 weight", 2)
        _channel_operands(x2, w2.shape[0], "vit_mlp", optional=("b2",), b2=b2)      # before fc1 is launched, not between the two GEMMs
        h, pre = _dense_gemm(x2, w1, 0, EPI_BIAS_GELU, bias=b1, with_pre=True, mode=mode)
        y, _ = _dense_gemm(h, w2, 0, EPI_BIAS if b2 is not None else EPI_NONE, bias=b2, mode=mode)
        ctx.save_for_backward(x2, w1, pre, h, w2)
        ctx.in_shape, ctx.has_b2, ctx.mode = x.shape, b2 is not None, mode
        return y.view(*x.shape[:-1], w2.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w1, pre, h, w2 = ctx.saved_tensors
        mode = ctx.mode
        dy2 = req(dy.reshape(-1, dy.shape[-1]).contiguous(), F32, "vit_mlp grad", 2)
        dpre, _ = _dense_gemm(dy2, w2, 1, EPI_DGELU, pre_in=pre, mode=mode)
        dw2 = _dense_wgrad(dy2, h, mode) if ctx.needs_input_grad[3] else None
        db2 = colsum(dy2) if ctx.has_b2 and ctx.needs_input_grad[4] else None
        dx = _dense_gemm(dpre, w1, 1, EPI_NONE, mode=mode)[0].view(ctx.in_shape) if ctx.needs_input_grad[0] else None
        dw1 = _dense_wgrad(dpre, x2, mode) if ctx.needs_input_grad[1] else None
        db1 = colsum(dpre) if ctx.needs_input_grad[2] else None
        return dx, dw1, db1, dw2, db2, None


def vit_linear(x, w, b=None, bf16=True, mode="bf16"):
    """x W^T (+ b) for a ViT Linear (x (..., K), w (N, K) as nn.Linear).  bf16=True on a shape the kernels take
    (vit_linear_supported): the ftx_dense_* kernels -- x, w and (backward) dy rounded to bf16 as MFMA operands, fp32 accumulation,
    fp32 output, bias and gradients (include/ftx.h).  Any other call runs the library path the model ran before
    (models/transformers._LinearFn, with bf16 the library bf16 GEMMs).
    mode="split": the three-piece split kernels (ftx_dense_gemm_split / ftx_dense_wgrad_split: fp32-class results on the bf16 MFMA);
    `bf16` is then ignored, and a shape the kernels do not take runs the FP32 library path (_LinearFn(..., False))."""
    if mode not in _DENSE_MODES:
        raise ValueError(f"vit_linear mode must be 'bf16' or 'split', got {mode!r}")
    if (mode == "split" or bf16) and vit_linear_supported(x, w):
        return _VitLinear.apply(x, w, b, mode)
    from .models.transformers import _LinearFn
    return _LinearFn.apply(x, w, b, mode != "split" and bool(bf16))


def vit_mlp(x, w1, b1, w2, b2=None, mode="bf16"):
    """fc2(gelu(fc1(x))) with exact GELU, bf16 operands and fp32 everything else, as one autograd node (see _VitMlp).  b2 None: fc2's
    bias is left to the caller (Block.chain).  Shapes the kernels do not take run the library bf16 path with nn.GELU().
    mode="split": the node on the three-piece split kernels; shapes they do not take run the fp32 library path."""
    if mode not in _DENSE_MODES:
        raise ValueError(f"vit_mlp mode must be 'bf16' or 'split', got {mode!r}")
    if (b1 is not None and vit_linear_supported(x, w1) and w2.is_cuda and w2.dtype == F32 and w2.shape[1] == w1.shape[0]
            and w2.shape[0] % 64 == 0):
        return _VitMlp.apply(x, w1, b1, w2, b2, mode)
    from .models.transformers import _LinearFn
    lib_bf16 = mode != "split"
    return _LinearFn.apply(torch.nn.functional.gelu(_LinearFn.apply(x, w1, b1, lib_bf16)), w2, b2, lib_bf16)


# ---------------------------------------------------------------- patch embedding and tap stems of the ViT in training
def _dense_mode(mode, who):
    if mode not in _DENSE_MODES:
        raise ValueError(f"{who} mode must be 'bf16' or 'split', got {mode!r}")
    return mode


def vit_patch_embed_supported(img, weight):
    """True when ftx_vit_patch_embed_* and its backward take this embedding: fp32 CUDA tensors, a square patch that is a multiple of 4,
    c patch patch and the width multiples of 64, whole patches."""
    from .vit_stems import vit_patch_embed_supported as supported
    return supported(img, weight)


def vit_patch_embed(img, weight, bias, cls, dist, pos, mode="split"):
    """The ViT's embedding as one node: tokens (b, t0 + g, dim) = [cls + pos[0], (dist + pos[1]), unfold(img) W^T + bias + pos[t0:]] for
    img (b, c, h, w), weight (dim, c, patch, patch) as nn.Conv2d keeps it, cls / dist (dim elements in any shape; dist None: t0 = 1) and
    pos ((t0 + g) dim elements), on the dense GEMM kernels of `mode` ("split" | "bf16", include/ftx.h).  Differentiable in every
    operand; the image gradient is computed only when img asks for it.  The bias gradient is ftx_colsum of the patch rows of d pos (the
    frames summed first): reproducible, and not the bits of a column sum over all b g rows."""
    from .vit_stems import _VitPatchEmbed
    return _VitPatchEmbed.apply(img, weight, bias, cls, dist, pos, _dense_mode(mode, "vit_patch_embed"))


def vit_tap_stem(tokens, weight, bias, t0=0, mode="split"):
    """The Conv1x1 -> ReLU of a tap stem on the token grid in training: rows (b g, co) = ReLU(tokens[:, t0:] W^T + bias) for tokens
    (b, t0 + g, dim) WITH their t0 leading (cls / dist) rows -- they are skipped by addressing, in the forward and in both gradients, and
    the gradient of the tokens comes back whole with those rows zero.  weight (co, dim) or (co, dim, 1, 1).  The BatchNorm behind it is
    functional.batch_norm on the rows.  mode "split" | "bf16" (include/ftx.h: ftx_vit_tap_stem_train_fwd_*, ftx_vit_tap_stem_bwd_*)."""
    from .vit_stems import _VitTapStem
    return _VitTapStem.apply(tokens, weight, bias, t0, _dense_mode(mode, "vit_tap_stem"))


# ---------------------------------------------------------------- fused sample_down
class _SampleDown(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, conv_w, conv_b, gamma, beta, running_mean, running_var, momentum, eps, training, oh, ow):
        L = _lib.load()
        img = req(img.contiguous(), F32, "sample_down img", 4)
        b, c, h, w = img.shape
        if c != 3 or conv_w.numel() != 9:
            raise ValueError("sample_down: the fused kernel is the 3 -> 3 channel BilinearModule of the reference")
        w_shape = conv_w.shape          # (3, 3), or (3, 3, 1, 1) as nn.Conv2d keeps it: the gradient goes back in that shape
        conv_w = req(conv_w.contiguous().view(3, 3), F32, "sample_down conv weight", 2)
        _channel_operands(img, 3, "sample_down", conv_b=conv_b, gamma=gamma, beta=beta, running_mean=running_mean, running_var=running_var)
        out = _empty((b, 3, int(oh), int(ow)), F32, img)
        saved = torch.empty((33,), dtype=torch.float64, device=img.device)
        ws_bytes = int(L.ftx_sample_down_workspace_bytes())
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=img.device)
        check(L.ftx_sample_down_fwd(ptr(img), b, h, w, int(oh), int(ow), ptr(conv_w), ptr(conv_b), ptr(gamma), ptr(beta), ptr(running_mean),
                                    ptr(running_var), float(momentum), float(eps), int(bool(training)), ptr(out), ptr(saved), ptr(ws), ws_bytes, stream()),
              "ftx_sample_down_fwd")
        ctx.save_for_backward(img, conv_w, conv_b, gamma, saved)
        ctx.training, ctx.w_shape = bool(training), w_shape
        ctx.dims = (b, h, w, int(oh), int(ow))
        return out

    @staticmethod
    def backward(ctx, go):
        L = _lib.load()
        if not ctx.training:
            raise RuntimeError("sample_down: backward is implemented for training-mode statistics only")
        img, conv_w, conv_b, gamma, saved = ctx.saved_tensors
        b, h, w, oh, ow = ctx.dims
        go = req(go.contiguous(), F32, "sample_down grad", 4)
        gw = _empty((3, 3), F32, go)
        gb, gg, gbeta = _empty((3,), F32, go), _empty((3,), F32, go), _empty((3,), F32, go)
        ws_bytes = int(L.ftx_sample_down_workspace_bytes())
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=go.device)
        check(L.ftx_sample_down_bwd(ptr(img), ptr(go), b, h, w, oh, ow, ptr(conv_w), ptr(conv_b), ptr(gamma), ptr(saved), ptr(gw), ptr(gb), ptr(gg),
                                    ptr(gbeta), ptr(ws), ws_bytes, stream()), "ftx_sample_down_bwd")
        return None, gw.view(ctx.w_shape), gb, gg, gbeta, None, None, None, None, None, None, None


def sample_down(img, conv_w, conv_b, gamma, beta, running_mean, running_var, momentum, eps, training, size):
    """Conv1x1(3->3) + ReLU + BatchNorm2d + nearest pick, fused (image_models_billinear.py:8-24).  Differentiable in the convolution's
    and the BatchNorm's parameters; img is the input image, and an img that asks for a gradient is refused."""
    _refuse_grad(img, "sample_down", "img", "the fused kernel is for the input image")
    return _SampleDown.apply(img, conv_w, conv_b, gamma, beta, running_mean, running_var, momentum, eps, training, size[0], size[1])


# ---------------------------------------------------------------- fused losses + metric
class _FusionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, l3, l2, l3b, l2b, label, class_weights, lambda_xm, conf3d, conf2d, ignore_index, ce_scale=1.0):
        # every operand is checked before anything is launched: the kernel reads C class weights, n rows of all four heads and
        # adds 64-bit counts into C x C cells of each matrix
        l3 = req(l3.contiguous(), F32, "loss lidar_seg_logit", 2)
        l2 = req(l2.contiguous(), F32, "loss img_seg_logit", 2)
        n, c = l3.shape
        if l2.shape != (n, c):
            raise ValueError("fusion_loss: img_seg_logit must be (%d, %d), got %s" % (n, c, tuple(l2.shape)))
        dual = l3b is not None or l2b is not None
        if dual:
            if l3b is None or l2b is None:
                raise ValueError("fusion_loss: the dual head needs both second heads")
            l3b = req(l3b.contiguous(), F32, "loss lidar_seg_logit2", 2)
            l2b = req(l2b.contiguous(), F32, "loss img_seg_logit2", 2)
            for t, name in ((l3b, "lidar_seg_logit2"), (l2b, "img_seg_logit2")):
                if t.shape != (n, c):
                    raise ValueError("fusion_loss: %s must be (%d, %d), got %s" % (name, n, c, tuple(t.shape)))
        label = req(label.contiguous(), I64, "loss label", 1)
        if label.shape[0] != n:
            raise ValueError("fusion_loss: label must have %d entries, got %d" % (n, label.shape[0]))
        if class_weights is not None:
            req(class_weights, F32, "loss class_weights", 1)
            if class_weights.shape[0] != c:
                raise ValueError("fusion_loss: class_weights must have %d entries, got %d" % (c, class_weights.shape[0]))
        for t, name in ((conf3d, "conf3d"), (conf2d, "conf2d")):
            if t is not None:
                req(t, I64, "fusion_loss " + name, 2)
                if tuple(t.shape) != (c, c):
                    raise ValueError("fusion_loss: %s must be (%d, %d), got %s" % (name, c, c, tuple(t.shape)))
        for t in (l2, l3b, l2b, label, class_weights, conf3d, conf2d):
            if t is not None and t.device != l3.device:
                raise ValueError("fusion_loss: every operand must be on %s" % l3.device)
        L = _lib.load()
        losses = _empty((2,), F32, l3)
        g3, g2 = torch.empty_like(l3), torch.empty_like(l2)
        g3b = torch.empty_like(l3) if dual else None
        g2b = torch.empty_like(l2) if dual else None
        ws_bytes = int(L.ftx_fusion_loss_workspace_bytes())
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=l3.device)
        check(L.ftx_fusion_loss_mix(ptr(l3), ptr(l2), ptr(l3b), ptr(l2b), ptr(label), ptr(class_weights), float(ce_scale), float(lambda_xm), n, c,
                                    int(ignore_index), ptr(losses), ptr(g3), ptr(g2), ptr(g3b), ptr(g2b), ptr(conf3d), ptr(conf2d), ptr(ws), ws_bytes,
                                    stream()), "ftx_fusion_loss_mix")
        ctx.save_for_backward(g3, g2, g3b, g2b) if dual else ctx.save_for_backward(g3, g2)
        ctx.dual = dual
        return losses

    @staticmethod
    def backward(ctx, g):
        # the kernel produced d(loss_2d + loss_3d); loss_2d depends only on (l2, l2b), loss_3d only on (l3, l3b)
        if ctx.dual:
            g3, g2, g3b, g2b = ctx.saved_tensors
            return g3 * g[1], g2 * g[0], g3b * g[1], g2b * g[0], None, None, None, None, None, None, None
        g3, g2 = ctx.saved_tensors
        if not torch.equal(g[0], g[1]):
            raise RuntimeError("fusion_loss (single head): loss_2d and loss_3d share logits; call backward on their sum")
        return g3 * g[0], g2 * g[0], None, None, None, None, None, None, None, None, None


def fusion_loss(preds, seg_label, class_weights, lambda_xm, dual_head, conf3d=None, conf2d=None, ignore_index=0, mix="additive"):
    """(loss_2d, loss_3d) in one fused pass; conf3d / conf2d (C,C) int64 tensors, when given, accumulate the SegIoU confusion
    matrices of models/metric.py:37-58.  mix="additive": CE + lambda*KL (SemanticTrainer.py:158-178); mix="torchpack":
    (1-lambda)*CE + lambda*KL when lambda > 0 (modules/SemanticTorchpackTrainer.py:70-106)."""
    if mix not in ("additive", "torchpack"):
        raise ValueError("fusion_loss: mix must be 'additive' or 'torchpack'")
    ce_scale = (1.0 - float(lambda_xm)) if (mix == "torchpack" and lambda_xm > 0) else 1.0
    out = _FusionLoss.apply(preds["lidar_seg_logit"], preds["img_seg_logit"], preds["lidar_seg_logit2"] if dual_head else None,
                            preds["img_seg_logit2"] if dual_head else None, seg_label.long(), class_weights, lambda_xm, conf3d, conf2d, ignore_index,
                            ce_scale)
    return out[0], out[1]


def _seg_loss_call(logit, label, class_weights, conf, ignore_index, want_grad):
    """Operand checks, then ftx_seg_loss.  Returns (0-dim loss, (n,c) gradient or None)."""
    # every operand is checked before anything is launched: the kernel reads C class weights and n rows, and adds 64-bit counts
    # into C x C cells of the matrix
    logit = req(logit.contiguous(), F32, "seg_loss logit", 2)
    n, c = logit.shape
    if not isinstance(label, torch.Tensor) or label.dim() != 1 or label.shape[0] != n:
        raise ValueError("seg_loss: seg_label must have %d entries, got shape %s" % (n, tuple(getattr(label, "shape", ()))))
    label = req(label.contiguous(), I64, "seg_loss seg_label", 1)
    if class_weights is not None:
        req(class_weights, F32, "seg_loss class_weights", 1)
        if class_weights.shape[0] != c:
            raise ValueError("seg_loss: class_weights must have %d entries, got %d" % (c, class_weights.shape[0]))
    if conf is not None:
        req(conf, I64, "seg_loss conf", 2)
        if tuple(conf.shape) != (c, c):
            raise ValueError("seg_loss: conf must be (%d, %d), got %s" % (c, c, tuple(conf.shape)))
    for t in (label, class_weights, conf):
        if t is not None and t.device != logit.device:
            raise ValueError("seg_loss: every operand must be on %s" % logit.device)
    L = _lib.load()
    loss = _empty((), F32, logit)
    grad = torch.empty_like(logit) if want_grad else None
    ws_bytes = int(L.ftx_seg_loss_workspace_bytes())
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=logit.device)
    check(L.ftx_seg_loss(ptr(logit), ptr(label), ptr(class_weights), n, c, int(ignore_index), ptr(loss), ptr(grad), ptr(conf), ptr(ws), ws_bytes,
                         stream()), "ftx_seg_loss")
    return loss, grad


class _SegLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, label, class_weights, conf, ignore_index):
        loss, grad = _seg_loss_call(logit, label, class_weights, conf, ignore_index, True)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None


def seg_loss(logit, seg_label, class_weights=None, conf=None, ignore_index=0):
    """Weighted-mean cross-entropy of ONE head, F.cross_entropy(logit, seg_label, weight=class_weights), as a 0-dim tensor: the loss
    of the LiDAR-only and image-only models (SemanticTrainer.py:180-186) and the per-batch validation loss (validate.py:122-128).
    conf (C,C) int64, when given, accumulates the SegIoU confusion matrix of models/metric.py:37-58.  Under torch.no_grad(), or for
    a logit that requires no gradient, the forward-only kernel runs and no (n, C) gradient buffer is allocated."""
    if isinstance(seg_label, torch.Tensor) and seg_label.dtype != I64 and not seg_label.dtype.is_floating_point:
        seg_label = seg_label.long()
    if torch.is_grad_enabled() and isinstance(logit, torch.Tensor) and logit.requires_grad:
        return _SegLoss.apply(logit, seg_label, class_weights, conf, ignore_index)
    return _seg_loss_call(logit, seg_label, class_weights, conf, ignore_index, False)[0]


def eval_scatter_back(logits3d, logits2d, inverse, gt, class_labels, conf3d=None, conf2d=None, conf_ens=None, want_preds=True):
    """Predictions of the model points mapped to the original points + confusion-matrix update in one kernel
    (reference data/utils/validate.py:62-120, data/utils/evaluate.py:12-26; see include/ftx.h).

    inverse (M,) int64: row of the model point of every original point (frame offset already added); gt (M,)
    learning ids; class_labels (C,) original id of every learning id.  conf_* are (C,C) int64 accumulators.
    Returns (pred_3d, pred_2d, pred_ens) in original label ids (None where not computed)."""
    L = _lib.load()
    ref = logits3d if logits3d is not None else logits2d
    if ref is None:
        raise ValueError("eval_scatter_back needs at least one logits tensor")
    for t, name in ((logits3d, "logits3d"), (logits2d, "logits2d")):
        if t is not None:
            req(t, F32, "eval_scatter_back " + name, 2)
    n, c = ref.shape
    if logits3d is not None and logits2d is not None and logits3d.shape != logits2d.shape:
        raise ValueError("eval_scatter_back: logits shapes differ")
    req(inverse, I64, "eval_scatter_back inverse", 1)
    gt = gt.to(I32).contiguous()
    req(gt, I32, "eval_scatter_back gt", 1)
    class_labels = class_labels.to(device=ref.device, dtype=I32).contiguous()
    if class_labels.numel() != c or gt.shape[0] != inverse.shape[0]:
        raise ValueError("eval_scatter_back: class_labels must have one id per class and gt one label per original point")
    m = inverse.shape[0]
    for t, name in ((conf3d, "conf3d"), (conf2d, "conf2d"), (conf_ens, "conf_ens")):
        if t is not None:
            req(t, I64, "eval_scatter_back " + name, 2)
            if tuple(t.shape) != (c, c):
                raise ValueError("eval_scatter_back: %s must be (%d, %d)" % (name, c, c))
    mk = (lambda cond: _empty((m,), I32, ref) if (want_preds and cond) else None)
    p3, p2, pe = mk(logits3d is not None), mk(logits2d is not None), mk(logits3d is not None and logits2d is not None)
    bad = torch.zeros((1,), dtype=I32, device=ref.device)
    check(L.ftx_eval_scatter_back(ptr(logits3d), ptr(logits2d), n, c, ptr(inverse), ptr(gt), m, ptr(class_labels), ptr(p3), ptr(p2), ptr(pe),
                                  ptr(conf3d), ptr(conf2d), ptr(conf_ens), ptr(bad), stream()), "ftx_eval_scatter_back")
    return p3, p2, pe, bad


# ---- colour jitter of the image-side augmentation (semantic_kitti_dataloader.py:196-212), csrc/ftx_image.hip ----
JITTER_OPS = {"brightness": 0, "contrast": 1, "saturation": 2, "hue": 3}


def _jitter_args(image: torch.Tensor, ops):
    """Host-side checks of a uint8 (H, W, 3) frame (a crop view with a row pitch is fine) and the packed op codes / factors."""
    if not isinstance(image, torch.Tensor) or not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 3:
        raise ValueError("color jitter: expected a (H, W, 3) uint8 CUDA tensor")
    h, w, c = image.shape
    if image.stride(2) != 1 or image.stride(1) != c or image.stride(0) < c * w:
        raise ValueError(f"color jitter: pixels must be packed within a row (strides {image.stride()})")
    ops = list(ops or [])
    codes = np.zeros(4, dtype=np.int32)
    factors = np.zeros(4, dtype=np.float64)
    if len(ops) > 4:
        raise ValueError("color jitter: at most 4 ops")
    for i, (op, f) in enumerate(ops):
        if op not in JITTER_OPS:
            raise ValueError(f"color jitter: unknown op {op!r}")
        codes[i], factors[i] = JITTER_OPS[op], float(f)
    vp = ctypes.c_void_p
    return (h, w, c, image.stride(0), codes.ctypes.data_as(vp), factors.ctypes.data_as(vp), len(ops),
            (codes, factors), any(op == "contrast" for op, _ in ops))


def _jitter_workspace(image, h, w, needed):
    if not needed:
        return 0, 0
    nbytes = _ws_bytes("ftx_color_jitter_workspace_bytes", h, w)
    return _carve(image, nbytes)[0], nbytes


def color_jitter_u8(image: torch.Tensor, ops) -> torch.Tensor:
    """ColorJitter's ops on a uint8 (H, W, 3) frame, bit-exact with Pillow: `ops` is the ordered list of (name, factor) that
    data.augment.draw_color_jitter returns (names: brightness, contrast, saturation, hue).  Returns a contiguous (H, W, 3) uint8."""
    L = _lib.load()
    h, w, c, pitch, codes, factors, n, keep, needs_ws = _jitter_args(image, ops)
    out = torch.empty((h, w, c), dtype=torch.uint8, device=image.device)
    ws, ws_bytes = _jitter_workspace(image, h, w, needs_ws)
    check(L.ftx_color_jitter_u8(ptr(image), pitch, h, w, c, codes, factors, n, ptr(out), ws, ws_bytes, stream()), "ftx_color_jitter_u8")
    return out


def color_jitter_to_chw(image: torch.Tensor, ops=None, flip=False, normalizer=None) -> torch.Tensor:
    """The same ops, fused with the conversion to the model's input: float32(u8) / 255 (correctly rounded, numpy's division), the
    optional left-right flip, (x - mean) / std with normalizer = (mean, std), HWC -> CHW.  Returns a (3, H, W) float32."""
    L = _lib.load()
    h, w, c, pitch, codes, factors, n, keep, needs_ws = _jitter_args(image, ops)
    out = torch.empty((c, h, w), dtype=torch.float32, device=image.device)
    mean = std = None
    if normalizer is not None:
        mean = np.ascontiguousarray(np.asarray(normalizer[0], dtype=np.float32).reshape(3))
        std = np.ascontiguousarray(np.asarray(normalizer[1], dtype=np.float32).reshape(3))
    vp = ctypes.c_void_p
    ws, ws_bytes = _jitter_workspace(image, h, w, needs_ws)
    check(L.ftx_color_jitter_chw(ptr(image), pitch, h, w, c, codes, factors, n, 1 if flip else 0,
                                 None if mean is None else mean.ctypes.data_as(vp), None if std is None else std.ctypes.data_as(vp),
                                 ptr(out), ws, ws_bytes, stream()), "ftx_color_jitter_chw")
    return out


# ---- image resize of the NuScenes loader (nuscenes_dataloader.py:185, Image.BILINEAR), csrc/ftx_resize.hip ----
_RESIZE_TABLES = {}


def resize_table(in_size: int, out_size: int, device):
    """Pillow's coefficient table of one axis (include/ftx.h) on `device`: (bounds (out, 2) int32, kk (out, ksize) int32, ksize).
    Computed on the host by ftx_resize_coeffs_host and uploaded once per (in, out, device); later calls return the same tensors."""
    device = torch.device(device)
    key = (int(in_size), int(out_size), device.index if device.index is not None else torch.cuda.current_device())
    hit = _RESIZE_TABLES.get(key)
    if hit is not None:
        return hit
    L = _lib.load()
    ksize = int(L.ftx_resize_ksize(key[0], key[1]))
    if ksize < 0:
        check(ksize, "ftx_resize_ksize")
    bounds = np.empty((key[1], 2), dtype=np.int32)
    kk = np.empty((key[1], ksize), dtype=np.int32)
    vp = ctypes.c_void_p
    check(L.ftx_resize_coeffs_host(key[0], key[1], bounds.ctypes.data_as(vp), kk.ctypes.data_as(vp)), "ftx_resize_coeffs_host")
    dev = torch.device("cuda", key[2])
    if len(_RESIZE_TABLES) >= 256:
        _RESIZE_TABLES.clear()
    hit = _RESIZE_TABLES[key] = (torch.from_numpy(bounds).to(dev), torch.from_numpy(kk).to(dev), ksize)
    return hit


def resize_bilinear_u8(image_u8: torch.Tensor, size) -> torch.Tensor:
    """PIL's `image.resize(size, Image.BILINEAR)` on a uint8 RGB frame, bit-exact with Pillow's 8-bit resample: image_u8 (H, W, 3), or a
    batch (B, H, W, 3) of equal-sized frames resized by the same launches; a crop view with a row pitch is fine (pixels packed within
    a row, as for the colour jitter).  size = (width, height), Pillow's order.  Returns a contiguous (height, width, 3) or
    (B, height, width, 3) uint8; both directions are supported.  When the size does not change the INPUT is returned, a view and
    not the copy Pillow makes.  The coefficient tables stay on the device (resize_table), so a stream of equal-sized frames makes no
    host-to-device copy and allocates the output only."""
    if not isinstance(image_u8, torch.Tensor) or not image_u8.is_cuda or image_u8.dtype != torch.uint8 or image_u8.dim() not in (3, 4):
        raise ValueError("resize_bilinear_u8: expected a (H, W, 3) or (B, H, W, 3) uint8 CUDA tensor")
    batched = image_u8.dim() == 4
    n = image_u8.shape[0] if batched else 1
    h, w, c = image_u8.shape[-3:]
    st = image_u8.stride()
    if c != 3 or st[-1] != 1 or st[-2] != c or st[-3] < c * w or (batched and st[0] < 0):
        raise ValueError(f"resize_bilinear_u8: 3 channels, pixels packed within a row (shape {tuple(image_u8.shape)}, strides {st})")
    ow, oh = (int(v) for v in size)
    if ow <= 0 or oh <= 0 or h <= 0 or w <= 0:
        raise ValueError(f"resize_bilinear_u8: sizes must be positive, got {(w, h)} -> {(ow, oh)}")
    if (ow, oh) == (w, h):
        return image_u8
    L = _lib.load()
    out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=image_u8.device)
    if n == 0:
        return out
    bx, kx, ksx = resize_table(w, ow, image_u8.device) if ow != w else (None, None, 0)
    by, ky, ksy = resize_table(h, oh, image_u8.device) if oh != h else (None, None, 0)
    nbytes = _ws_bytes("ftx_resize_workspace_bytes", n, h, w, oh, ow)
    ws = hold = 0
    if nbytes:
        if torch.cuda.is_current_stream_capturing():   # from the graph's pool; the kernels recorded below are ordered before its reuse
            hold = torch.empty((nbytes,), dtype=torch.uint8, device=image_u8.device)
            ws = hold.data_ptr()
        else:
            ws = _carve(image_u8, nbytes)[0]
    check(L.ftx_resize_bilinear_u8(ptr(image_u8), st[0] if batched else 0, st[-3], n, h, w, c, ptr(bx), ptr(kx), ksx, ptr(by), ptr(ky), ksy,
                                   oh, ow, ptr(out), ws, nbytes, stream()), "ftx_resize_bilinear_u8")
    return out if batched else out[0]


# ---------------------------------------------------------------- Dropout
# The counter-based Dropout of the library; the node and its wrappers live in dropout.py.
from .dropout import dropout, dropout_mask  # noqa: E402,F401
