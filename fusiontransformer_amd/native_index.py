"""Host side of the native index build of the SPVCNN LiDAR branch (include/ftx.h: ftx_spvcnn_index_levels / _maps / _pairs).

`index_steps` has the contract of SPVCNN._index_steps(x, ahead=True): a generator that yields "sync" exactly twice -- once before each of
the two host reads (all level sizes, then the five submanifold pair counts) -- and returns `(z, x0)` carrying the same structures the
per-op Python build leaves (CoordinateManager with coordinates, hash tables and KernelMaps; the PointTensor's point <-> voxel caches),
as views into three arenas, one torch allocation per phase.  The views hold the arenas, so reference counts give the lifetime and
sparse.PendingIndex's record_stream walk covers them.  Three library calls replace the ~110 launches through Python."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from . import functional as spf
from .native_eval import MAP, MAP_KEYS, PV, PV_STRIDES, STRIDES
from .sparse import CoordinateManager, HostRead, KernelMap, PointTensor, SparseTensor

_vp = ctypes.c_void_p
_DT = {"i32": (torch.int32, 4), "i64": (torch.int64, 8), "f32": (torch.float32, 4)}

# ftx_spvcnn_index_layout's words, in its order
WORDS = (["a_total", "b_total", "c_total", "a_coords", "a_points", "a_uniq", "a_first", "a_skeys", "a_order"]
         + [f"{k}{l}" for l in range(5) for k in ("coords", "tkeys", "tvals", "cap")] + ["x0"]
         + [f"{k}{m}" for m in range(9) for k in ("nbr", "pos", "koff")]
         + [f"{k}{m}" for m in range(5, 9) for k in ("pos_t", "pair_in", "pair_out")]
         + [f"{k}{j}" for j in range(3) for k in ("vidx", "vcnt", "vseg", "didx", "dw", "dorder", "dseg")]
         + [f"{k}{m}" for m in range(5) for k in ("pos_t", "pair_in", "pair_out")])


class Refused(Exception):
    """The library refused the batch before launching anything (its text is the message); the caller takes the per-op path."""


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _error():
    return _lib.load().ftx_last_error().decode("utf-8", "replace")


def layout(n, c_in, level_off=None, pair_counts=None, with_backward_segments=False):
    """{name: byte offset} of every array in its arena (host only; raises Refused for arguments the library refuses)."""
    L = _lib.load()
    n_words = int(L.ftx_spvcnn_index_layout_words())
    assert n_words == len(WORDS)
    words = np.zeros(n_words, dtype=np.int64)
    rc = L.ftx_spvcnn_index_layout(int(n), int(c_in), _np_ptr(level_off), _np_ptr(pair_counts), int(bool(with_backward_segments)), _np_ptr(words))
    if rc != 0:
        raise Refused(_error())
    return dict(zip(WORDS, (int(w) for w in words)))


def levels_arena_bytes(n):
    return int(_lib.load().ftx_spvcnn_index_levels_arena_bytes(int(n)))


def maps_arena_bytes(n, c_in, level_off, with_backward_segments=False):
    return int(_lib.load().ftx_spvcnn_index_maps_arena_bytes(int(n), int(c_in), _np_ptr(level_off), int(bool(with_backward_segments))))


def pairs_arena_bytes(n, level_off, pair_counts):
    return int(_lib.load().ftx_spvcnn_index_pairs_arena_bytes(int(n), _np_ptr(level_off), _np_ptr(pair_counts)))


def _view(arena, off, kind, *shape):
    dtype, size = _DT[kind]
    count = int(np.prod(shape)) if shape else 1
    return arena[off:off + count * size].view(dtype).view(*shape)


class _Read:
    """The pinned words one phase reports back; quacks like sparse.HostRead for PendingIndex (`ready`)."""

    def __init__(self, host):
        self.host = host
        self.event = torch.cuda.Event()
        self.event.record()
        HostRead.latest = self

    def ready(self):
        return self.event.query()

    def values(self, count):
        self.event.synchronize()
        return np.array(self.host[:count].tolist(), dtype=np.int32)


def _table(keys, vals, n, capacity):
    t = spf.HashTable.__new__(spf.HashTable)
    t.n, t.capacity, t.keys, t.vals = int(n), int(capacity), keys, vals
    return t


def _alloc(nbytes, device):
    return torch.empty((int(nbytes),), dtype=torch.uint8, device=device)


def index_steps(x, init_res, after_res, with_backward_segments=None):
    """SPVCNN._index_steps(x, ahead=True) through the library.  Raises Refused (before anything is launched) for a batch the library
    does not take; `with_backward_segments` defaults to the grad mode, as the per-op build decides."""
    L = _lib.load()
    if with_backward_segments is None:
        with_backward_segments = torch.is_grad_enabled()
    bwd = int(bool(with_backward_segments))
    coords = x.C
    if coords.dtype != torch.float32:
        coords = coords.float()
    coords = coords.contiguous()
    feats = x.F
    if not (torch.is_tensor(feats) and feats.is_cuda and coords.is_cuda and feats.dtype == torch.float32 and feats.dim() == 2
            and coords.dim() == 2 and coords.shape[1] == 4 and feats.shape[0] == coords.shape[0]):
        raise Refused("native index: (n, 4) coordinates and (n, c) float32 features on the GPU expected")
    feats_c = feats.contiguous()
    n, c_in = int(feats.shape[0]), int(feats.shape[1])
    dev = coords.device
    st = _lib.stream()
    ir, ar = float(init_res), float(after_res)
    if c_in < 4 or c_in % 4 or c_in > 1024:
        raise Refused("native index: the feature width must be a multiple of 4 in [4, 1024]")
    lay = layout(n, c_in)
    arena_a = _alloc(lay["a_total"], dev)
    pinned = torch.empty((16,), dtype=torch.int32, pin_memory=True)
    rc = L.ftx_spvcnn_index_levels(coords.data_ptr(), n, ir, ar, arena_a.data_ptr(), arena_a.shape[0], pinned.data_ptr(), st)
    if rc != 0:
        raise Refused(_error())
    read = _Read(pinned)
    yield "sync"
    level_off = read.values(6)
    try:
        lay = layout(n, c_in, level_off, None, bwd)
    except Refused as e:
        raise RuntimeError(f"native index: {e}") from None
    arena_b = _alloc(lay["b_total"], dev)
    pinned2 = torch.empty((16,), dtype=torch.int32, pin_memory=True)
    _lib.check(L.ftx_spvcnn_index_maps(coords.data_ptr(), n, ir, ar, feats_c.data_ptr(), c_in, _np_ptr(level_off), bwd, arena_a.data_ptr(), arena_a.shape[0],
                                       arena_b.data_ptr(), arena_b.shape[0], pinned2.data_ptr(), st), "ftx_spvcnn_index_maps")
    read = _Read(pinned2)
    yield "sync"
    pair_counts = read.values(5)
    try:
        lay = layout(n, c_in, level_off, pair_counts, bwd)
    except Refused as e:
        raise RuntimeError(f"native index: {e}") from None
    arena_c = _alloc(lay["c_total"], dev)
    rows = np.zeros(6, dtype=np.int64)
    maps = np.zeros(len(MAP_KEYS), dtype=MAP)
    pvs = np.zeros(len(PV_STRIDES), dtype=PV)
    _lib.check(L.ftx_spvcnn_index_pairs(n, c_in, _np_ptr(level_off), bwd, _np_ptr(pair_counts), arena_a.data_ptr(), arena_b.data_ptr(), arena_b.shape[0],
                                        arena_c.data_ptr(), arena_c.shape[0], _np_ptr(rows), _np_ptr(maps), _np_ptr(pvs), None, st), "ftx_spvcnn_index_pairs")
    return _structures(feats, coords, n, c_in, ir != ar, bwd, lay, level_off, pair_counts, arena_a, arena_b, arena_c, (rows, maps, pvs))


def _structures(feats, coords, n, c_in, rescaled, bwd, lay, level_off, pair_counts, A, B, C, tables):
    """(z, x0) as the per-op build leaves them, every tensor a view into the arenas."""
    sizes = [int(level_off[l + 1] - level_off[l]) for l in range(5)]
    points = _view(A, lay["a_points"], "i32", n, 4)
    uniq = _view(A, lay["a_uniq"], "i64", 5 * n)
    first = _view(A, lay["a_first"], "i32", 5 * n)
    skeys = _view(A, lay["a_skeys"], "i64", 5, n)
    order = _view(A, lay["a_order"], "i32", 5, n)
    cm = CoordinateManager()
    cm.points = points
    cm.level_data = {}
    for l, s in enumerate(STRIDES):
        lo, hi = int(level_off[l]), int(level_off[l + 1])
        cm.level_data[s] = (uniq[lo:hi], first[lo:hi], l, skeys[l], order[l])
        cm.coords[s] = _view(B, lay[f"coords{l}"], "i32", sizes[l], 4)
        cap = lay[f"cap{l}"]
        cm.tables[s] = _table(_view(B, lay[f"tkeys{l}"], "i64", cap), _view(B, lay[f"tvals{l}"], "i32", cap), sizes[l], cap)
    for m, key in enumerate(MAP_KEYS):
        ks, s, stride = key
        l = STRIDES.index(s)
        sub = stride == 1
        k, n_in, n_out = (27, sizes[l], sizes[l]) if sub else (8, sizes[l], sizes[l + 1])
        n_pairs = int(pair_counts[l]) if sub else n_in
        arena = C if sub else B
        cm.kernel_maps[key] = KernelMap(_view(B, lay[f"nbr{m}"], "i32", k, n_out), _view(B, lay[f"pos{m}"], "i32", k, n_out),
                                        _view(arena, lay[f"pos_t{m}"], "i32", k, n_in), _view(arena, lay[f"pair_in{m}"], "i32", n_pairs),
                                        _view(arena, lay[f"pair_out{m}"], "i32", n_pairs), _view(B, lay[f"koff{m}"], "i32", k + 1), n_pairs, n_in, n_out,
                                        cm.coords[s * stride], fine_bijective=not sub, submanifold=sub)
    zc = _view(A, lay["a_coords"], "f32", n, 4) if rescaled else coords
    z = PointTensor(feats, zc)
    af = z.additional_features
    af["vox_seg"], af["devox_seg"] = {}, {}
    for j, s in enumerate(PV_STRIDES):
        l = STRIDES.index(s)
        af["idx_query"][s] = _view(B, lay[f"vidx{j}"], "i32", n)
        af["counts"][s] = _view(B, lay[f"vcnt{j}"], "i32", sizes[l])
        af["vox_seg"][s] = spf.Segments.from_parts(order[l], _view(B, lay[f"vseg{j}"], "i32", sizes[l] + 1), sizes[l])
        z.idx_query[s] = _view(B, lay[f"didx{j}"], "i32", n, 8)
        z.weights[s] = _view(B, lay[f"dw{j}"], "f32", n, 8)
        af["devox_seg"][s] = spf.Segments.from_parts(_view(B, lay[f"dorder{j}"], "i32", 8 * n), _view(B, lay[f"dseg{j}"], "i32", sizes[l] + 1),
                                                     sizes[l]) if bwd else None
    x0 = SparseTensor(_view(B, lay["x0"], "f32", sizes[0], c_in), cm.coords[1], 1)
    x0.cm = cm
    x0.check()
    x0.native_tables = tables      # (rows, maps, pvs) as phase C wrote them: what ftx_spvcnn_eval reads
    return z, x0
