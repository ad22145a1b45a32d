"""Host side of the native training executor of the SPVCNN LiDAR branch (include/ftx.h: ftx_spvcnn_train_fwd / _bwd).

The program is native_eval's (the same walk, records, tables and routes), cut into five segments: a segment ends at each of the two
voxelisations that feed a Dropout, so Dropout stays torch's, with its RNG stream and the injected masks.  With the library's own
counter-based Dropout (SPVCNN.set_native_dropout; include/ftx.h: ftx_dropout) the two are ops of the program instead, which then runs
in the eval program's three segments through ftx_spvcnn_train_fwd_rng / _bwd_rng.  Each segment is ONE
autograd node (`_Segment`): its forward is one library call, its backward one library call that walks the segment's ops in reverse
and issues what the per-op nodes of functional.py issue.  Everything the backward reads lives in one arena per forward, allocated
from torch's allocator and freed when the graph dies."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from . import functional as spf
from . import native_eval as ne
from .models.spvcnn import step_counter
from .native_eval import Unsupported, _P, _ptr

TRAIN_LAYER = np.dtype([("dweight", _P), ("dbias", _P), ("dgamma", _P), ("dbeta", _P), ("momentum", "<f4"), ("reserved", "<i4")])
TRAIN_PV = np.dtype([("devox_order", _P), ("devox_seg_off", _P)])
SEGMENTS = (0, 1, 2, 3, 4)       # stem | encoder | z1 (+ middle addend) -> y1 | Dropout, up1, up2, z2 -> y3 | Dropout, up3, up4, z3
SEGMENTS_DROPOUT = (0, 1, 2, 2, 2)      # SPVCNN.set_native_dropout: Dropout is an op of the program, so stem | encoder | decoder as in eval
GRAD_FIELDS = ("dweight", "dbias", "dgamma", "dbeta")      # of the refs (weight, bias, gamma, beta) of a layer, in that order
_K, _SEG, _LAYER, _MAP, _SRC, _SRC2, _DST, _RELU, _LEVEL, _CH = range(10)     # fields of an op tuple


class Refused(Exception):
    """The library refused the batch's tables before its first launch; the caller takes the per-op path."""


def check_record_sizes():
    ne.check_record_sizes()
    L = _lib.load()
    assert int(L.ftx_spvcnn_train_layer_bytes()) == TRAIN_LAYER.itemsize and int(L.ftx_spvcnn_train_pv_bytes()) == TRAIN_PV.itemsize


def gradient_targets(op):
    """The slots the backward of `op` sends a gradient to, by operand (the input features need none)."""
    kind, src, src2 = op[_K], op[_SRC], op[_SRC2]
    out = []
    if kind in (ne.OP_CONV_BN, ne.OP_LINEAR_BN, ne.OP_VOXELIZE, ne.OP_DEVOXELIZE, ne.OP_CONCAT, ne.OP_ADD) and src != ne.SLOT_INPUT:
        out.append(src)
    if kind in (ne.OP_CONCAT, ne.OP_ADD) or (kind == ne.OP_CONV_BN and src2 >= 0):
        out.append(src2)
    return out


def saved_slots(op):
    """The slots the backward of `op` reads: what the per-op node saves (input and output of a layer; the index ops save no features)."""
    if op[_K] in (ne.OP_CONV_BN, ne.OP_LINEAR_BN):
        return [op[_SRC], op[_DST]]
    return []


class TrainProgram:
    """The training program of one SPVCNN: `program` (native_eval.Program with five segments, or -- native_dropout -- three and the two
    Dropouts as ops), `backward` (the op indices in the order
    the backward issues them), `contributions` (per slot the ops whose backward writes its gradient), `grad_table` (per parameter where
    its gradient goes: (layer, field of TRAIN_LAYER, (dict, name) of the parameter)) and the per-segment views of these."""

    def __init__(self, net, native_dropout=False):
        self.native_dropout = bool(native_dropout)
        if self.native_dropout:
            self.segments = SEGMENTS_DROPOUT
            self.program = P = ne.emit_program(net, segments=SEGMENTS_DROPOUT, dropout=True)
        else:
            self.segments = SEGMENTS
            self.program = P = ne.emit_program(net, segments=SEGMENTS)
        self.n_segments = len(set(self.segments))
        ops = P.ops
        self.backward = list(range(len(ops) - 1, -1, -1))
        self.contributions = {}
        for i, op in enumerate(ops):
            for s in gradient_targets(op):
                self.contributions.setdefault(s, []).append(i)
        for s, who in self.contributions.items():
            if len(who) > 2:       # a third term would make the sum depend on the order autograd adds in
                raise Unsupported(f"slot {s} would receive {len(who)} gradient contributions")
        writers = {}
        for i, op in enumerate(ops):
            writers.setdefault(op[_DST], []).append(i)
        self.saved = sorted({s for op in ops for s in saved_slots(op)})
        for i, op in enumerate(ops):       # ADD_EXT writes its slot in place: every op that saves that slot comes after it
            for s in saved_slots(op):
                if any(w > i for w in writers.get(s, [])):
                    raise Unsupported(f"slot {s} is written again after op {i} saved it")
        self.src_level = []
        level = {ne.SLOT_INPUT: 0}
        for op in ops:
            self.src_level.append(level[op[_SRC]])
            level[op[_DST]] = op[_LEVEL]
        self.grad_table, self.momentum, self.bns = [], [], []
        seg_of_layer = {}
        for op in ops:
            if op[_K] in (ne.OP_CONV_BN, ne.OP_LINEAR_BN):
                if op[_LAYER] in seg_of_layer:
                    raise Unsupported("a layer runs twice")
                seg_of_layer[op[_LAYER]] = op[_SEG]
        for li, l in enumerate(P.layers):
            bn = l["bn"]
            if bn.momentum is None:
                raise Unsupported("BatchNorm with a cumulative moving average")
            self.momentum.append(float(bn.momentum))
            self.bns.append(bn)
            for field, ref in zip(GRAD_FIELDS, l["refs"][:4]):
                if ref is not None:
                    self.grad_table.append((li, field, ref))
        # per segment: its parameters (the inputs of its autograd node after the features), where each gradient lies in the segment's
        # one flat gradient buffer, and its BatchNorm modules
        self.seg_params, self.seg_bns = [], []
        for s in range(self.n_segments):
            entries, off = [], 0
            for li, field, ref in self.grad_table:
                if seg_of_layer[li] != s:
                    continue
                shape = tuple(ref[0][ref[1]].shape)
                n = int(np.prod(shape))
                entries.append((li, field, ref, shape, off, n))
                off += n
            self.seg_params.append(dict(entries=entries, total=off, sizes=[e[5] for e in entries],
                                        fields={f: (np.array([e[0] for e in entries if e[1] == f], dtype=np.int64),
                                                    np.array([4 * e[4] for e in entries if e[1] == f], dtype=np.int64)) for f in GRAD_FIELDS}))
            self.seg_bns.append([self.bns[li] for li in sorted(seg_of_layer) if seg_of_layer[li] == s])
        self.in_slot, self.out_slot = [], []
        for s in range(self.n_segments):
            last = [op for op in ops if op[_SEG] == s][-1]
            self.out_slot.append(last[_DST])
            self.in_slot.append(ne.SLOT_INPUT if s == 0 else self.out_slot[s - 1])
        self.out_shape = [(op[_LEVEL], op[_CH]) for op in (next(o for o in reversed(ops) if o[_SEG] == s) for s in range(self.n_segments))]
        self.in_channels = [P.layers[ops[0][_LAYER]]["ca"]] + [c for _, c in self.out_shape[:-1]]

    def parameters(self):
        return [ref[0][ref[1]] for _, _, ref in self.grad_table]


def grad_routes(tp: TrainProgram, layers, rows, kms):
    """For every sparse convolution whose input needs a gradient the route of its data gradient (functional._conv_route(grad=True))."""
    out = np.full(len(tp.program.ops), -1, dtype=np.int32)
    for i, op in enumerate(tp.program.ops):
        if op[_K] == ne.OP_CONV_BN and op[_MAP] >= 0 and op[_SRC] != ne.SLOT_INPUT:
            l = layers[op[_LAYER]]
            out[i] = ne.ROUTES[spf._conv_route(kms[op[_MAP]], bool(l["transposed"]), int(l["co"]), int(l["ca"]), int(l["kvol"]),
                                               int(rows[tp.src_level[i]]), int(l["bf16"]), grad=True)]
    return out


def arena_bytes(layers, ops, rows, maps, pvs, routes, groutes) -> int:
    """ftx_spvcnn_train_arena_bytes of the tables (host only); raises Refused with the library's text for tables it refuses."""
    L = _lib.load()
    n = int(L.ftx_spvcnn_train_arena_bytes(_ptr(layers), len(layers), _ptr(ops), len(ops), _ptr(rows), _ptr(maps), len(maps), _ptr(pvs), len(pvs), _ptr(routes),
                                           _ptr(groutes)))
    if n == 0:
        raise Refused("ftx_spvcnn_train_arena_bytes: " + L.ftx_last_error().decode("utf-8", "replace"))
    return n


def _alias(storage, byte_offset, shape, device):
    """A float32 tensor over a piece of the arena that is NOT a view of it for autograd (its own version counter: Dropout may work in
    place on it while the nodes of other pieces hold theirs)."""
    return torch.empty(0, dtype=torch.float32, device=device).set_(storage, byte_offset // 4, shape)


class NativeTrain(ne._Host):
    """Per-module state of the training executor: the program and the model table.  Runs are per forward."""

    def __init__(self, net, native_dropout=False):
        check_record_sizes()
        self.tp = TrainProgram(net, native_dropout)
        super().__init__(self.tp.program)
        self.runs = 0              # forwards this executor ran (the tests' witness)
        self.last_arena_bytes = 0

    def trainable(self):
        return all(p.requires_grad for p in self.tp.parameters())

    def begin(self, z, x0, arena=None, rng=None):
        """Fill the tables of one batch and allocate its arena; raises Refused (nothing launched) for a batch the library does not take.
        arena (optional): nbytes -> a contiguous uint8 CUDA tensor of that many bytes, 256-byte aligned, to run in instead of a fresh
        torch.empty -- a view into a larger buffer is fine (the tests' guard bands).
        rng: (seed, call_base) of this forward's Dropout ops, for a program that holds them (SPVCNN.set_native_dropout), else None."""
        tp = self.tp
        if tp.native_dropout != (rng is not None):
            raise ValueError("native train: (seed, call_base) go with a program that holds Dropout ops, and only with it")
        try:
            layers = self.model_table()
        except Unsupported as e:
            raise Refused(str(e))
        try:
            rows, maps, pvs, routes, kms = ne.batch_tables(self.program, layers, z, x0)
        except (KeyError, AttributeError) as e:      # an index that was prepared without the structures built ahead
            raise Refused(f"the batch's index lacks {e}")
        groutes = grad_routes(tp, layers, rows, kms)
        need = arena_bytes(layers, self.ops, rows, maps, pvs, routes, groutes)
        tpvs = np.zeros(len(ne.PV_STRIDES), dtype=TRAIN_PV)
        segs = z.additional_features.setdefault("devox_seg", {})
        for r, s in zip(tpvs, ne.PV_STRIDES):
            if segs.get(s) is None:      # as utils.voxel_to_point: the backward of a devoxelise that needs a gradient is the sorted one
                segs[s] = spf.devoxelize_segments(z.idx_query[s], z.weights[s], int(rows[ne.STRIDES.index(s)]))
            r["devox_order"], r["devox_seg_off"] = segs[s].order.data_ptr(), segs[s].seg_off.data_ptr()
        tl = np.zeros(len(layers), dtype=TRAIN_LAYER)
        tl["momentum"] = tp.momentum
        feats = _lib.req(x0.F.contiguous(), torch.float32, "native train input features", 2)
        if arena is None:
            arena = torch.empty((need,), dtype=torch.uint8, device=feats.device)
        else:
            arena = _lib.req(arena(need), torch.uint8, "native train arena", 1)
            if arena.shape[0] != need or arena.data_ptr() % 256 or arena.device != feats.device:
                raise ValueError(f"native train: the arena must be {need} bytes on {feats.device}, 256-byte aligned")
        self.runs += 1
        self.last_arena_bytes = need
        return _Run(self, layers, tl, rows, maps, pvs, tpvs, routes, groutes, (kms, z, x0, segs), feats, arena, rng)


class _Run:
    """One forward and its backward: the batch tables, the arena, and how far either direction has come."""

    def __init__(self, ex, layers, tl, rows, maps, pvs, tpvs, routes, groutes, keep, feats, arena, rng=None):
        self.rng = rng                # (seed, call_base): the backward recomputes the masks from the pair the forward drew with
        self.ex, self.layers, self.tl, self.rows, self.maps, self.pvs, self.tpvs = ex, layers, tl, rows, maps, pvs, tpvs
        self.routes, self.groutes, self.keep, self.feats, self.arena = routes, groutes, keep, feats, arena
        self.storage = arena.untyped_storage()
        self.base = arena.data_ptr()
        self.origin = self.base - arena.storage_offset()      # the storage's first byte (uint8: elements are bytes); = base for a fresh arena
        self.forward_done = -1
        self.backward_next = None     # the segment whose backward comes next; None until the forward is complete, -1 when consumed

    def segment(self, seg, x, addend=None):
        """Segment `seg` on `x` (the previous segment's result, after Dropout where one sits between) as one autograd node."""
        sp = self.ex.tp.seg_params[seg]
        params = [ref[0][ref[1]] for _, _, ref, _, _, _ in sp["entries"]]
        return _Segment.apply(self, seg, x, addend, *params)

    def _forward(self, seg, x, addend):
        tp = self.ex.tp
        if seg != self.forward_done + 1:
            raise RuntimeError(f"native train: segment {seg} issued after segment {self.forward_done}")
        n_pts = int(self.rows[ne.POINTS])
        level, ch = tp.out_shape[seg]
        x = _lib.req(x.contiguous(), torch.float32, "native train segment input", 2)
        want = (int(self.rows[0 if seg == 0 else tp.out_shape[seg - 1][0]]), tp.in_channels[seg])
        if tuple(x.shape) != want:
            raise ValueError(f"native train: segment {seg} takes {want} features, got {tuple(x.shape)}")
        if addend is not None:
            addend = _lib.req(addend.contiguous(), torch.float32, "native train fusion addend", 2)
            if tuple(addend.shape) != (n_pts, tp.in_channels[seg]) or seg not in (1, 2):
                raise ValueError("native train: the fusion addend does not match the point features")
        live = [c for c in map(step_counter, tp.seg_bns[seg]) if c is not None]
        if live:
            torch._foreach_add_(live, 1)
        last = seg == tp.n_segments - 1
        out = torch.empty((n_pts, ch), dtype=torch.float32, device=x.device) if last else None
        where = ctypes.c_void_p()
        L = _lib.load()
        ops = self.ex.ops
        entry, rng = ("ftx_spvcnn_train_fwd", ()) if self.rng is None else ("ftx_spvcnn_train_fwd_rng", self.rng)
        _lib.check(getattr(L, entry)(_ptr(self.layers), _ptr(self.tl), len(self.layers), _ptr(ops), len(ops), _ptr(self.rows), _ptr(self.maps),
                                     len(self.maps), _ptr(self.pvs), len(self.pvs), _ptr(self.routes), _ptr(self.groutes), seg, seg, x.data_ptr(),
                                     _lib.ptr(addend) if seg == 1 else None, _lib.ptr(addend) if seg == 2 else None, self.base,
                                     self.arena.shape[0], _lib.ptr(out), ctypes.byref(where), spf._stream_scratch(), *rng), entry)
        self.forward_done = seg
        if last:
            self.backward_next = seg
            return x, out
        return x, _alias(self.storage, int(where.value) - self.origin, (int(self.rows[level]), ch), x.device)

    def _backward(self, seg, x, grad_out):
        tp = self.ex.tp
        if self.backward_next != seg:
            raise RuntimeError(f"native train: the backward of segment {seg} was asked for when that of segment {self.backward_next} is due: a run gives "
                               "its gradients once, segment by segment from the last (a second backward needs a second forward)")
        sp = tp.seg_params[seg]
        grad_out = _lib.req(grad_out.contiguous(), torch.float32, "native train output gradient", 2)
        flat = torch.empty((sp["total"],), dtype=torch.float32, device=grad_out.device)
        base = flat.data_ptr()
        for f, (idx, off) in sp["fields"].items():
            self.tl[f][idx] = base + off
        where = ctypes.c_void_p()
        L = _lib.load()
        ops = self.ex.ops
        self.backward_next = -1       # whatever happens below, this run is consumed from here
        entry, rng = ("ftx_spvcnn_train_bwd", ()) if self.rng is None else ("ftx_spvcnn_train_bwd_rng", self.rng)
        _lib.check(getattr(L, entry)(_ptr(self.layers), _ptr(self.tl), len(self.layers), _ptr(ops), len(ops), _ptr(self.rows), _ptr(self.maps),
                                     len(self.maps), _ptr(self.pvs), _ptr(self.tpvs), len(self.pvs), _ptr(self.routes), _ptr(self.groutes), seg, seg,
                                     x.data_ptr(), grad_out.data_ptr(), self.base, self.arena.shape[0], ctypes.byref(where), spf._stream_scratch(), *rng),
                   entry)
        self.backward_next = seg - 1
        grads = [g.view(e[3]) if len(e[3]) > 1 else g for g, e in zip(torch.split(flat, sp["sizes"]), sp["entries"])]
        gin = None
        if seg > 0:
            gin = _alias(self.storage, int(where.value) - self.origin, tuple(x.shape), x.device)
        return gin, grads


class _Segment(torch.autograd.Function):
    """One segment of the training program: (run, segment, features, fusion addend or None, *the segment's parameters) -> features."""

    @staticmethod
    def forward(ctx, run, seg, x, addend, *params):
        x, out = run._forward(seg, x, addend)
        ctx.run, ctx.seg, ctx.has_addend = run, seg, addend is not None
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        gin, grads = ctx.run._backward(ctx.seg, x, grad_out)
        return (None, None, gin, gin if ctx.has_addend else None, *grads)
