"""Host side of the native eval-mode executor of the SPVCNN LiDAR branch (include/ftx.h: ftx_spvcnn_eval).

The network is emitted ONCE per model as a static op program over numbered buffers (`emit_program`, a walk over the module tree in the
order of SPVCNN._backbone_steps); per batch the host only fills tables -- the kernel maps and point <-> voxel indices that
SPVCNN._index_steps(ahead=True) built, the row counts, and the route of every convolution from functional._conv_route, which stays the
one routing rule -- and makes one library call per network segment.  All intermediates live in an arena the module owns."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from . import functional as spf
from .models.spvcnn import BatchNorm, Conv3d, operand_mode

_P = "<i8"   # a device pointer in a table
LAYER = np.dtype([("weight", _P), ("bias", _P), ("gamma", _P), ("beta", _P), ("mean", _P), ("var", _P), ("ca", "<i4"), ("co", "<i4"),
                  ("kvol", "<i4"), ("stride", "<i4"), ("transposed", "<i4"), ("bf16", "<i4"), ("eps", "<f4"), ("kind", "<i4")])
OP = np.dtype([("kind", "<i4"), ("segment", "<i4"), ("layer", "<i4"), ("map", "<i4"), ("src", "<i4"), ("src2", "<i4"), ("dst", "<i4"),
               ("relu", "<i4"), ("level", "<i4"), ("channels", "<i4"), ("reserved0", "<i4"), ("reserved1", "<i4")])
MAP = np.dtype([("nbr", _P), ("pos", _P), ("pos_t", _P), ("pair_in", _P), ("pair_out", _P), ("koff", _P), ("n_pairs", "<i8"), ("n_in", "<i8"),
                ("n_out", "<i8"), ("kvol", "<i4"), ("fine_bijective", "<i4")])
PV = np.dtype([("vox_idx", _P), ("vox_counts", _P), ("vox_order", _P), ("vox_seg_off", _P), ("devox_idx", _P), ("devox_weights", _P),
               ("n_vox", "<i8"), ("level", "<i4"), ("reserved", "<i4")])

LAYER_CONV_BN, LAYER_LINEAR_BN = 1, 2
OP_CONV_BN, OP_LINEAR_BN, OP_VOXELIZE, OP_DEVOXELIZE, OP_CONCAT, OP_ADD, OP_ADD_EXT, OP_DROPOUT = 1, 2, 3, 4, 5, 6, 7, 8
ROUTE_ROWS = 4
ROUTES = {spf._EMPTY: 0, spf._DIRECT: 1, spf._OSTAT: 2, spf._PAIRS: 3}
SLOT_INPUT, SLOT_OUTPUT, SLOT_FIRST = 0, 1, 2
SEG_STEM, SEG_ENCODER, SEG_DECODER = 0, 1, 2
POINTS = 5                               # `level` of the point set; voxel level l has stride 2 ** l
STRIDES = (1, 2, 4, 8, 16)
# kernel maps of a batch in table order: the 3^3 map of every level, then the strided 2^3 map between consecutive levels
MAP_KEYS = tuple((3, s, 1) for s in STRIDES) + tuple((2, s, 2) for s in STRIDES[:-1])
PV_STRIDES = (1, 16, 4)                  # where points and voxels exchange features (SPVCNN._index_steps)

_vp = ctypes.c_void_p


def check_record_sizes():
    L = _lib.load()
    assert int(L.ftx_spvcnn_layer_bytes()) == LAYER.itemsize and int(L.ftx_spvcnn_op_bytes()) == OP.itemsize
    assert int(L.ftx_spvcnn_map_bytes()) == MAP.itemsize and int(L.ftx_spvcnn_pv_bytes()) == PV.itemsize


class Unsupported(Exception):
    """The module tree holds something the executor does not run; the caller takes the Python path."""


def _refs(weight, bias, bn):
    """Where a layer's six tensors live: (dict, name) per tensor (None: absent), in the model table's order.  The module's own
    parameter / buffer dicts are kept, not the tensors: `.to()` / `.cuda()` REPLACE a module's buffers, and a table built from a
    tensor object taken earlier would go on reading the old running statistics."""
    pick = lambda r: None if r is None else (r[0]._parameters, r[1])
    return (pick(weight), pick(bias), (bn._parameters, "weight"), (bn._parameters, "bias"), (bn._buffers, "running_mean"), (bn._buffers, "running_var"))


def layer_tensors(layer):
    """(weight, bias, gamma, beta, running_mean, running_var) of a program layer as the modules hold them NOW."""
    return tuple(None if r is None else r[0][r[1]] for r in layer["refs"])


class Program:
    """Static program of one SPVCNN: `ops` (tuples in OP's field order) and `layers` (per layer of the model table its static fields,
    its module and `refs`, where its six tensors live: see layer_tensors)."""

    def __init__(self):
        self.ops, self.layers = [], []
        self.n_slots = SLOT_FIRST
        self.early_channels = self.middle_channels = self.out_channels = 0    # of z0, z1 (what the fusion addends must have) and z3

    def _slot(self):
        self.n_slots += 1
        return self.n_slots - 1

    def _op(self, kind, seg, src, level, channels, layer=-1, map_=-1, src2=-1, relu=0, dst=None, reserved0=0):
        dst = self._slot() if dst is None else dst
        self.ops.append((kind, seg, layer, map_, src, src2, dst, int(relu), level, channels, reserved0, 0))
        return dst

    def dropout(self, seg, slot, level, channels, site, p):
        """OP_DROPOUT in place on `slot` (the training program's alone): site number in `layer`, the float32 bits of p in reserved0."""
        return self._op(OP_DROPOUT, seg, slot, level, channels, layer=site, dst=slot, reserved0=int(np.float32(p).view(np.int32)))

    def conv_bn(self, seg, conv, bn, src, level, residual=-1, relu=True):
        """-> (slot, level) of Conv3d -> BatchNorm (-> + residual) (-> ReLU), as models/spvcnn._conv_bn."""
        if not isinstance(conv, Conv3d) or not isinstance(bn, BatchNorm) or not bn.track_running_stats or not bn.affine:
            raise Unsupported("Conv3d -> BatchNorm with running statistics expected")
        ks, s = conv.kernel_size, conv.stride
        if ks == 1 and s == 1 and not conv.t:
            map_, out_level = -1, level
        elif ks == 3 and s == 1 and not conv.t:
            map_, out_level = MAP_KEYS.index((3, STRIDES[level], 1)), level
        elif ks == 2 and s == 2:
            fine = level - 1 if conv.t else level
            if not 0 <= fine < len(STRIDES) - 1:
                raise Unsupported("strided convolution outside the five levels")
            map_, out_level = MAP_KEYS.index((2, STRIDES[fine], 2)), (fine if conv.t else fine + 1)
        else:
            raise Unsupported(f"Conv3d(kernel_size={ks}, stride={s}, transpose={conv.t})")
        ca, co = conv.in_channels, conv.out_channels
        if ca % 4 or co % 4 or (ks == 1 and max(ca, co) > 512):
            raise Unsupported(f"Conv3d {ca} -> {co}: the kernels take channel counts that are multiples of 4")
        self.layers.append(dict(kind=LAYER_CONV_BN, refs=_refs((conv, "kernel"), None, bn), ca=ca, co=co,
                                kvol=conv.k, stride=s, transposed=int(bool(conv.t)), eps=float(bn.eps), module=conv, bn=bn))
        return self._op(OP_CONV_BN, seg, src, out_level, co, layer=len(self.layers) - 1, map_=map_, src2=residual, relu=relu), out_level

    def linear_bn_relu(self, seg, seq, src, dst=None):
        """nn.Sequential(Linear, BatchNorm, ReLU) on point rows, as models/spvcnn._linear_bn_relu."""
        lin, bn = seq[0], seq[1]
        if not isinstance(lin, torch.nn.Linear) or not isinstance(bn, BatchNorm) or not bn.track_running_stats or not bn.affine:
            raise Unsupported("Linear -> BatchNorm with running statistics expected")
        co, ca = lin.weight.shape
        if ca % 4 or co % 4 or max(ca, co) > 512:
            raise Unsupported(f"Linear {ca} -> {co}: the rows kernel takes multiples of 4 up to 512")
        self.layers.append(dict(kind=LAYER_LINEAR_BN, refs=_refs((lin, "weight"), (lin, "bias") if lin.bias is not None else None, bn), ca=ca, co=co,
                                kvol=0, stride=1, transposed=0, eps=float(bn.eps), module=lin, bn=bn))
        return self._op(OP_LINEAR_BN, seg, src, POINTS, co, layer=len(self.layers) - 1, relu=True, dst=dst)

    def block(self, seg, blk, src, level):
        return self.conv_bn(seg, blk.net[0], blk.net[1], src, level, relu=True)

    def residual(self, seg, blk, src, level):
        if len(blk.downsample) == 0:
            shortcut = src
        else:
            shortcut, _ = self.conv_bn(seg, blk.downsample[0], blk.downsample[1], src, level, relu=False)
        h, lv = self.conv_bn(seg, blk.net[0], blk.net[1], src, level, relu=True)
        return self.conv_bn(seg, blk.net[3], blk.net[4], h, lv, residual=shortcut, relu=True)

    def ops_array(self):
        return np.array(self.ops, dtype=OP)


def emit_program(net, segments=(SEG_STEM, SEG_ENCODER, SEG_DECODER, SEG_DECODER, SEG_DECODER), dropout=False) -> Program:
    """The forward of SPVCNN._backbone_steps from "voxelized" on, op by op in the order that method issues them.  `segments`: the
    segment number of the stem, of the encoder, of the voxelise that feeds the first Dropout (with the middle-fusion add in front of
    it), of the decoder up to the voxelise that feeds the second Dropout, and of the rest.  Dropout is the identity in eval mode, so the
    eval program runs the last three as one; the training program (native_train.py) ends a segment at each, or -- dropout=True, never for
    eval -- holds an OP_DROPOUT (site 0 for y1, site 1 for y3, p of net.dropout) behind each of the two and runs in the same three."""
    P = Program()
    s_stem, s_enc, s_y1, s_dec, s_rest = segments
    cs = net.cs
    pv = {s: i for i, s in enumerate(PV_STRIDES)}
    # ---- stem, z0
    x0, _ = P.conv_bn(s_stem, net.stem[0], net.stem[1], SLOT_INPUT, 0)
    x0, _ = P.conv_bn(s_stem, net.stem[3], net.stem[4], x0, 0)
    z0 = P._op(OP_DEVOXELIZE, s_stem, x0, POINTS, cs[0], map_=pv[1])
    # ---- encoder
    P._op(OP_ADD_EXT, s_enc, z0, POINTS, cs[0], layer=0, dst=z0)
    cur = P._op(OP_VOXELIZE, s_enc, z0, 0, cs[0], map_=pv[1])
    level, skips = 0, [(x0, cs[0])]
    for i, stage in enumerate((net.stage1, net.stage2, net.stage3, net.stage4)):
        cur, level = P.block(s_enc, stage[0], cur, level)
        cur, level = P.residual(s_enc, stage[1], cur, level)
        cur, level = P.residual(s_enc, stage[2], cur, level)
        skips.append((cur, cs[i + 1]))
    x4 = cur
    z1v = P._op(OP_DEVOXELIZE, s_enc, x4, POINTS, cs[4], map_=pv[16])
    t = P.linear_bn_relu(s_enc, net.point_transforms[0], z0)
    z1 = P._op(OP_ADD, s_enc, z1v, POINTS, cs[4], src2=t)
    # ---- decoder
    P._op(OP_ADD_EXT, s_y1, z1, POINTS, cs[4], layer=1, dst=z1)
    cur = P._op(OP_VOXELIZE, s_y1, z1, 4, cs[4], map_=pv[16])
    if dropout:
        P.dropout(s_y1, cur, 4, cs[4], 0, net.dropout.p)

    def up(seg, mod, cur, level, skip, o):
        cur, level = P.block(seg, mod[0], cur, level)
        cur = P._op(OP_CONCAT, seg, cur, level, o + skip[1], src2=skip[0])
        cur, level = P.residual(seg, mod[1][0], cur, level)
        return P.residual(seg, mod[1][1], cur, level)

    cur, level = up(s_dec, net.up1, cur, 4, skips[3], cs[5])
    cur, level = up(s_dec, net.up2, cur, level, skips[2], cs[6])
    z2v = P._op(OP_DEVOXELIZE, s_dec, cur, POINTS, cs[6], map_=pv[4])
    t = P.linear_bn_relu(s_dec, net.point_transforms[1], z1)
    z2 = P._op(OP_ADD, s_dec, z2v, POINTS, cs[6], src2=t)
    cur = P._op(OP_VOXELIZE, s_dec, z2, 2, cs[6], map_=pv[4])
    if dropout:
        P.dropout(s_dec, cur, 2, cs[6], 1, net.dropout.p)
    cur, level = up(s_rest, net.up3, cur, 2, skips[1], cs[7])
    cur, level = up(s_rest, net.up4, cur, level, skips[0], cs[8])
    z3v = P._op(OP_DEVOXELIZE, s_rest, cur, POINTS, cs[8], map_=pv[1])
    t = P.linear_bn_relu(s_rest, net.point_transforms[2], z2)
    P._op(OP_ADD, s_rest, z3v, POINTS, cs[8], src2=t, dst=SLOT_OUTPUT)
    P.early_channels, P.middle_channels, P.out_channels = cs[0], cs[4], cs[8]
    if level != 0 or P.n_slots > 256:
        raise Unsupported("unexpected topology")
    return P


def layer_table(program: Program) -> np.ndarray:
    """The model table of the program's layers at the parameters' present addresses."""
    rec = np.zeros(len(program.layers), dtype=LAYER)
    for r, l in zip(rec, program.layers):
        w, b, g, be, m, v = layer_tensors(l)
        for t in (w, b, g, be, m, v):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                raise Unsupported("parameters must be contiguous float32")
        r["weight"], r["bias"], r["gamma"], r["beta"], r["mean"], r["var"] = (0 if t is None else t.data_ptr() for t in (w, b, g, be, m, v))
        r["ca"], r["co"], r["kvol"], r["stride"], r["transposed"], r["eps"], r["kind"] = l["ca"], l["co"], l["kvol"], l["stride"], l["transposed"], l["eps"], l["kind"]
        r["bf16"] = spf.OPERANDS[operand_mode(l["module"])]     # the record's operand mode: 0 fp32, 1 bf16, 2 split
    return rec


def batch_tables(program: Program, layers: np.ndarray, z, x0):
    """(rows, maps, pvs, routes) of one batch from the structures SPVCNN._index_steps(ahead=True) left on `z` / `x0.cm`."""
    cm = x0.cm
    rows = np.zeros(6, dtype=np.int64)
    for l, s in enumerate(STRIDES):
        rows[l] = cm.coords[s].shape[0]
    rows[POINTS] = z.F.shape[0]
    maps = np.zeros(len(MAP_KEYS), dtype=MAP)
    kms = []
    for r, key in zip(maps, MAP_KEYS):
        km = cm.kernel_maps[key]
        kms.append(km)
        r["nbr"], r["pos"], r["pos_t"], r["pair_in"], r["pair_out"], r["koff"] = (t.data_ptr() for t in (km.nbr, km.pos, km.pos_t, km.pair_in, km.pair_out, km.koff))
        r["n_pairs"], r["n_in"], r["n_out"], r["kvol"], r["fine_bijective"] = km.n_pairs, km.n_in, km.n_out, km.kvol, int(km.fine_bijective)
    pvs = np.zeros(len(PV_STRIDES), dtype=PV)
    af = z.additional_features
    for r, s in zip(pvs, PV_STRIDES):
        seg = af["vox_seg"][s]
        r["vox_idx"], r["vox_counts"] = af["idx_query"][s].data_ptr(), af["counts"][s].data_ptr()
        r["vox_order"], r["vox_seg_off"] = seg.order.data_ptr(), seg.seg_off.data_ptr()
        r["devox_idx"], r["devox_weights"] = z.idx_query[s].data_ptr(), z.weights[s].data_ptr()
        r["n_vox"], r["level"] = seg.m, STRIDES.index(s)
    routes = np.zeros(len(program.ops), dtype=np.int32)
    for i, op in enumerate(program.ops):
        kind, layer, map_, level = op[0], op[2], op[3], op[8]
        if kind == OP_LINEAR_BN or (kind == OP_CONV_BN and map_ < 0):
            routes[i] = ROUTE_ROWS
        elif kind == OP_CONV_BN:
            l = layers[layer]
            routes[i] = ROUTES[spf._conv_route(kms[map_], bool(l["transposed"]), int(l["ca"]), int(l["co"]), int(l["kvol"]), int(rows[level]), int(l["bf16"]))]
    return rows, maps, pvs, routes, kms


def _ptr(a):
    return a.ctypes.data_as(_vp)


def arena_bytes(layers, ops, rows, maps, pvs, routes) -> int:
    """ftx_spvcnn_eval_arena_bytes of the tables (host only); raises with the library's text for tables it refuses."""
    L = _lib.load()
    n = int(L.ftx_spvcnn_eval_arena_bytes(_ptr(layers), len(layers), _ptr(ops), len(ops), _ptr(rows), _ptr(maps), len(maps), _ptr(pvs), len(pvs), _ptr(routes)))
    if n == 0:
        raise RuntimeError("ftx_spvcnn_eval_arena_bytes: " + L.ftx_last_error().decode("utf-8", "replace"))
    return n


class _Host:
    """What both executors keep per module: the program, its op table and the model table (rebuilt when a parameter moved or a layer's
    operand mode -- set_bf16 / set_split -- changed)."""

    def __init__(self, program):
        self.program = program
        self.ops = program.ops_array()
        self.refs = [r for l in program.layers for r in l["refs"] if r is not None]
        self.modules = [l["module"] for l in program.layers]
        self.key = None
        self.layers = None

    def model_table(self):
        key = tuple([d[n].data_ptr() for d, n in self.refs] + [operand_mode(m) for m in self.modules])
        if key != self.key:
            self.layers = layer_table(self.program)
            self.key = key
        return self.layers


class NativeEval(_Host):
    """Per-module state of the executor: the program, the model table and one arena per (device, stream)."""

    def __init__(self, net):
        check_record_sizes()
        super().__init__(emit_program(net))
        self.arenas = {}

    def arena(self, nbytes, device):
        st = _lib.stream()
        k = (device.index, st)
        buf = self.arenas.get(k)
        if buf is None or buf.shape[0] < nbytes:
            # the first batch gets what it needs; a larger one later grows the arena geometrically, so batches of varying size settle
            buf = self.arenas[k] = torch.empty((int(nbytes) if buf is None else int(nbytes * 1.25),), dtype=torch.uint8, device=device)
            buf.record_stream(torch.cuda.current_stream(device))
        return buf

    def begin(self, z, x0):
        """Fill the tables of one batch and size the arena; returns the run whose `segments(first, last, ...)` issues the network."""
        layers = self.model_table()
        rows, maps, pvs, routes, kms = batch_tables(self.program, layers, z, x0)
        need = arena_bytes(layers, self.ops, rows, maps, pvs, routes)
        feats = _lib.req(x0.F.contiguous(), torch.float32, "native eval input features", 2)
        out = torch.empty((int(rows[POINTS]), self.program.out_channels), dtype=torch.float32, device=feats.device)
        return _Run(self, layers, rows, maps, pvs, routes, kms, feats, self.arena(need, feats.device), out)


class _Run:
    def __init__(self, ex, layers, rows, maps, pvs, routes, keep, feats, arena, out):
        self.ex, self.layers, self.rows, self.maps, self.pvs, self.routes = ex, layers, rows, maps, pvs, routes
        self.keep, self.feats, self.arena, self.out = keep, feats, arena, out

    def segments(self, first, last, add_early=None, add_middle=None):
        L = _lib.load()
        prog = self.ex.program
        for t, c in ((add_early, prog.early_channels), (add_middle, prog.middle_channels)):
            if t is not None:
                _lib.req(t, torch.float32, "native eval fusion addend", 2)
                if tuple(t.shape) != (int(self.rows[POINTS]), c):
                    raise ValueError("native eval: the fusion addend does not match the point features")
        ops = self.ex.ops
        _lib.check(L.ftx_spvcnn_eval(_ptr(self.layers), len(self.layers), _ptr(ops), len(ops), _ptr(self.rows), _ptr(self.maps), len(self.maps),
                                     _ptr(self.pvs), len(self.pvs), _ptr(self.routes), self.feats.data_ptr(), int(first), int(last),
                                     _lib.ptr(add_early), _lib.ptr(add_middle), self.arena.data_ptr(), self.arena.shape[0], self.out.data_ptr(),
                                     _lib.stream()), "ftx_spvcnn_eval")
        return self.out
