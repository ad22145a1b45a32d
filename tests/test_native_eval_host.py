"""Host side of the native eval executor (include/ftx.h: ftx_spvcnn_eval): record layouts, the arena size as a pure host function of
the tables, table validation before anything touches a device, and the program emitted from the module tree.  No GPU: every call
here is refused, or answers, before its first launch."""
import ctypes

import numpy as np
import pytest
import torch

from fusiontransformer_amd import native_eval as ne
from fusiontransformer_amd.models.spvcnn import SPVCNN, BatchNorm, Conv3d

FTX_EINVAL, FTX_EWORKSPACE = -1, -3
FAKE = 1 << 20          # a non-null, 256-byte aligned "device address" for tables that are only validated, never launched


@pytest.fixture(scope="module")
def net():
    torch.manual_seed(0)
    return SPVCNN()


@pytest.fixture(scope="module")
def program(net):
    return ne.emit_program(net)


def tables(program, rows=(1000, 600, 300, 120, 40, 1500), subm_pairs_per_row=5, pairs=None):
    """Self-consistent tables of a batch with the given rows per level (+ points); every pointer is FAKE.  Routes as
    functional._conv_route picks them for fp32 layers too wide for the output-stationary kernel: direct for the transposed layers,
    pairs elsewhere, rows for the dense ones."""
    rows = np.array(rows, dtype=np.int64)
    layers = ne.layer_table(program)
    ops = program.ops_array()
    maps = np.zeros(len(ne.MAP_KEYS), dtype=ne.MAP)
    for i, (ks, s, st) in enumerate(ne.MAP_KEYS):
        l = ne.STRIDES.index(s)
        m = maps[i]
        m["kvol"], m["n_in"], m["n_out"] = ks ** 3, rows[l], rows[l] if st == 1 else rows[l + 1]
        m["n_pairs"] = rows[l] * subm_pairs_per_row if st == 1 else rows[l]
        if pairs is not None and st == 1:
            m["n_pairs"] = pairs[l]
        m["fine_bijective"] = int(st == 2)
        for f in ("nbr", "pos", "pos_t", "pair_in", "pair_out", "koff"):
            m[f] = FAKE
    pvs = np.zeros(len(ne.PV_STRIDES), dtype=ne.PV)
    for i, s in enumerate(ne.PV_STRIDES):
        pvs[i]["level"], pvs[i]["n_vox"] = ne.STRIDES.index(s), rows[ne.STRIDES.index(s)]
        for f in ("vox_idx", "vox_counts", "vox_order", "vox_seg_off", "devox_idx", "devox_weights"):
            pvs[i][f] = FAKE
    routes = np.zeros(len(ops), dtype=np.int32)
    for i, op in enumerate(program.ops):
        if op[0] == ne.OP_LINEAR_BN or (op[0] == ne.OP_CONV_BN and op[3] < 0):
            routes[i] = ne.ROUTE_ROWS
        elif op[0] == ne.OP_CONV_BN:
            routes[i] = ne.ROUTES["direct"] if program.layers[op[2]]["transposed"] else ne.ROUTES["pairs"]
    return layers, ops, rows, maps, pvs, routes


def call(ftx_lib, t, arena=FAKE, arena_bytes=None, first=0, last=2):
    layers, ops, rows, maps, pvs, routes = t
    if arena_bytes is None:
        arena_bytes = ne.arena_bytes(*t)
    p = ne._ptr
    rc = ftx_lib.ftx_spvcnn_eval(p(layers), len(layers), p(ops), len(ops), p(rows), p(maps), len(maps), p(pvs), len(pvs), p(routes), FAKE, first, last,
                                 None, None, arena, arena_bytes, FAKE, None)
    return rc, ftx_lib.ftx_last_error().decode()


def size(ftx_lib, t):
    layers, ops, rows, maps, pvs, routes = t
    p = ne._ptr
    return ftx_lib.ftx_spvcnn_eval_arena_bytes(p(layers), len(layers), p(ops), len(ops), p(rows), p(maps), len(maps), p(pvs), len(pvs), p(routes))


def test_record_sizes_match_the_numpy_layouts(ftx_lib):
    assert ftx_lib.ftx_spvcnn_layer_bytes() == ne.LAYER.itemsize == 80
    assert ftx_lib.ftx_spvcnn_op_bytes() == ne.OP.itemsize == 48
    assert ftx_lib.ftx_spvcnn_map_bytes() == ne.MAP.itemsize == 80
    assert ftx_lib.ftx_spvcnn_pv_bytes() == ne.PV.itemsize == 64
    ne.check_record_sizes()


def test_arena_size_is_a_host_function_monotone_and_aligned(ftx_lib, program):
    base_rows = [81237, 43016, 20197, 8102, 2949, 81237]
    base_pairs = [382735, 219664, 126675, 56976, 20329]
    base = ne.arena_bytes(*tables(program, base_rows, pairs=base_pairs))
    assert base % 256 == 0 and base > 4 * 81237 * 128
    assert base == ne.arena_bytes(*tables(program, base_rows, pairs=base_pairs)), "the size depends on the tables alone"
    for i in range(6):
        for step in (1, 63, 5000):
            rows = list(base_rows)
            rows[i] += step
            if i == 0:
                rows[5] = max(rows[5], 1)
            b = ne.arena_bytes(*tables(program, rows, pairs=base_pairs))
            assert b >= base and b % 256 == 0, (i, step, b, base)
    for i in range(5):
        for step in (1, 4097):
            pairs = list(base_pairs)
            pairs[i] += step
            b = ne.arena_bytes(*tables(program, base_rows, pairs=pairs))
            assert b >= base and b % 256 == 0, (i, step, b, base)
    small = ne.arena_bytes(*tables(program, [1, 1, 1, 1, 1, 1], pairs=[1] * 5))
    assert 0 < small < base and small % 256 == 0
    assert ne.arena_bytes(*tables(program, [0] * 6, pairs=[0] * 5)) % 256 == 0      # an empty batch is sized, not refused


def test_tables_are_refused_before_anything_touches_a_device(ftx_lib, program):
    t = tables(program)
    need = ne.arena_bytes(*t)
    rc, msg = call(ftx_lib, t, arena=None)
    assert rc == FTX_EINVAL and "arena" in msg
    rc, msg = call(ftx_lib, t, arena_bytes=need - 1)
    assert rc == FTX_EWORKSPACE and str(need) in msg and str(need - 1) in msg
    rc, msg = call(ftx_lib, t, first=2, last=1)
    assert rc == FTX_EINVAL and "segments" in msg

    # a route the entry point does not take: the direct (scatter) route on a 3x3x3 layer, the output-stationary route on a wide one,
    # a pair-list route on a dense layer, a code that is no route
    conv3 = next(i for i, op in enumerate(program.ops) if op[0] == ne.OP_CONV_BN and op[3] >= 0 and program.layers[op[2]]["kvol"] == 27)
    wide = next(i for i, op in enumerate(program.ops) if op[0] == ne.OP_CONV_BN and op[3] >= 0 and program.layers[op[2]]["co"] == 128)
    dense = next(i for i, op in enumerate(program.ops) if op[0] == ne.OP_LINEAR_BN)
    for op, route, text in ((conv3, ne.ROUTES["direct"], "direct route"), (wide, ne.ROUTES["ostat"], "output-stationary"),
                            (dense, ne.ROUTES["pairs"], "rows route"), (conv3, 9, "route 9"), (conv3, ne.ROUTES["empty"], "empty route")):
        layers, ops, rows, maps, pvs, routes = tables(program)
        routes[op] = route
        bad = (layers, ops, rows, maps, pvs, routes)
        rc, msg = call(ftx_lib, bad, arena_bytes=need)
        assert rc == FTX_EINVAL and text in msg and f"op {op} " in msg, (op, route, rc, msg)
        assert size(ftx_lib, bad) == 0, "the size query refuses the same tables"

    # a channel count that is not a multiple of 4
    layers, ops, rows, maps, pvs, routes = tables(program)
    layers = layers.copy()
    layers[3]["co"] = 30
    rc, msg = call(ftx_lib, (layers, ops, rows, maps, pvs, routes), arena_bytes=need)
    assert rc == FTX_EINVAL and "multiples of 4" in msg and "co=30" in msg
    # a kernel map that does not join the slots it is used on, a slot read before it is written
    layers, ops, rows, maps, pvs, routes = tables(program)
    maps[0]["n_out"] += 1
    rc, msg = call(ftx_lib, (layers, ops, rows, maps, pvs, routes), arena_bytes=need)
    assert rc == FTX_EINVAL and "kernel map 0" in msg
    layers, ops, rows, maps, pvs, routes = tables(program)
    ops = ops.copy()
    ops[1]["src"] = 200
    rc, msg = call(ftx_lib, (layers, ops, rows, maps, pvs, routes), arena_bytes=need)
    assert rc == FTX_EINVAL and "not written before it is read" in msg
    with pytest.raises(RuntimeError, match="not written before"):
        ne.arena_bytes(layers, ops, rows, maps, pvs, routes)


def test_row_kernels_validate_their_arguments(ftx_lib):
    assert ftx_lib.ftx_rows_concat(None, 6, None, 8, 4, None, None) == FTX_EINVAL and b"multiples of 4" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_rows_concat(None, 8, None, 8, 4, None, None) == FTX_EINVAL and b"null" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_rows_concat(None, 8, None, 8, 0, None, None) == 0
    assert ftx_lib.ftx_rows_add(None, None, 3, 10, None, None) == FTX_EINVAL and b"multiple of 4" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_rows_add(None, None, 0, 8, None, None) == 0
    f = ctypes.c_float(1e-5)
    assert ftx_lib.ftx_spconv_reduce_bn_eval(None, None, 4, 30, 27, None, None, None, None, None, f, 1, None, None) == FTX_EINVAL
    assert b"multiple of 4" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_spconv_reduce_bn_eval(None, None, 4, 32, 5, None, None, None, None, None, f, 1, None, None) == FTX_EINVAL
    assert b"kvol must be 8 or 27" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_spconv_reduce_bn_eval(None, None, 4, 32, 27, None, None, None, None, None, f, 1, None, None) == FTX_EINVAL
    assert b"null" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_spconv_reduce_bn_eval(None, None, 0, 32, 8, None, None, None, None, None, f, 1, None, None) == 0


def test_program_references_every_parameter_exactly_once(net, program):
    expected = []
    for m in net.modules():
        if isinstance(m, Conv3d):
            expected.append(m.kernel)
        elif isinstance(m, BatchNorm):
            expected += [m.weight, m.bias, m.running_mean, m.running_var]
    for seq in net.point_transforms:
        expected += [seq[0].weight, seq[0].bias]
    assert len({id(t) for t in expected}) == len(expected)
    got = [t for l in program.layers for t in ne.layer_tensors(l) if t is not None]
    assert sorted(id(t) for t in got) == sorted(id(t) for t in expected)
    # and the model holds nothing the program leaves out, except the BatchNorm step counters
    held = {id(t) for t in list(net.parameters()) + [b for n, b in net.named_buffers() if not n.endswith("num_batches_tracked")]}
    assert held == {id(t) for t in got}
    table = ne.layer_table(program)
    ptrs = [int(r[f]) for r in table for f in ("weight", "bias", "gamma", "beta", "mean", "var") if r[f]]
    assert sorted(ptrs) == sorted(t.data_ptr() for t in expected)
    # the table follows a module whose buffers were replaced (what .to() / .cuda() do), not the tensor objects of emission time
    bn = net.stem[1]
    old = bn.running_mean
    bn.running_mean = old.clone()
    assert int(ne.layer_table(program)[0]["mean"]) == bn.running_mean.data_ptr() != old.data_ptr()
    convs = [l for l in program.layers if l["kind"] == ne.LAYER_CONV_BN]
    assert len(convs) == sum(isinstance(m, Conv3d) for m in net.modules()) and len(program.layers) - len(convs) == 3


def test_program_shape(program):
    ops = program.ops_array()
    assert list(ops["segment"]) == sorted(ops["segment"]) and set(ops["segment"]) == {0, 1, 2}
    ext = ops[ops["kind"] == ne.OP_ADD_EXT]
    assert list(ext["layer"]) == [0, 1] and list(ext["segment"]) == [1, 2], "the fusion addends open the encoder and the decoder"
    assert ops[-1]["dst"] == ne.SLOT_OUTPUT and (ops["dst"] == ne.SLOT_OUTPUT).sum() == 1
    assert (program.early_channels, program.middle_channels, program.out_channels) == (32, 256, 96)


def test_switch_is_off_by_default_and_reaches_every_model(net):
    from fusiontransformer_amd.config import fusion_cfg, lidar_cfg
    from fusiontransformer_amd.models.build import build_model
    assert net.lidar_native_eval is False and net._native is None
    assert not any(getattr(m, "ftx_native_eval", False) for m in net.modules())
    for cfg, path in ((lidar_cfg(), "backbone"), (fusion_cfg("middle"), "lidar_backbone"), (fusion_cfg("early"), "lidar_backbone"),
                      (fusion_cfg("late"), "lidar_backbone.backbone")):
        cfg.MODEL.vit_depth = 1
        cfg.MODEL.late_feat_block_number = 0
        if cfg.MODEL.middle_feat_block_number:
            cfg.MODEL.middle_feat_block_number = 0
        for on in (False, True):
            cfg.MODEL.lidar_native_eval = on
            spv = build_model(cfg)[0]
            for name in path.split("."):
                spv = getattr(spv, name)
            assert spv.lidar_native_eval is on
            assert all(m.ftx_native_eval is on for m in spv.modules() if isinstance(m, Conv3d))
    x = type("X", (), {"F": torch.zeros(4, 4)})()
    net.set_native_eval(True).eval()
    with torch.no_grad():
        assert net._native_executor(x) is None, "CPU tensors take the existing path"
    net.set_native_eval(False).train()
