"""Host side of the native training executor (include/ftx.h: ftx_spvcnn_train_fwd / _bwd): record layouts, the training program and its
backward as emitted from the module tree, the arena size as a pure host function of the tables, table validation before anything
touches a device, and the switch.  No GPU: every call here is refused, or answers, before its first launch."""
import ctypes

import numpy as np
import pytest
import torch

from fusiontransformer_amd import native_eval as ne
from fusiontransformer_amd import native_train as nt
from fusiontransformer_amd.models.spvcnn import SPVCNN, BatchNorm, Conv3d
from tests.test_native_eval_host import FAKE, tables

FTX_EINVAL, FTX_EWORKSPACE = -1, -3


@pytest.fixture(scope="module")
def net():
    torch.manual_seed(0)
    return SPVCNN()


@pytest.fixture(scope="module")
def tp(net):
    return nt.TrainProgram(net)


def train_tables(tp, *args, **kw):
    """tests/test_native_eval_host.tables of the training program plus the data-gradient routes functional._conv_route(grad=True) gives
    on such maps: direct for the strided layers, pairs for the others; none for the first convolution of the stem."""
    layers, ops, rows, maps, pvs, routes = tables(tp.program, *args, **kw)
    groutes = np.full(len(ops), -1, dtype=np.int32)
    for i, op in enumerate(tp.program.ops):
        if op[0] == ne.OP_CONV_BN and op[3] >= 0 and op[4] != ne.SLOT_INPUT:
            l = tp.program.layers[op[2]]
            groutes[i] = ne.ROUTES["direct"] if (l["kvol"] == 8 and not l["transposed"]) else ne.ROUTES["pairs"]
    return layers, ops, rows, maps, pvs, routes, groutes


def size(ftx_lib, t):
    layers, ops, rows, maps, pvs, routes, groutes = t
    p = ne._ptr
    return ftx_lib.ftx_spvcnn_train_arena_bytes(p(layers), len(layers), p(ops), len(ops), p(rows), p(maps), len(maps), p(pvs), len(pvs), p(routes), p(groutes))


def call(ftx_lib, t, direction, arena=FAKE, arena_bytes=None, first=0, last=0, seg_in=FAKE):
    layers, ops, rows, maps, pvs, routes, groutes = t
    if arena_bytes is None:
        arena_bytes = nt.arena_bytes(*t)
    p = ne._ptr
    tl = np.zeros(len(layers), dtype=nt.TRAIN_LAYER)
    for f in nt.GRAD_FIELDS:
        tl[f] = FAKE
    tpvs = np.zeros(len(pvs), dtype=nt.TRAIN_PV)
    where = ctypes.c_void_p()
    if direction == "fwd":
        rc = ftx_lib.ftx_spvcnn_train_fwd(p(layers), p(tl), len(layers), p(ops), len(ops), p(rows), p(maps), len(maps), p(pvs), len(pvs), p(routes), p(groutes),
                                          first, last, seg_in, None, None, arena, arena_bytes, FAKE, ctypes.byref(where), None)
    else:
        rc = ftx_lib.ftx_spvcnn_train_bwd(p(layers), p(tl), len(layers), p(ops), len(ops), p(rows), p(maps), len(maps), p(pvs), p(tpvs), len(pvs), p(routes),
                                          p(groutes), first, last, seg_in, FAKE, arena, arena_bytes, ctypes.byref(where), None)
    return rc, ftx_lib.ftx_last_error().decode()


def test_record_sizes_match_the_numpy_layouts(ftx_lib):
    assert ftx_lib.ftx_spvcnn_train_layer_bytes() == nt.TRAIN_LAYER.itemsize == 40
    assert ftx_lib.ftx_spvcnn_train_pv_bytes() == nt.TRAIN_PV.itemsize == 16
    # the eval executor's records keep their sizes
    assert (ftx_lib.ftx_spvcnn_layer_bytes(), ftx_lib.ftx_spvcnn_op_bytes(), ftx_lib.ftx_spvcnn_map_bytes(), ftx_lib.ftx_spvcnn_pv_bytes()) == (80, 48, 80, 64)
    nt.check_record_sizes()


def test_training_program_is_the_eval_program_cut_into_five_segments(net, tp):
    ev = ne.emit_program(net)
    drop_seg = lambda ops: [op[:1] + op[2:] for op in ops]
    assert drop_seg(tp.program.ops) == drop_seg(ev.ops), "same walk, same ops, same slots"
    assert set(ev.ops_array()["segment"]) == {0, 1, 2}, "the eval program keeps its three segments"
    ops = tp.program.ops_array()
    assert list(ops["segment"]) == sorted(ops["segment"]) and set(ops["segment"]) == {0, 1, 2, 3, 4} and tp.n_segments == 5
    # a segment ends at the voxelise that feeds each Dropout; the middle-fusion addend opens the first of them
    for seg in (2, 3):
        assert ops[ops["segment"] == seg][-1]["kind"] == ne.OP_VOXELIZE
    assert [(o["kind"], o["layer"]) for o in ops[ops["segment"] == 2]] == [(ne.OP_ADD_EXT, 1), (ne.OP_VOXELIZE, -1)]
    ext = ops[ops["kind"] == ne.OP_ADD_EXT]
    assert list(ext["layer"]) == [0, 1] and list(ext["segment"]) == [1, 2]
    assert tp.out_slot[-1] == ne.SLOT_OUTPUT and tp.in_slot[0] == ne.SLOT_INPUT and tp.in_slot[1:] == tp.out_slot[:-1]
    # the slot a Dropout rewrites (or replaces) is read by the segment behind it only
    for seg in (3, 4):
        s = tp.in_slot[seg]
        readers = {op[1] for op in tp.program.ops if s in (op[4], op[5])}
        assert readers == {seg}


def test_backward_is_the_forward_reversed_with_at_most_two_contributions(net, tp):
    n = len(tp.program.ops)
    assert tp.backward == list(range(n))[::-1]
    assert max(len(v) for v in tp.contributions.values()) == 2
    assert all(1 <= len(v) <= 2 for v in tp.contributions.values())
    # every slot but the input features and the output receives a gradient; the first convolution of the stem sends none
    written = {op[6] for op in tp.program.ops}
    assert set(tp.contributions) == written - {ne.SLOT_OUTPUT}
    assert ne.SLOT_INPUT not in tp.contributions and tp.program.ops[0][4] == ne.SLOT_INPUT
    # the operands of an ADD take the gradient of the sum as it is: they have no other reader
    for op in tp.program.ops:
        if op[0] == ne.OP_ADD:
            assert len(tp.contributions[op[4]]) == 1 and len(tp.contributions[op[5]]) == 1
    # no buffer the backward reads has a later writer (ADD_EXT works in place BEFORE the first op that saves its slot)
    for i, op in enumerate(tp.program.ops):
        for s in nt.saved_slots(op):
            assert not [w for w, o in enumerate(tp.program.ops) if o[6] == s and w > i], (i, s)
    assert ne.SLOT_INPUT in tp.saved and len(tp.saved) > 60


def test_three_contributions_are_refused(net):
    tp = nt.TrainProgram(net)
    ops = list(tp.program.ops)
    # a third reader of the stem output (devoxelise + skip are its two)
    x0_slot = ops[1][6]
    extra = (ne.OP_DEVOXELIZE, 4, -1, 0, x0_slot, -1, 250, 0, ne.POINTS, 32, 0, 0)
    orig = ne.emit_program

    def emit(net_, segments=None):
        P = orig(net_, segments=segments)
        P.ops.insert(len(P.ops) - 1, extra)
        return P
    ne.emit_program = emit
    try:
        with pytest.raises(ne.Unsupported, match="3 gradient contributions"):
            nt.TrainProgram(net)
    finally:
        ne.emit_program = orig


def test_gradient_table_holds_every_parameter_exactly_once(net, tp):
    got = tp.parameters()
    assert len({id(t) for t in got}) == len(got)
    assert {id(t) for t in got} == {id(p) for p in net.parameters()}
    fields = {}
    for li, field, ref in tp.grad_table:
        fields.setdefault(li, []).append(field)
    for li, l in enumerate(tp.program.layers):
        assert fields[li] == [f for f, r in zip(nt.GRAD_FIELDS, l["refs"][:4]) if r is not None]
    # per segment: every parameter of the segment's layers, contiguous places in one flat buffer
    seen = []
    for s, sp in enumerate(tp.seg_params):
        off = 0
        for li, field, ref, shape, o, n in sp["entries"]:
            assert o == off and n == int(np.prod(shape)) and o % 4 == 0
            off += n
            seen.append(id(ref[0][ref[1]]))
        assert off == sp["total"]
    assert sorted(seen) == sorted(id(p) for p in net.parameters())
    assert sum(len(b) for b in tp.seg_bns) == sum(isinstance(m, BatchNorm) for m in net.modules())
    assert sum(isinstance(m, Conv3d) for m in net.modules()) + 3 == len(tp.program.layers)


def test_arena_size_is_a_host_function_monotone_and_aligned(ftx_lib, tp):
    base_rows = [81237, 43016, 20197, 8102, 2949, 81237]
    base_pairs = [382735, 219664, 126675, 56976, 20329]
    base = nt.arena_bytes(*train_tables(tp, base_rows, pairs=base_pairs))
    assert base % 256 == 0 and base == size(ftx_lib, train_tables(tp, base_rows, pairs=base_pairs)), "the size depends on the tables alone"
    assert base > 3 * 4 * 81237 * 32 * 10, "at least input, output and convolution output of the ten finest layers"
    for i in range(6):
        for step in (1, 47, 63, 255, 5000):
            rows = list(base_rows)
            rows[i] += step
            b = nt.arena_bytes(*train_tables(tp, rows, pairs=base_pairs))
            assert b >= base and b % 256 == 0, (i, step, b, base)
    for i in range(5):
        for step in (1, 255, 257, 4097, 100000):
            pairs = list(base_pairs)
            pairs[i] += step
            b = nt.arena_bytes(*train_tables(tp, base_rows, pairs=pairs))
            assert b >= base and b % 256 == 0, (i, step, b, base)
    small = nt.arena_bytes(*train_tables(tp, [1, 1, 1, 1, 1, 1], pairs=[1] * 5))
    assert 0 < small < base and small % 256 == 0
    with pytest.raises(nt.Refused, match="at least one row"):       # the training BatchNorm of a level without rows has no statistics
        nt.arena_bytes(*train_tables(tp, [5, 4, 3, 2, 0, 9], pairs=[5, 4, 3, 2, 0]))


def test_tables_are_refused_before_anything_touches_a_device(ftx_lib, tp):
    t = train_tables(tp)
    need = nt.arena_bytes(*t)
    for direction in ("fwd", "bwd"):
        rc, msg = call(ftx_lib, t, direction, arena=None)
        assert rc == FTX_EINVAL and "arena" in msg
        rc, msg = call(ftx_lib, t, direction, arena_bytes=need - 1)
        assert rc == FTX_EWORKSPACE and str(need) in msg and str(need - 1) in msg
        rc, msg = call(ftx_lib, t, direction, first=2, last=1)
        assert rc == FTX_EINVAL and "segments" in msg
        rc, msg = call(ftx_lib, t, direction, first=5, last=5)
        assert rc == FTX_EINVAL and "segments" in msg
        rc, msg = call(ftx_lib, t, direction, seg_in=None)
        assert rc == FTX_EINVAL and "null input" in msg
        # z1 is read by two segments: the segment it opens must be given the buffer itself, not a replacement
        rc, msg = call(ftx_lib, t, direction, first=2, last=2, seg_in=FAKE + 256)
        assert rc == FTX_EINVAL and "also read by another segment" in msg

    program = tp.program
    conv3 = next(i for i, op in enumerate(program.ops) if op[0] == ne.OP_CONV_BN and op[3] >= 0 and program.layers[op[2]]["kvol"] == 27 and op[4] != 0)
    wide = next(i for i, op in enumerate(program.ops) if op[0] == ne.OP_CONV_BN and op[3] >= 0 and program.layers[op[2]]["co"] == 128)
    dense = next(i for i, op in enumerate(program.ops) if op[0] == ne.OP_LINEAR_BN)
    down = next(i for i, op in enumerate(program.ops) if op[0] == ne.OP_CONV_BN and program.layers[op[2]]["kvol"] == 8 and not program.layers[op[2]]["transposed"])
    # a forward route the op cannot take
    for op, route, text in ((conv3, ne.ROUTES["direct"], "direct route"), (wide, ne.ROUTES["ostat"], "output-stationary"),
                            (dense, ne.ROUTES["pairs"], "rows route"), (conv3, 9, "route 9"), (conv3, ne.ROUTES["empty"], "empty route")):
        bad = train_tables(tp)
        bad[5][op] = route
        for direction in ("fwd", "bwd"):
            rc, msg = call(ftx_lib, bad, direction, arena_bytes=need)
            assert rc == FTX_EINVAL and text in msg and f"op {op} " in msg, (op, route, rc, msg)
        assert size(ftx_lib, bad) == 0, "the size query refuses the same tables"
    # a data-gradient route the op cannot take
    for op, route, text in ((conv3, ne.ROUTES["direct"], "direct gradient route"), (conv3, ne.ROUTES["empty"], "empty gradient route"),
                            (down, ne.ROUTES["ostat"], "gradient route 2"), (conv3, -1, "gradient route -1")):
        bad = train_tables(tp)
        bad[6][op] = route
        rc, msg = call(ftx_lib, bad, "bwd", arena_bytes=need, first=4, last=4)
        assert rc == FTX_EINVAL and text in msg and f"op {op} " in msg, (op, route, rc, msg)
        assert size(ftx_lib, bad) == 0
    # a missing kernel map, a map that does not join its slots, a missing point-voxel index
    layers, ops, rows, maps, pvs, routes, groutes = train_tables(tp)
    rc, msg = call(ftx_lib, (layers, ops, rows, maps[:5], pvs, routes, groutes), "fwd", arena_bytes=need)
    assert rc == FTX_EINVAL and "kernel map 5 missing" in msg
    maps[0]["n_out"] += 1
    rc, msg = call(ftx_lib, (layers, ops, rows, maps, pvs, routes, groutes), "fwd", arena_bytes=need)
    assert rc == FTX_EINVAL and "kernel map 0" in msg
    layers, ops, rows, maps, pvs, routes, groutes = train_tables(tp)
    rc, msg = call(ftx_lib, (layers, ops, rows, maps, pvs[:1], routes, groutes), "bwd", arena_bytes=need)
    assert rc == FTX_EINVAL and "point-voxel index" in msg
    pvs[1]["vox_idx"] = 0
    rc, msg = call(ftx_lib, (layers, ops, rows, maps, pvs, routes, groutes), "fwd", arena_bytes=need)
    assert rc == FTX_EINVAL and "null voxel index" in msg
    # a slot with three readers that need a gradient
    layers, ops, rows, maps, pvs, routes, groutes = train_tables(tp)
    ops = ops.copy()
    d = int(np.flatnonzero(ops["kind"] == ne.OP_DEVOXELIZE)[-1])
    ops[d]["src"] = ops[d - 1]["src2"]          # the last block's input (convolution + shortcut read it) in place of its output
    rc, msg = call(ftx_lib, (layers, ops, rows, maps, pvs, routes, groutes), "fwd", arena_bytes=need)
    assert rc == FTX_EINVAL and "more than two gradient contributions" in msg, msg
    layers, ops, rows, maps, pvs, routes, groutes = train_tables(tp)
    with pytest.raises(nt.Refused, match="not written before"):
        ops = ops.copy()
        ops[1]["src"] = 200
        nt.arena_bytes(layers, ops, rows, maps, pvs, routes, groutes)


def test_rows_split_validates_its_arguments(ftx_lib):
    assert ftx_lib.ftx_rows_split(None, 4, 6, 8, None, None, None) == FTX_EINVAL and b"multiples of 4" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_rows_split(None, -1, 8, 8, None, None, None) == FTX_EINVAL and b"n < 0" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_rows_split(None, 4, 8, 8, None, None, None) == FTX_EINVAL and b"null" in ftx_lib.ftx_last_error()
    assert ftx_lib.ftx_rows_split(None, 0, 8, 8, None, None, None) == 0
    assert ftx_lib.ftx_rows_split(FAKE, 4, 8, 8, FAKE + 4, FAKE, None) == FTX_EINVAL and b"16-byte aligned" in ftx_lib.ftx_last_error()


def test_a_layer_that_writes_the_output_slot_is_refused(ftx_lib, tp):
    """The backward of a layer reads the layer's result; the backward is not given the output buffer."""
    layers, ops, rows, maps, pvs, routes, groutes = train_tables(tp)
    ops = ops.copy()
    lin = int(np.flatnonzero(ops["kind"] == ne.OP_LINEAR_BN)[-1])
    assert ops[-1]["kind"] == ne.OP_ADD and ops[-1]["src2"] == ops[lin]["dst"]
    ops[lin]["dst"] = ne.SLOT_OUTPUT
    assert size(ftx_lib, (layers, ops, rows, maps, pvs, routes, groutes)) == 0
    assert "may not write the output slot" in ftx_lib.ftx_last_error().decode()


def test_switch_is_off_by_default_and_reaches_every_model(net):
    from fusiontransformer_amd.config import fusion_cfg, lidar_cfg
    from fusiontransformer_amd.models.build import build_model
    assert net.lidar_native_train is False and net._native_tr is None
    for cfg, path in ((lidar_cfg(), "backbone"), (fusion_cfg("middle"), "lidar_backbone"), (fusion_cfg("early"), "lidar_backbone"),
                      (fusion_cfg("late"), "lidar_backbone.backbone")):
        cfg.MODEL.vit_depth = 1
        cfg.MODEL.late_feat_block_number = 0
        if cfg.MODEL.middle_feat_block_number:
            cfg.MODEL.middle_feat_block_number = 0
        for on in (False, True):
            cfg.MODEL.lidar_native_train = on
            spv = build_model(cfg)[0]
            for name in path.split("."):
                spv = getattr(spv, name)
            assert spv.lidar_native_train is on
            assert spv.lidar_native_eval is False and spv.lidar_native_index is False and spv.lidar_bf16 is False, "independent switches"
    x = type("X", (), {"F": torch.zeros(4, 4)})()
    net.set_native_train(True).train()
    assert net._native_trainer(x) is None, "CPU tensors take the existing path"
    assert net._native_tr is None, "nothing is built for a forward the executor does not run"
    net.set_native_eval(True).set_native_index(True).set_bf16(True)
    assert net.lidar_native_train is True
    net.set_native_eval(False).set_native_index(False).set_bf16(False).set_native_train(False)
    assert net.lidar_native_train is False and net._native_tr is None


def test_step_counter_names_exactly_the_counters_a_training_forward_bumps():
    """models/spvcnn.step_counter is the one rule every site that bumps num_batches_tracked asks (BatchNorm.fused, _conv_bn, this
    executor's _Run._forward, the image branch's stems): the module's own counter in training mode with running statistics, None in eval
    mode, without running statistics, and once _fusion_common.bump_batchnorm_counters counts for the module."""
    from fusiontransformer_amd.models._fusion_common import bump_batchnorm_counters
    from fusiontransformer_amd.models.image_models_billinear import Net2DBillinear
    from fusiontransformer_amd.models.spvcnn import step_counter
    torch.manual_seed(0)
    lidar = SPVCNN(cr=0.25)
    image = Net2DBillinear(num_classes=4, dual_head=False, backbone_2d_kwargs=dict(vit_depth=2, middle_feat_block_number=0, late_feat_block_number=1))
    for model, n_bns in ((lidar, 52), (image, 3)):      # 2 stem + 23 encoder + 24 decoder + 3 point transforms; sample_down + two taps
        bns = [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]
        assert len(bns) == n_bns
        model.train()
        assert all(step_counter(m) is m.num_batches_tracked for m in bns)
        model.eval()
        assert all(step_counter(m) is None for m in bns)
        model.train()
        bns[1].eval()      # a module frozen on its own keeps its counter
        assert [step_counter(m) is None for m in bns] == [i == 1 for i in range(n_bns)]
        before = [int(m.num_batches_tracked) for m in bns]
        bump_batchnorm_counters(model)      # counts once for every training module and marks them all
        assert [int(m.num_batches_tracked) - b for m, b in zip(bns, before)] == [i != 1 for i in range(n_bns)]
        bns[1].train()
        assert all(step_counter(m) is None for m in bns), "the model's one launch counts for them from here on"
        model.eval()
        assert all(step_counter(m) is None for m in bns)
    for bn in (BatchNorm(8, track_running_stats=False), torch.nn.BatchNorm2d(8, track_running_stats=False)):
        bn.train()
        assert bn.num_batches_tracked is None and step_counter(bn) is None
    bn = BatchNorm(8).train()
    assert step_counter(bn) is bn.num_batches_tracked
