"""Host side of the library's Dropout (include/ftx.h: ftx_dropout, FTX_SPVCNN_OP_DROPOUT, ftx_spvcnn_train_fwd_rng / _bwd_rng): the numpy
restatement of the random stream (tests/dropout_ref.py) against Random123's published Philox4x32-10 vectors, the threshold and the
scale, its keep rate, the training program with the op, and the checker's conditions on it.  No GPU: every library call here is
refused, or answers, before its first launch."""
import ctypes

import numpy as np
import pytest
import torch

from fusiontransformer_amd import native_eval as ne
from fusiontransformer_amd import native_train as nt
from fusiontransformer_amd.models.spvcnn import SPVCNN
from tests import dropout_ref as R
from tests import test_native_eval_host as eh
from tests import test_native_train_host as th

FTX_EINVAL = -1
FAKE = eh.FAKE
TRAIN = "ftx_spvcnn_train: "
P03 = int(np.float32(0.3).view(np.int32))


# ---------------------------------------------------------------- the restatement
KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter,key,out", KNOWN, ids=["zeros", "ones", "pi"])
def test_restatement_reproduces_the_published_philox_vectors(counter, key, out):
    assert tuple(int(w) for w in R.philox4x32_10(counter, key)) == out


def test_counter_layout_of_an_element():
    """Element g of draw (seed, call): block g >> 2 in the low counter words, the call in the high ones, the seed as the key, word g & 3."""
    seed, call, elem0 = (0x299f31d0 << 32) | 0xa4093822, (0x03707344 << 32) | 0x13198a2e, ((0x05a308d3 << 32) | 0x243f6a88) << 2      # q has 62 bits
    block = [int(w) for w in R.philox4x32_10((0x243f6a88, 0x05a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))]
    assert [int(u) for u in R.uniform_words(4, seed, call, elem0)] == block
    assert [int(u) for u in R.uniform_words(3, seed, call, elem0 + 1)] == block[1:]
    # q crosses 2^32 inside a call, and the logical index wraps at 2^64
    u = R.uniform_words(8, 5, 9, (1 << 34) - 4)
    assert [int(w) for w in u[:4]] == [int(w) for w in R.philox4x32_10((0xffffffff, 0, 9, 0), (5, 0))]
    assert [int(w) for w in u[4:]] == [int(w) for w in R.philox4x32_10((0, 1, 9, 0), (5, 0))]
    assert [int(w) for w in R.uniform_words(8, 5, 9, (1 << 64) - 4)[4:]] == [int(w) for w in R.philox4x32_10((0, 0, 9, 0), (5, 0))]


def test_threshold_and_scale():
    assert R.threshold(0.3) == 1288490188 and R.threshold(0.0) == 0 and R.threshold(0.5) == 1 << 31
    assert R.scale(0.3) == np.float32(1 / 0.7) and R.scale(0.3).dtype == np.float32 and R.scale(0.0) == np.float32(1.0)
    assert R.threshold(np.float32(0.3)) == 1288490240 and R.scale(np.float32(0.3)) == np.float32(1 / 0.7), "as the entries see p = 0.3"
    assert R.threshold(np.float32(0.999999)) < 1 << 32
    assert R.keep_mask(4096, 0.0, 3, 4).all()
    x = np.array([1.5, -0.0, np.inf, np.nan, 1e-40], dtype=np.float32)
    assert R.dropout(x, 0.0, 1, 2).tobytes() == x.tobytes(), "p = 0 returns x bit for bit"


@pytest.mark.parametrize("seed,call", [(0, 0), (1234, 7), ((1 << 63) + 5, 3)])
def test_keep_rate_of_the_restatement(seed, call):
    """2^20 Bernoulli(0.7) draws: sigma = sqrt(0.21 / 2^20) = 4.5e-4, and 2.5e-3 is more than five of them."""
    rate = float(R.keep_mask(1 << 20, 0.3, seed, call).mean())
    print("keep rate (seed %d, call %d): %.5f" % (seed, call, rate))
    assert abs(rate - 0.7) <= 2.5e-3, rate


# ---------------------------------------------------------------- the entries' argument checks
def test_dropout_entries_refuse_bad_arguments_before_a_launch(ftx_lib):
    err = lambda: ftx_lib.ftx_last_error().decode()
    for p in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        assert ftx_lib.ftx_dropout(FAKE, 8, p, 0, 0, 0, FAKE, None) == FTX_EINVAL and "outside [0, 1)" in err(), p
        assert ftx_lib.ftx_dropout_mask(8, p, 0, 0, 0, FAKE, None) == FTX_EINVAL and "outside [0, 1)" in err(), p
    assert ftx_lib.ftx_dropout(FAKE, -1, 0.3, 0, 0, 0, FAKE, None) == FTX_EINVAL and "n < 0" in err()
    assert ftx_lib.ftx_dropout_mask(-1, 0.3, 0, 0, 0, FAKE, None) == FTX_EINVAL and "n < 0" in err()
    assert ftx_lib.ftx_dropout(None, 8, 0.3, 0, 0, 0, FAKE, None) == FTX_EINVAL and "null" in err()
    assert ftx_lib.ftx_dropout(FAKE, 8, 0.3, 0, 0, 0, None, None) == FTX_EINVAL and "null" in err()
    assert ftx_lib.ftx_dropout_mask(8, 0.3, 0, 0, 0, None, None) == FTX_EINVAL and "null" in err()
    assert ftx_lib.ftx_dropout(FAKE + 2, 8, 0.3, 0, 0, 0, FAKE + 256, None) == FTX_EINVAL and "4-byte aligned" in err()
    for y in (FAKE + 4, FAKE - 4, FAKE + 28, FAKE - 28):      # any overlap but y == x
        assert ftx_lib.ftx_dropout(FAKE, 8, 0.3, 0, 0, 0, y, None) == FTX_EINVAL and "overlap" in err(), y
    assert ftx_lib.ftx_dropout(None, 0, 0.3, 0, 0, 0, None, None) == 0 and ftx_lib.ftx_dropout_mask(0, 0.3, 0, 0, 0, None, None) == 0
    assert ftx_lib.ftx_dropout_sweep_elements() == 2048 * 256 * 4


def test_wrappers_refuse_bad_arguments():
    from fusiontransformer_amd import functional as spf
    x = torch.zeros(8)
    with pytest.raises(ValueError, match="CUDA"):
        spf.dropout(x, 0.3, 0, 0)
    with pytest.raises(ValueError, match="CUDA"):
        spf.dropout_mask((8,), 0.3, 0, 0, device="cpu")
    for bad in (dict(p=1.0), dict(p=-0.5), dict(p=float("nan")), dict(p=0.99999999), dict(seed=-1), dict(seed=1 << 64), dict(call=1.5), dict(elem0=-1)):
        kw = dict(p=0.3, seed=0, call=0, elem0=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            spf.dropout(x, **kw)
        with pytest.raises(ValueError):
            spf.dropout_mask((8,), **kw)


# ---------------------------------------------------------------- program and checker
@pytest.fixture(scope="module")
def net():
    torch.manual_seed(0)
    return SPVCNN()


@pytest.fixture(scope="module")
def tps(net):
    return nt.TrainProgram(net), nt.TrainProgram(net, native_dropout=True)


def sites(ops):
    return [int(i) for i in np.flatnonzero(ops["kind"] == ne.OP_DROPOUT)]


def test_program_with_the_switch_on_has_three_segments_and_two_dropout_ops(net, tps):
    five, three = tps
    ops5, ops3 = five.program.ops_array(), three.program.ops_array()
    assert three.n_segments == 3 and sorted(set(ops3["segment"])) == [0, 1, 2] and list(ops3["segment"]) == sorted(ops3["segment"])
    d = sites(ops3)
    assert len(d) == 2 and len(ops3) == len(ops5) + 2 and not sites(ops5)
    without = np.delete(ops3, d)
    for f in ops5.dtype.names:
        if f != "segment":
            assert (without[f] == ops5[f]).all(), f
    assert (without["segment"] == np.minimum(ops5["segment"], 2)).all(), "the eval program's segments"
    assert (without["segment"] == ne.emit_program(net).ops_array()["segment"]).all()
    for site, i in enumerate(d):
        o, vox = ops3[i], ops3[i - 1]
        assert vox["kind"] == ne.OP_VOXELIZE and o["src"] == o["dst"] == vox["dst"] and o["level"] == vox["level"] and o["channels"] == vox["channels"]
        assert o["layer"] == site and o["reserved0"] == P03 and o["segment"] == 2 and o["map"] == -1 and o["src2"] == -1
    assert [(int(ops3[i]["level"]), int(ops3[i]["channels"])) for i in d] == [(4, net.cs[4]), (2, net.cs[6])], "y1 and y3"
    # the five-segment program ends a segment where the three-segment one has the op
    assert [int(ops5[i - s - 1]["segment"]) for s, i in enumerate(d)] == [2, 3] and [int(ops5[i - s]["segment"]) for s, i in enumerate(d)] == [3, 4]
    assert set(id(p) for p in three.parameters()) == set(id(p) for p in net.parameters())
    assert not sites(ne.emit_program(net).ops_array()), "emit_program never emits a Dropout for eval"


def test_program_is_accepted_and_needs_no_more_arena(ftx_lib, tps):
    five, three = tps
    for kw in (dict(), dict(rows=[81237, 43016, 20197, 8102, 2949, 81237], pairs=[382735, 219664, 126675, 56976, 20329]), dict(rows=[1] * 6, pairs=[1] * 5)):
        a5, a3 = th.size(ftx_lib, th.train_tables(five, **kw)), th.size(ftx_lib, th.train_tables(three, **kw))
        assert a3 > 0 and a3 % 256 == 0 and a3 <= a5, (kw, a3, a5, ftx_lib.ftx_last_error())
        assert a3 == a5, "the op adds no region"


def rng_call(ftx_lib, t, direction, arena=FAKE, first=0, last=0):
    layers, ops, rows, maps, pvs, routes, groutes = t
    p = ne._ptr
    tl = np.zeros(len(layers), dtype=nt.TRAIN_LAYER)
    for f in nt.GRAD_FIELDS:
        tl[f] = FAKE
    tpvs = np.zeros(len(pvs), dtype=nt.TRAIN_PV)
    where = ctypes.c_void_p()
    if direction == "fwd":
        rc = ftx_lib.ftx_spvcnn_train_fwd_rng(p(layers), p(tl), len(layers), p(ops), len(ops), p(rows), p(maps), len(maps), p(pvs), len(pvs), p(routes),
                                              p(groutes), first, last, FAKE, None, None, arena, 1 << 40, FAKE, ctypes.byref(where), None, 7, 8)
    else:
        rc = ftx_lib.ftx_spvcnn_train_bwd_rng(p(layers), p(tl), len(layers), p(ops), len(ops), p(rows), p(maps), len(maps), p(pvs), p(tpvs), len(pvs),
                                              p(routes), p(groutes), first, last, FAKE, FAKE, arena, 1 << 40, ctypes.byref(where), None, 7, 8)
    return rc, ftx_lib.ftx_last_error().decode()


def mutated(three, mutate):
    t = list(th.train_tables(three))
    t[1] = t[1].copy()
    mutate(t[1])
    return tuple(t)


def refused_everywhere(ftx_lib, t, text):
    assert th.size(ftx_lib, t) == 0 and ftx_lib.ftx_last_error().decode() == text, ftx_lib.ftx_last_error()
    for direction in ("fwd", "bwd"):
        assert rng_call(ftx_lib, t, direction, arena=None) == (FTX_EINVAL, text)
        assert th.call(ftx_lib, t, direction, arena=None, arena_bytes=1 << 40) == (FTX_EINVAL, text)


def test_checker_conditions_on_the_op(ftx_lib, tps):
    five, three = tps
    ops = three.program.ops_array()
    d0, d1 = sites(ops)
    t = th.train_tables(three)
    for direction in ("fwd", "bwd"):      # accepted: the _rng entries go on to ask for the arena
        rc, msg = rng_call(ftx_lib, t, direction, arena=None)
        assert rc == FTX_EINVAL and "the arena must be a 256-byte aligned device buffer" in msg, msg

    def not_in_place(o):
        o[d0]["dst"] = 200
    refused_everywhere(ftx_lib, mutated(three, not_in_place), TRAIN + "op %d (dropout): Dropout works in place on an arena slot (layer = its site number >= 0)" % d0)

    def negative_site(o):
        o[d1]["layer"] = -1
    refused_everywhere(ftx_lib, mutated(three, negative_site), TRAIN + "op %d (dropout): Dropout works in place on an arena slot (layer = its site number >= 0)" % d1)

    def on_the_input(o):
        o[d0]["src"] = o[d0]["dst"] = ne.SLOT_INPUT
        o[d0]["level"], o[d0]["channels"] = 0, 4
    t_in = mutated(three, on_the_input)
    assert th.size(ftx_lib, t_in) == 0 and "Dropout works in place on an arena slot" in ftx_lib.ftx_last_error().decode()

    def already_read(o):      # on z1, which the voxelise in front of it has read
        z1 = o[d0 - 1]["src"]
        o[d0]["src"] = o[d0]["dst"] = z1
        o[d0]["level"], o[d0]["channels"] = ne.POINTS, o[d0 - 1]["channels"]
    slot = int(ops[d0 - 1]["src"])
    refused_everywhere(ftx_lib, mutated(three, already_read),
                       TRAIN + "op %d (dropout): slot %d is read before the Dropout reaches it, and the backward would read it after" % (d0, slot))

    for p, shown in ((1.0, "1"), (-0.25, "-0.25"), (float("nan"), None), (2.0, "2")):
        def out_of_range(o, p=p):
            o[d1]["reserved0"] = int(np.float32(p).view(np.int32))
        t_p = mutated(three, out_of_range)
        assert th.size(ftx_lib, t_p) == 0
        msg = ftx_lib.ftx_last_error().decode()
        assert msg.startswith(TRAIN + "op %d (dropout): p = " % d1) and msg.endswith("outside [0, 1)") and (shown is None or "p = %s " % shown in msg), msg
        assert rng_call(ftx_lib, t_p, "fwd", arena=None) == (FTX_EINVAL, msg)

    def p_zero(o):
        o[d0]["reserved0"] = 0
    assert th.size(ftx_lib, mutated(three, p_zero)) == th.size(ftx_lib, t)

    # kind 9 is as unknown as before
    def kind_nine(o):
        o[d0]["kind"] = 9
    refused_everywhere(ftx_lib, mutated(three, kind_nine), TRAIN + "op %d: unknown kind 9" % d0)


def test_a_slot_whose_gradient_is_another_buffers_is_refused(ftx_lib, tps):
    """The backward scales the slot's gradient buffer in place: not the caller's grad_out (a segment's result), not a sum's buffer."""
    five, three = tps
    ops = three.program.ops_array()
    d0 = sites(ops)[0]

    def ends_its_segment(o):       # everything behind the first Dropout moves to a fourth segment
        o["segment"][d0 + 1:] = 3
    t = mutated(three, ends_its_segment)
    assert th.size(ftx_lib, t) == 0
    assert ftx_lib.ftx_last_error().decode() == TRAIN + "op %d (dropout): slot %d is an operand of an add or the result of its segment: its gradient is another buffer's" % (
        d0, int(ops[d0]["src"]))


def test_eval_executor_refuses_the_op(ftx_lib, net, tps):
    five, three = tps
    program = ne.emit_program(net, dropout=True)
    ops = program.ops_array()
    d0 = sites(ops)[0]
    assert set(ops["segment"]) == {0, 1, 2}
    t = eh.tables(program)
    text = "ftx_spvcnn_eval: op %d (dropout): the eval program has no Dropout (it is the identity in eval mode)" % d0
    assert eh.size(ftx_lib, t) == 0 and ftx_lib.ftx_last_error().decode() == text
    assert eh.call(ftx_lib, t, arena=None, arena_bytes=1 << 40) == (FTX_EINVAL, text)


def test_plain_entries_refuse_a_program_with_the_op(ftx_lib, tps):
    five, three = tps
    t = th.train_tables(three)
    d0 = sites(t[1])[0]
    for direction in ("fwd", "bwd"):
        rc, msg = th.call(ftx_lib, t, direction, arena=None, arena_bytes=1 << 40)
        entry = "ftx_spvcnn_train_" + direction
        assert rc == FTX_EINVAL and msg == "%s: op %d is a Dropout, which draws from the random stream: call %s_rng with (seed, call_base)" % (entry, d0, entry), msg
        # and the _rng entries run a program without the op as the plain ones do
        rc, msg = rng_call(ftx_lib, th.train_tables(five), direction, arena=None)
        assert rc == FTX_EINVAL and "the arena must be a 256-byte aligned device buffer" in msg


# ---------------------------------------------------------------- the switch
def test_switch_is_off_by_default_and_changes_nothing_else(net):
    from fusiontransformer_amd.config import fusion_cfg, get_cfg_defaults, lidar_cfg
    from fusiontransformer_amd.models.build import build_model
    assert get_cfg_defaults().MODEL.lidar_native_dropout is False
    assert net.lidar_native_dropout is False and net.dropout_state() == {"seed": 0, "forwards": 0}
    assert nt.SEGMENTS == (0, 1, 2, 3, 4) and nt.TrainProgram(net).n_segments == 5
    for cfg, path in ((lidar_cfg(), "backbone"), (fusion_cfg("middle"), "lidar_backbone")):
        cfg.MODEL.vit_depth, cfg.MODEL.late_feat_block_number = 1, 0
        if cfg.MODEL.middle_feat_block_number:
            cfg.MODEL.middle_feat_block_number = 0
        for on in (False, True):
            cfg.MODEL.lidar_native_dropout = on
            torch.manual_seed(77)
            model = build_model(cfg)[0]
            spv = getattr(model, path)
            assert spv.lidar_native_dropout is on and spv.dropout_state() == {"seed": 77 if on else 0, "forwards": 0}
            assert spv.lidar_native_train is False and spv.lidar_native_eval is False and spv.lidar_native_index is False and spv.lidar_bf16 is False
            assert not [k for k in model.state_dict() if "drop" in k], "the state is not in the checkpoint"
    torch.manual_seed((1 << 64) - 3)
    s = SPVCNN().set_native_dropout(True)
    assert s.dropout_state() == {"seed": (1 << 64) - 3, "forwards": 0}
    s.set_native_dropout(True, seed=(1 << 64) + 5)
    assert s.dropout_state()["seed"] == 5, "masked to 64 bits"
    s._native_tr = object()
    s.set_native_dropout(False)
    assert s._native_tr is None and s.lidar_native_dropout is False, "the program is emitted again"
    s.set_dropout_state({"seed": 9, "forwards": 4})
    assert s.dropout_state() == {"seed": 9, "forwards": 4}
    with pytest.raises(ValueError):
        s.set_dropout_state({"seed": -1, "forwards": 0})
    with pytest.raises(RuntimeError, match="no training forward"):
        s.last_dropout_masks()
