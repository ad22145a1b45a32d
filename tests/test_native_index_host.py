"""Host side of the native index build (include/ftx.h: ftx_spvcnn_index_levels / _maps / _pairs): arena sizes as pure host functions,
the layout every view is cut from, argument validation before anything touches a device, and the switch.  No GPU: every call here is
refused, or answers, before its first launch."""
import ctypes

import numpy as np
import pytest
import torch

from fusiontransformer_amd import native_eval as ne
from fusiontransformer_amd import native_index as ni
from fusiontransformer_amd.models.spvcnn import SPVCNN

FTX_EINVAL, FTX_EWORKSPACE = -1, -3
FAKE = ctypes.c_void_p(1 << 20)       # a non-null, 256-byte aligned "device address" for arguments that are only validated
HUGE = 1 << 40

OFF = np.array([0, 1000, 1600, 1900, 2020, 2060], dtype=np.int32)       # level sizes 1000, 600, 300, 120, 40
PAIRS = np.array([5000, 3000, 1500, 600, 200], dtype=np.int32)
N, C = 1500, 4


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def err(lib):
    return lib.ftx_last_error().decode()


def test_arena_sizes_are_host_functions_monotone_and_aligned(ftx_lib):
    L = ftx_lib
    prev = 0
    for n in (1, 2, 7, 255, 256, 1500, 81237, 324948, 2_000_000):
        a = L.ftx_spvcnn_index_levels_arena_bytes(n)
        assert a > 0 and a % 256 == 0 and a >= prev, n
        assert a == L.ftx_spvcnn_index_levels_arena_bytes(n)
        prev = a
    # B: monotone in n, in c_in, in every level size, in the backward flag
    base = L.ftx_spvcnn_index_maps_arena_bytes(N, C, p(OFF), 0)
    assert base > 0 and base % 256 == 0
    assert L.ftx_spvcnn_index_maps_arena_bytes(N + 1, C, p(OFF), 0) >= base
    assert L.ftx_spvcnn_index_maps_arena_bytes(N, C + 4, p(OFF), 0) > base
    with_bwd = L.ftx_spvcnn_index_maps_arena_bytes(N, C, p(OFF), 1)
    assert with_bwd > base and with_bwd % 256 == 0
    pairs_base = L.ftx_spvcnn_index_pairs_arena_bytes(N, p(OFF), p(PAIRS))
    assert pairs_base > 0 and pairs_base % 256 == 0
    sizes = np.diff(OFF)
    for l in range(5):
        grown = sizes.copy()
        grown[:l + 1] += 7                                           # level l and every finer one: the sizes stay non-increasing
        off = np.concatenate([[0], np.cumsum(grown)]).astype(np.int32)
        n = N
        b = L.ftx_spvcnn_index_maps_arena_bytes(n, C, p(off), 0)
        assert b >= L.ftx_spvcnn_index_maps_arena_bytes(n, C, p(OFF), 0) and b % 256 == 0, l
        assert L.ftx_spvcnn_index_pairs_arena_bytes(n, p(off), p(PAIRS)) >= L.ftx_spvcnn_index_pairs_arena_bytes(n, p(OFF), p(PAIRS)), l
        more = PAIRS.copy()
        more[l] += 100
        c = L.ftx_spvcnn_index_pairs_arena_bytes(N, p(OFF), p(more))
        assert c > pairs_base and c % 256 == 0, l
    assert ni.levels_arena_bytes(N) == L.ftx_spvcnn_index_levels_arena_bytes(N)
    assert ni.maps_arena_bytes(N, C, OFF, True) == with_bwd and ni.pairs_arena_bytes(N, OFF, PAIRS) == pairs_base


def test_layout_regions_are_aligned_disjoint_and_inside_their_arena(ftx_lib):
    assert ftx_lib.ftx_spvcnn_index_layout_words() == len(ni.WORDS) and len(set(ni.WORDS)) == len(ni.WORDS)
    lay = ni.layout(N, C, OFF, PAIRS, True)
    assert lay["a_total"] == ni.levels_arena_bytes(N) and lay["b_total"] == ni.maps_arena_bytes(N, C, OFF, True)
    assert lay["c_total"] == ni.pairs_arena_bytes(N, OFF, PAIRS)
    sizes = [int(s) for s in np.diff(OFF)]
    regions = {"a": [("a_coords", 16 * N), ("a_points", 16 * N), ("a_uniq", 40 * N), ("a_first", 20 * N), ("a_skeys", 40 * N), ("a_order", 20 * N)],
               "b": [("x0", 4 * sizes[0] * C)], "c": []}
    for l in range(5):
        regions["b"] += [(f"coords{l}", 16 * sizes[l]), (f"tkeys{l}", 8 * lay[f"cap{l}"]), (f"tvals{l}", 4 * lay[f"cap{l}"])]
        assert lay[f"cap{l}"] == ftx_lib.ftx_hashtable_capacity(sizes[l])
        regions["c"] += [(f"pos_t{l}", 4 * 27 * sizes[l]), (f"pair_in{l}", 4 * int(PAIRS[l])), (f"pair_out{l}", 4 * int(PAIRS[l]))]
    for m, (ks, s, stride) in enumerate(ne.MAP_KEYS):
        l = ne.STRIDES.index(s)
        k, n_out = ks ** 3, sizes[l] if stride == 1 else sizes[l + 1]
        regions["b"] += [(f"nbr{m}", 4 * k * n_out), (f"pos{m}", 4 * k * n_out), (f"koff{m}", 4 * (k + 1))]
        if stride == 2:
            regions["b"] += [(f"pos_t{m}", 4 * 8 * sizes[l]), (f"pair_in{m}", 4 * sizes[l]), (f"pair_out{m}", 4 * sizes[l])]
    for j, s in enumerate(ne.PV_STRIDES):
        m = sizes[ne.STRIDES.index(s)]
        regions["b"] += [(f"vidx{j}", 4 * N), (f"vcnt{j}", 4 * m), (f"vseg{j}", 4 * (m + 1)), (f"didx{j}", 32 * N), (f"dw{j}", 32 * N),
                         (f"dorder{j}", 32 * N), (f"dseg{j}", 4 * (m + 1))]
    for arena, items in regions.items():
        spans = sorted((lay[name], lay[name] + nbytes, name) for name, nbytes in items)
        for (lo, hi, name), nxt in zip(spans, spans[1:] + [(lay[arena + "_total"], 0, "end")]):
            # the three sorted entry lists of the backward lie back to back in one region: 4-byte entries, as the per-level rows of `order`
            assert lo % (4 if name.startswith("dorder") else 256) == 0, name
            assert hi <= nxt[0], (name, nxt[2])
    # without the backward flag the segment regions are absent, and the arena is smaller
    lay0 = ni.layout(N, C, OFF, None, False)
    assert lay0["b_total"] < lay["b_total"] and lay0["c_total"] == 0 and lay0["dorder0"] == 0
    assert ni.layout(N, C)["b_total"] == 0


def test_table_records_have_the_executors_strides(ftx_lib):
    """Phase C writes rows[6], map_t[9], pv_t[3] into the caller's host arrays: the binding's records are the library's."""
    assert ne.MAP.itemsize == ftx_lib.ftx_spvcnn_map_bytes() == 80 and ne.PV.itemsize == ftx_lib.ftx_spvcnn_pv_bytes() == 64
    assert len(ne.MAP_KEYS) == 9 and ne.MAP_KEYS[:5] == tuple((3, s, 1) for s in (1, 2, 4, 8, 16)) and ne.PV_STRIDES == (1, 16, 4)


def _levels(lib, coords=FAKE, n=N, ir=1.0, ar=1.0, arena=FAKE, nbytes=HUGE, pinned=FAKE):
    return lib.ftx_spvcnn_index_levels(coords, n, ir, ar, arena, nbytes, pinned, None)


def _maps(lib, off=OFF, n=N, c=C, coords=FAKE, feats=FAKE, bwd=0, a=FAKE, a_bytes=HUGE, b=FAKE, b_bytes=HUGE, pinned=FAKE):
    return lib.ftx_spvcnn_index_maps(coords, n, 1.0, 1.0, feats, c, None if off is None else p(off), bwd, a, a_bytes, b, b_bytes, pinned, None)


def _pairs(lib, pairs=PAIRS, off=OFF, n=N, a=FAKE, b=FAKE, b_bytes=HUGE, c=FAKE, c_bytes=HUGE, tables=True):
    rows, maps, pvs = np.zeros(6, np.int64), np.zeros(9, ne.MAP), np.zeros(3, ne.PV)
    return lib.ftx_spvcnn_index_pairs(n, C, None if off is None else p(off), 0, None if pairs is None else p(pairs), a, b, b_bytes, c, c_bytes,
                                      p(rows) if tables else None, p(maps), p(pvs), None, None)


def test_levels_refuses_bad_arguments_before_any_launch(ftx_lib):
    L = ftx_lib
    for n in (0, -5):
        assert _levels(L, n=n) == FTX_EINVAL and "n < 1" in err(L)
    assert L.ftx_spvcnn_index_levels_arena_bytes(0) == 0 and "n < 1" in err(L)
    assert _levels(L, n=1 << 28) == FTX_EINVAL and "too large" in err(L)
    assert _levels(L, coords=None) == FTX_EINVAL and "null pointer" in err(L)
    assert _levels(L, pinned=None) == FTX_EINVAL and "null pointer" in err(L)
    assert _levels(L, coords=ctypes.c_void_p((1 << 20) + 4)) == FTX_EINVAL and "16-byte aligned" in err(L)
    assert _levels(L, ar=0.0) == FTX_EINVAL and "positive" in err(L)
    assert _levels(L, arena=None) == FTX_EINVAL and "256-byte aligned" in err(L)
    assert _levels(L, arena=ctypes.c_void_p((1 << 20) + 64)) == FTX_EINVAL and "256-byte aligned" in err(L)
    need = L.ftx_spvcnn_index_levels_arena_bytes(N)
    assert _levels(L, nbytes=need - 256) == FTX_EWORKSPACE and "ftx_spvcnn_index_levels_arena_bytes" in err(L)


def test_maps_refuses_bad_arguments_before_any_launch(ftx_lib):
    L = ftx_lib
    assert _maps(L, n=0) == FTX_EINVAL and "n < 1" in err(L)
    assert _maps(L, off=None) == FTX_EINVAL and "null level offsets" in err(L)
    for c in (0, 3, 6, 2048):
        assert _maps(L, c=c) == FTX_EINVAL and "multiple of 4" in err(L), c
    bad = {"start": [5, 1000, 1600, 1900, 2020, 2060], "empty level": [0, 1000, 1600, 1900, 1900, 1940], "descending": [0, 1000, 900, 1200, 1300, 1340],
           "above n": [0, 1501, 2101, 2401, 2521, 2561], "coarser larger than finer": [0, 600, 1600, 1900, 2020, 2060]}
    for what, off in bad.items():
        off = np.array(off, dtype=np.int32)
        assert _maps(L, off=off) == FTX_EINVAL and ("level" in err(L)), what
        assert L.ftx_spvcnn_index_maps_arena_bytes(N, C, p(off), 0) == 0, what
        assert _pairs(L, off=off) == FTX_EINVAL, what
    assert _maps(L, coords=None) == FTX_EINVAL and "null pointer" in err(L)
    assert _maps(L, feats=None) == FTX_EINVAL and "null pointer" in err(L)
    assert _maps(L, pinned=None) == FTX_EINVAL and "null pointer" in err(L)
    assert _maps(L, b=None) == FTX_EINVAL and "256-byte aligned" in err(L)
    assert _maps(L, a=ctypes.c_void_p((1 << 20) + 128)) == FTX_EINVAL and "256-byte aligned" in err(L)
    need = L.ftx_spvcnn_index_maps_arena_bytes(N, C, p(OFF), 0)
    assert _maps(L, b_bytes=need - 256) == FTX_EWORKSPACE and "arena" in err(L)
    assert _maps(L, a_bytes=L.ftx_spvcnn_index_levels_arena_bytes(N) - 256) == FTX_EWORKSPACE and "arena" in err(L)
    assert _maps(L, bwd=1, b_bytes=need) == FTX_EWORKSPACE, "the arena of a build without backward segments does not hold one with them"


def test_pairs_refuses_bad_arguments_before_any_launch(ftx_lib):
    L = ftx_lib
    assert _pairs(L, pairs=None) == FTX_EINVAL and "null" in err(L)
    for l in range(5):
        over = PAIRS.copy()
        over[l] = 27 * int(np.diff(OFF)[l]) + 1
        assert _pairs(L, pairs=over) == FTX_EINVAL and "outside 0 .. 27" in err(L), l
        assert L.ftx_spvcnn_index_pairs_arena_bytes(N, p(OFF), p(over)) == 0
        neg = PAIRS.copy()
        neg[l] = -1
        assert _pairs(L, pairs=neg) == FTX_EINVAL and "outside 0 .. 27" in err(L), l
    assert _pairs(L, tables=False) == FTX_EINVAL and "null table" in err(L)
    assert _pairs(L, c=None) == FTX_EINVAL and "256-byte aligned" in err(L)
    need = L.ftx_spvcnn_index_pairs_arena_bytes(N, p(OFF), p(PAIRS))
    assert _pairs(L, c_bytes=need - 256) == FTX_EWORKSPACE and "arena" in err(L)
    assert _pairs(L, b_bytes=256) == FTX_EWORKSPACE and "arena" in err(L)
    with pytest.raises(ni.Refused, match="outside 0 .. 27"):
        ni.layout(N, C, OFF, np.array([1 << 30] * 5, dtype=np.int32))


def test_switch_is_off_by_default_and_reaches_every_model():
    from fusiontransformer_amd.config import fusion_cfg, lidar_cfg
    from fusiontransformer_amd.models.build import build_model
    torch.manual_seed(0)
    net = SPVCNN()
    assert net.lidar_native_index is False and net.lidar_native_eval is False
    assert SPVCNN(lidar_native_index=True).lidar_native_index is True
    for cfg, path in ((lidar_cfg(), "backbone"), (fusion_cfg("middle"), "lidar_backbone"), (fusion_cfg("early"), "lidar_backbone"),
                      (fusion_cfg("late"), "lidar_backbone.backbone")):
        cfg.MODEL.vit_depth = 1
        cfg.MODEL.late_feat_block_number = 0
        if cfg.MODEL.middle_feat_block_number:
            cfg.MODEL.middle_feat_block_number = 0
        for on in (False, True):
            cfg.MODEL.lidar_native_index = on
            spv = build_model(cfg)[0]
            for name in path.split("."):
                spv = getattr(spv, name)
            assert spv.lidar_native_index is on
            assert spv.lidar_native_eval is False, "independent of the executor's switch"
    assert net.set_native_index(True) is net and net.lidar_native_index is True
    net.set_native_eval(True)
    net.set_native_index(False)
    assert net.lidar_native_eval is True and net.lidar_native_index is False


def test_cpu_tensors_take_the_existing_path(monkeypatch):
    """With the switch on, a batch on the CPU never reaches the library's builder: the per-op path answers (it has no CPU fallback)."""
    def never(*a, **k):
        raise AssertionError("the native builder was given CPU tensors")
    monkeypatch.setattr(ni, "index_steps", never)
    torch.manual_seed(0)
    net = SPVCNN().set_native_index(True)
    x = type("X", (), {"F": torch.zeros(8, 4), "C": torch.zeros(8, 4, dtype=torch.int32)})()
    with pytest.raises(ValueError, match="CUDA"):
        next(net._index_steps(x, ahead=True))
