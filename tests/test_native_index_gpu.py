"""The native index build of the SPVCNN LiDAR branch on the GPU (ftx_spvcnn_index_levels / _maps / _pairs, SPVCNN.set_native_index)
against the per-op Python build: every array bit for bit, eval logits, one training step, the C-caller path from points to point
features, and arenas across batches of different size.  Everything compared is an integer, or a float32 from the same arithmetic, so
every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import product_inputs, small_cfg

pytestmark = pytest.mark.gpu

STRIDES = (1, 2, 4, 8, 16)


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    """torch.equal, and the same bit patterns for floats (torch.equal alone takes -0.0 for 0.0)."""
    if a.shape != b.shape or a.dtype != b.dtype or not torch.equal(a, b):
        return False
    return a.dtype != torch.float32 or torch.equal(bits(a), bits(b))


def _spv(pres=1, vres=1):
    from fusiontransformer_amd.models.spvcnn import SPVCNN
    torch.manual_seed(0)
    return SPVCNN(pres=pres, vres=vres)


def _tensor(feats, coords):
    from fusiontransformer_amd.sparse import SparseTensor
    f = torch.from_numpy(np.ascontiguousarray(feats)).cuda()
    c = torch.from_numpy(np.ascontiguousarray(coords)).cuda()
    return SparseTensor(f, c)


def _drain(steps):
    syncs = 0
    while True:
        try:
            tok = next(steps)
            assert tok == "sync"
            syncs += 1
        except StopIteration as done:
            return done.value, syncs


def _build_both(feats, coords, pres=1, vres=1, grad=False):
    """((z, x0) of the per-op build, (z, x0) of the native build) of one batch, the native one without any fallback."""
    from fusiontransformer_amd import native_index as ni
    net = _spv(pres, vres)
    with torch.set_grad_enabled(grad):
        py, syncs = _drain(net._index_steps(_tensor(feats, coords), ahead=True))
        assert syncs == 2
        nat, syncs = _drain(ni.index_steps(_tensor(feats, coords), pres, vres))
        assert syncs == 2, "the native build yields once before each of its two host reads"
    torch.cuda.synchronize()
    return py, nat


def _assert_same_structures(py, nat, grad, what):
    (zp, xp), (zn, xn) = py, nat
    cp, cn = xp.cm, xn.cm
    assert same(cp.points, cn.points), what
    for l, s in enumerate(STRIDES):
        assert same(cp.coords[s], cn.coords[s]), (what, "coords", s)
        hp, fp, ip, kp, op = cp.level_data[s]
        hn, fn, i_n, kn, on = cn.level_data[s]
        assert same(hp, hn) and same(fp, fn) and ip == i_n == l and same(kp, kn) and same(op, on), (what, "level data", s)
        tp, tn = cp.tables[s], cn.tables[s]
        assert (tp.n, tp.capacity) == (tn.n, tn.capacity), (what, "table", s)
        rows = torch.arange(hp.shape[0], dtype=torch.int32, device="cuda")
        assert same(tn.query(hp), rows) and same(tp.query(hp), rows), (what, "table rows", s)
    assert set(cp.kernel_maps) == set(cn.kernel_maps) and len(cn.kernel_maps) == 9, what
    for key, kp in cp.kernel_maps.items():
        kn = cn.kernel_maps[key]
        for f in ("nbr", "pos", "pos_t", "pair_in", "pair_out", "koff", "out_coords"):
            assert same(getattr(kp, f), getattr(kn, f)), (what, key, f)
        for f in ("n_pairs", "n_in", "n_out", "kvol", "fine_bijective", "submanifold"):
            assert getattr(kp, f) == getattr(kn, f), (what, key, f)
            assert type(getattr(kp, f)) is type(getattr(kn, f)), (what, key, f)
    assert same(zp.C, zn.C) and same(zp.F, zn.F), what
    ap, an = zp.additional_features, zn.additional_features
    for s in (1, 16, 4):
        assert same(ap["idx_query"][s], an["idx_query"][s]) and same(ap["counts"][s], an["counts"][s]), (what, "voxel index", s)
        sp, sn = ap["vox_seg"][s], an["vox_seg"][s]
        assert sp.m == sn.m and same(sp.order, sn.order) and same(sp.seg_off, sn.seg_off), (what, "voxel segments", s)
        assert same(zp.idx_query[s], zn.idx_query[s]), (what, "corner rows", s)
        assert same(zp.weights[s], zn.weights[s]), (what, "trilinear weights", s)
        dp, dn = ap["devox_seg"][s], an["devox_seg"][s]
        if grad:
            assert dp.m == dn.m and same(dp.order, dn.order) and same(dp.seg_off, dn.seg_off), (what, "backward segments", s)
        else:
            assert dp is None and dn is None, (what, "backward segments", s)
    assert set(ap["idx_query"]) == set(an["idx_query"]) == {1, 16, 4} and set(zn.idx_query) == {1, 16, 4}
    assert same(xp.F, xn.F) and same(xp.C, xn.C) and xp.s == xn.s == 1, what
    rows, maps, pvs = xn.native_tables
    assert list(rows) == [cn.coords[s].shape[0] for s in STRIDES] + [zn.F.shape[0]]


def _cases():
    from fusiontransformer_amd.data.synth import make_batch
    rng = np.random.default_rng(5)
    out = {}
    b = make_batch([0, 1], max_points=2500)
    out["small"] = (b["feats"], b["coords"].astype(np.int32), 1, 1)
    b = make_batch([3])
    assert b["coords"].shape[0] > 10000
    out["kitti frame, batch 1"] = (b["feats"], b["coords"].astype(np.int32), 1, 1)
    b = make_batch([0, 1, 2, 3])
    assert b["coords"].shape[0] > 64000
    out["kitti frames, batch 4"] = (b["feats"], b["coords"].astype(np.int32), 1, 1)
    b = make_batch([10, 11], shape="nuscenes")
    out["nuscenes-shaped"] = (b["feats"], b["coords"].astype(np.int32), 1, 1)
    b = make_batch([4, 5], max_points=3000)
    c = b["coords"].astype(np.float32)
    c[:, :3] += rng.random((c.shape[0], 3), dtype=np.float32) * 0.999          # points inside their voxel: the trilinear weights are not 0 / 1
    pick = rng.integers(0, c.shape[0], size=c.shape[0] // 2)
    out["duplicated points"] = (np.concatenate([b["feats"], b["feats"][pick]]), np.concatenate([c, c[pick]]), 1, 1)
    out["float coordinates"] = (b["feats"], c, 1, 1)
    out["init_res != after_res"] = (b["feats"], c, 0.05, 0.1)
    out["init_res != after_res, ratio 3/7"] = (b["feats"], c, 3, 7)
    pts = np.unique(rng.integers(0, 8, size=(40, 3)), axis=0)
    tiny = np.concatenate([pts, np.zeros((pts.shape[0], 1), dtype=pts.dtype)], 1).astype(np.int32)
    out["tiny cloud"] = (rng.standard_normal((tiny.shape[0], 4)).astype(np.float32), tiny, 1, 1)
    out["one point"] = (np.ones((1, 4), np.float32), np.array([[3, 4, 5, 0]], np.int32), 1, 1)
    return out


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.mark.parametrize("grad", [False, True], ids=["no_grad", "enable_grad"])
@pytest.mark.parametrize("name", ["small", "kitti frame, batch 1", "kitti frames, batch 4", "nuscenes-shaped", "duplicated points", "float coordinates",
                                  "init_res != after_res", "init_res != after_res, ratio 3/7", "tiny cloud", "one point"])
def test_native_structures_equal_the_python_build(cases, name, grad):
    feats, coords, pres, vres = cases[name]
    py, nat = _build_both(feats, coords, pres, vres, grad)
    if name == "tiny cloud":
        assert nat[1].cm.coords[8].shape[0] == 1 and nat[1].cm.coords[16].shape[0] == 1
    if name.startswith("init_res"):
        assert not same(nat[0].C, torch.from_numpy(coords).cuda())
    _assert_same_structures(py, nat, grad, name)


def test_sort_workspace_bounds_cover_the_library_figure(ftx_lib):
    """The arenas reserve the sort temporaries by a bound (the sorting library's own figure needs a device): the bound holds at every size
    tried, with room; were it ever to fall short the phase answers FTX_EWORKSPACE before launching."""
    from fusiontransformer_amd import native_index as ni
    for n in (1, 100, 2500, 81237, 324948, 1_500_000):
        need = ftx_lib.ftx_levels_workspace_bytes(n, 5)
        lay = ni.layout(n, 4)
        reserved = lay["a_total"] - (lay["a_order"] + ((20 * n + 255) & ~255) + 256)      # what follows `order` and the level offsets
        print(f"level sort workspace at n = {n}: needs {need}, reserved {reserved}")
        assert 0 < need <= reserved, n


# ---------------------------------------------------------------- models
def _randomise_batchnorm(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            c = m.running_mean.shape[0]
            m.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(c, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(c, generator=g) * 0.2)


def _spvcnn(model, kind):
    return model.backbone if kind == "lidar" else (model.lidar_backbone.backbone if kind == "late" else model.lidar_backbone)


def _build(kind, seed=0):
    from fusiontransformer_amd.config import lidar_cfg
    from fusiontransformer_amd.models.build import build_model
    cfg = lidar_cfg() if kind == "lidar" else small_cfg(kind)
    torch.manual_seed(seed)
    built = build_model(cfg)
    model = built[0]
    _randomise_batchnorm(model, seed + 100)
    model = model.cuda()
    return cfg, model, _spvcnn(model, kind), built[1:]


def _forward(model, batch, prepare=None):
    pin = product_inputs(batch)
    if prepare is not None:
        prepare.prepare(pin["lidar"], wait=False)
        assert pin["lidar"].prepared is not None
    with torch.no_grad():
        out = model(pin)
    torch.cuda.synchronize()
    return out


def _same_outputs(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert same(a[k], b[k]), (what, k, (a[k] - b[k]).abs().max().item())


@pytest.fixture()
def count_native(monkeypatch):
    """How many batches went through the native builder to its end."""
    from fusiontransformer_amd import native_index as ni
    calls = []
    real = ni._structures
    monkeypatch.setattr(ni, "_structures", lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


@pytest.mark.parametrize("kind", ["lidar", "middle", "early", "late"])
def test_eval_logits_equal_the_switch_off(kind, count_native):
    from fusiontransformer_amd.data.synth import make_batch
    cfg, model, net, _ = _build(kind)
    model.eval()
    batch = make_batch([0, 1]) if kind in ("lidar", "middle") else make_batch([0, 1], max_points=2500)
    for native_eval in (False, True):
        net.set_native_eval(native_eval)
        net.set_native_index(False)
        off = _forward(model, batch)
        off_prepared = _forward(model, batch, prepare=net)
        assert not count_native
        net.set_native_index(True)
        assert net.lidar_native_eval is native_eval
        on = _forward(model, batch)
        assert len(count_native) == 1, "the native builder did not run"
        _same_outputs(on, off, (kind, native_eval))
        on_prepared = _forward(model, batch, prepare=net)
        assert len(count_native) == 2
        _same_outputs(on_prepared, off, (kind, native_eval, "prepare(wait=False)"))
        _same_outputs(off_prepared, off, (kind, native_eval, "prepare(wait=False), switch off"))
        for lvl in ("x0", "x1", "x2", "x3", "x4"):
            assert net.last_index[lvl].C.shape[1] == 4
        del count_native[:]
    net.set_native_index(False)
    _same_outputs(_forward(model, batch), off, (kind, "switched off again"))
    assert not count_native


def _level_rows(coords, stride):
    c = np.concatenate([coords[:, :3] // stride, coords[:, 3:]], 1)
    return len(np.unique(c, axis=0))


def _masks(coords, seed):
    g = torch.Generator().manual_seed(seed)
    return {"y1": (torch.rand(_level_rows(coords, 16), 256, generator=g) > 0.3).float().cuda(),
            "y3": (torch.rand(_level_rows(coords, 4), 128, generator=g) > 0.3).float().cuda()}


@pytest.mark.parametrize("kind", ["lidar", "middle"])
def test_train_steps_with_prefetch_equal_the_twin_with_the_switch_off(kind, count_native):
    """Two TrainSteps, each handing the next batch over for prefetch (SPVCNN.prepare(wait=False) inside the step): losses, every
    gradient and the parameters after Adam equal the twin's, whose index is built per op."""
    from fusiontransformer_amd.config import lidar_cfg
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    cfg = lidar_cfg() if kind == "lidar" else small_cfg("middle")
    torch.manual_seed(17)
    model, twin = build_model(cfg)[0], build_model(cfg)[0]
    twin.load_state_dict(model.state_dict())
    model, twin = model.cuda().train(), twin.cuda().train()
    net, net_twin = _spvcnn(model, kind), _spvcnn(twin, kind)
    net.set_native_index(True)
    assert net_twin.lidar_native_index is False
    step, step_twin = TrainStep(cfg, model), TrainStep(cfg, twin)
    batches = [make_batch([0, 1], max_points=6000), make_batch([2, 3], max_points=5000)]
    nxt = nxt_twin = None
    for s, which in enumerate((0, 1)):
        b = batches[which]
        pin = nxt if nxt is not None else product_inputs(b)
        pin_twin = nxt_twin if nxt_twin is not None else product_inputs(b)
        nxt, nxt_twin = product_inputs(batches[1 - which]), product_inputs(batches[1 - which])
        masks = _masks(b["coords"], 60 + s)
        net.dropout_masks = net_twin.dropout_masks = masks
        preds = step(pin, next_batch=nxt)
        preds_twin = step_twin(pin_twin, next_batch=nxt_twin)
        torch.cuda.synchronize()
        assert nxt["lidar"].prepared is not None and nxt_twin["lidar"].prepared is not None, "the prefetch did not start"
        for k in preds:
            assert same(preds[k], preds_twin[k]), (s, k)
        assert step.last.keys() == step_twin.last.keys()
        for k in step.last:
            assert same(step.last[k], step_twin.last[k]), (s, k)
        gt = dict(twin.named_parameters())
        n_grads = 0
        for n, p in model.named_parameters():
            assert (p.grad is None) == (gt[n].grad is None), (s, n)
            if p.grad is not None:
                assert same(p.grad, gt[n].grad), (s, n)
                n_grads += 1
        assert n_grads > 50
        for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
            assert same(p.detach(), q.detach()), (s, n)
    assert len(count_native) >= 2, "the native builder did not run in training"
    z = net.last_index["z"]
    assert all(z.additional_features["devox_seg"][s_] is not None for s_ in (1, 16, 4)), "training builds the backward's segments"


# ---------------------------------------------------------------- the C-caller path
def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def plain_arena(nbytes):
    return torch.empty(nbytes, dtype=torch.uint8, device="cuda")


def c_caller_inputs():
    """(feats (n, c_in), coords (n, 4) float32, the batch) of the C-caller recipe: two frames, at most 4000 points each."""
    from fusiontransformer_amd.data.synth import make_batch
    batch = make_batch([6, 7], max_points=4000)
    return torch.from_numpy(batch["feats"]).cuda(), torch.from_numpy(batch["coords"]).float().cuda().contiguous(), batch


def c_caller_index(L, feats, coords, arena=plain_arena, with_backward_segments=0, after=None):
    """ctypes only, no CoordinateManager: the three phases on arenas from arena(nbytes) (uint8, of exactly the phase's own figure);
    after(phase, arena), when given, runs behind every phase.  Returns the arenas, the two host reads and the tables phase C wrote."""
    from fusiontransformer_amd import native_eval as ne
    from fusiontransformer_amd import functional as spf
    n, c_in = feats.shape
    st = spf.stream()
    bwd = int(with_backward_segments)

    def sized(nbytes):
        assert nbytes > 0, L.ftx_last_error()
        return arena(nbytes)
    done = after or (lambda phase, buf: None)
    pinned = torch.empty(16, dtype=torch.int32, pin_memory=True)
    a = sized(L.ftx_spvcnn_index_levels_arena_bytes(n))
    spf.check(L.ftx_spvcnn_index_levels(coords.data_ptr(), n, 1.0, 1.0, a.data_ptr(), a.shape[0], pinned.data_ptr(), st), "levels")
    torch.cuda.current_stream().synchronize()                                   # host read 1
    done("levels", a)
    off = np.array(pinned[:6].tolist(), dtype=np.int32)
    b = sized(L.ftx_spvcnn_index_maps_arena_bytes(n, c_in, _np_ptr(off), bwd))
    assert L.ftx_spvcnn_index_maps(coords.data_ptr(), n, 1.0, 1.0, feats.data_ptr(), c_in, _np_ptr(off), bwd, a.data_ptr(), a.shape[0], b.data_ptr(),
                                   b.shape[0] - 256, pinned.data_ptr(), st) == -3, "an arena that is too small is refused"
    spf.check(L.ftx_spvcnn_index_maps(coords.data_ptr(), n, 1.0, 1.0, feats.data_ptr(), c_in, _np_ptr(off), bwd, a.data_ptr(), a.shape[0], b.data_ptr(),
                                      b.shape[0], pinned.data_ptr(), st), "maps")
    torch.cuda.current_stream().synchronize()                                   # host read 2
    done("maps", b)
    pairs = np.array(pinned[:5].tolist(), dtype=np.int32)
    c = sized(L.ftx_spvcnn_index_pairs_arena_bytes(n, _np_ptr(off), _np_ptr(pairs)))
    rows, maps, pvs = np.zeros(6, np.int64), np.zeros(9, ne.MAP), np.zeros(3, ne.PV)
    x0 = ctypes.c_void_p()
    spf.check(L.ftx_spvcnn_index_pairs(n, c_in, _np_ptr(off), bwd, _np_ptr(pairs), a.data_ptr(), b.data_ptr(), b.shape[0], c.data_ptr(), c.shape[0], _np_ptr(rows),
                                       _np_ptr(maps), _np_ptr(pvs), ctypes.byref(x0), st), "pairs")
    torch.cuda.current_stream().synchronize()
    done("pairs", c)
    assert list(maps["n_pairs"][:5]) == list(pairs) and rows[5] == n and x0.value
    return dict(a=a, b=b, c=c, off=off, pairs=pairs, rows=rows, maps=maps, pvs=pvs, x0=x0, n=n, c_in=c_in, bwd=bwd)


def c_caller_eval(L, net, t, arena=plain_arena):
    """ftx_spvcnn_eval on the tables c_caller_index returned: the model side (program, layer table, routes: the host's one routing rule,
    from the tables alone), an arena of exactly ftx_spvcnn_eval_arena_bytes from arena(nbytes).  Returns (z3, the arena)."""
    from fusiontransformer_amd import native_eval as ne
    from fusiontransformer_amd import functional as spf
    rows, maps, pvs = t["rows"], t["maps"], t["pvs"]
    ex = ne.NativeEval(net)
    layers = ex.model_table()
    km = lambda m: type("KM", (), dict(n_pairs=int(m["n_pairs"]), n_in=int(m["n_in"]), n_out=int(m["n_out"]), kvol=int(m["kvol"]),
                                       fine_bijective=bool(m["fine_bijective"]), submanifold=not m["fine_bijective"]))()
    kms = [km(m) for m in maps]
    routes = np.zeros(len(ex.program.ops), dtype=np.int32)
    for i, op in enumerate(ex.program.ops):
        kind, layer, map_, level = op[0], op[2], op[3], op[8]
        if kind == ne.OP_LINEAR_BN or (kind == ne.OP_CONV_BN and map_ < 0):
            routes[i] = ne.ROUTE_ROWS
        elif kind == ne.OP_CONV_BN:
            l = layers[layer]
            routes[i] = ne.ROUTES[spf._conv_route(kms[map_], bool(l["transposed"]), int(l["ca"]), int(l["co"]), int(l["kvol"]), int(rows[level]), False)]
    need = ne.arena_bytes(layers, ex.ops, rows, maps, pvs, routes)
    work = arena(need)
    z3 = torch.empty((t["n"], ex.program.out_channels), dtype=torch.float32, device="cuda")
    spf._stream_scratch()
    spf.check(L.ftx_spvcnn_eval(_np_ptr(layers), len(layers), _np_ptr(ex.ops), len(ex.ops), _np_ptr(rows), _np_ptr(maps), 9, _np_ptr(pvs), 3, _np_ptr(routes),
                                t["x0"], 0, 2, None, None, work.data_ptr(), need, z3.data_ptr(), spf.stream()), "ftx_spvcnn_eval")
    torch.cuda.synchronize()
    return z3, work


def test_c_caller_path_from_points_to_point_features(ftx_lib):
    """ctypes only, no CoordinateManager: the three phases, then ftx_spvcnn_eval on the tables phase C wrote; z3 equals the point features
    of the Python path (switches off)."""
    L = ftx_lib
    cfg, model, net, _ = _build("lidar", seed=2)
    model.eval()
    feats, coords, batch = c_caller_inputs()
    z3, _ = c_caller_eval(L, net, c_caller_index(L, feats, coords))
    from fusiontransformer_amd.sparse import SparseTensor
    with torch.no_grad():
        ref = net(SparseTensor(feats, torch.from_numpy(batch["coords"]).int().cuda()))
    torch.cuda.synchronize()
    assert net.lidar_native_index is False and net.lidar_native_eval is False
    assert same(z3, ref)


def test_alternating_batches_of_different_size(count_native):
    """Two batches of different size alternate through one model: every batch gets arenas of its own size, results stay those of a fresh
    model with the switch off, and the structures of an earlier batch stay valid while a later one is built."""
    from fusiontransformer_amd import native_index as ni
    from fusiontransformer_amd.data.synth import make_batch
    a, b = make_batch([5], max_points=1200), make_batch([6, 7], max_points=4000)
    cfg, model, net, _ = _build("middle", seed=3)
    model.eval()
    net.set_native_index(True).set_native_eval(True)
    outs = [_forward(model, x) for x in (a, b, a, b)]
    assert len(count_native) == 4
    _, fresh, fnet, _ = _build("middle", seed=3)
    fresh.eval()
    for x, idx in ((a, (0, 2)), (b, (1, 3))):
        ref = _forward(fresh, x)
        for i in idx:
            _same_outputs(outs[i], ref, ("alternating", i))
    # structures of batch `a` built first, then `b` built over whatever the allocator hands out, then `a` compared: nothing was reused under it
    spv = _spv()
    with torch.no_grad():
        first, _ = _drain(ni.index_steps(_tensor(a["feats"], a["coords"].astype(np.int32)), 1, 1))
        second, _ = _drain(ni.index_steps(_tensor(b["feats"], b["coords"].astype(np.int32)), 1, 1))
        py_a, _ = _drain(spv._index_steps(_tensor(a["feats"], a["coords"].astype(np.int32)), ahead=True))
        py_b, _ = _drain(spv._index_steps(_tensor(b["feats"], b["coords"].astype(np.int32)), ahead=True))
    torch.cuda.synchronize()
    _assert_same_structures(py_a, first, False, "first of two live batches")
    _assert_same_structures(py_b, second, False, "second of two live batches")
