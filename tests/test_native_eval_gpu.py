"""The native eval-mode path of the SPVCNN LiDAR branch on the GPU: the reduce that carries the eval BatchNorm
(ftx_spconv_reduce_bn_eval) against reduce + BatchNorm bit for bit and against float64, the two row kernels of the executor, and the
executor (ftx_spvcnn_eval, SPVCNN.set_native_eval) against the Python path bit for bit on every model that holds an SPVCNN."""
import numpy as np
import pytest
import torch

from tests import norm_ref as R
from tests import spconv_regimes as S
from tests.helpers import oracle_inputs, product_inputs, small_cfg
from tests.norm_ref import gen, randn, whole
from tests.test_spconv_regimes_gpu import bench_maps, get_map  # noqa: F401

pytestmark = pytest.mark.gpu
EPS = float(np.float32(1e-5))
TOL = 1e-3   # the project's eval gate (tests/test_model_gpu.py::test_eval_logits_match_oracle)


@pytest.fixture(scope="module")
def env():
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    yield spf, _lib.load()
    print("\nreduce_bn_eval: worst error / bound against float64: %.3g" % R.WORST.get("reduce_bn_eval", 0.0))


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    """torch.equal, and the same bit patterns (torch.equal alone takes -0.0 for 0.0)."""
    return a.shape == b.shape and torch.equal(a, b) and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------- the kernel
# production maps at full size: the 3x3x3 layers of tests/spconv_regimes.py plus the coarsest and second-finest level, and the strided
# 2x2x2 convolutions of the four stages (kvol 8, reduced through the coarse side)
REDUCE_CASES = [(e["name"], e["map"], e["co"]) for e in S.PRODUCTION if e["form"] == "conv"] + [
    ("64->64 L2", ("subm", 2), 64), ("256->256 L16", ("subm", 16), 256),
    ("down 32->32 L1->L2", ("down", 1), 32), ("down 32->32 L2->L4", ("down", 2), 32), ("down 64->64 L4->L8", ("down", 4), 64),
    ("down 128->128 L8->L16", ("down", 8), 128)]


@pytest.mark.parametrize("name,spec,co", REDUCE_CASES, ids=[c[0] for c in REDUCE_CASES])
def test_reduce_bn_eval_is_reduce_then_bn_eval(env, bench_maps, name, spec, co):
    spf, L = env
    km = get_map(bench_maps, spec)
    n, kvol, P = km.n_out, km.kvol, km.n_pairs
    assert kvol in (8, 27) and n == S.BENCH_VOXELS[spec[1] if spec[0] == "subm" else 2 * spec[1]]
    g = gen(17 * n + co)
    tmp = randn(g, P, co)
    gam, bet = torch.rand(co, generator=g).float() + 0.5, randn(g, co, scale=0.5)
    rm = randn(g, co, scale=0.3)
    rv = (10.0 ** (torch.rand(co, generator=g) * 9 - 6)).float()           # 1e-6 .. 1e3
    rv[3], rv[4] = 1e-6, 1e3
    res = randn(g, n, co)
    # planted columns: 0 -- every sum, mean and shift exactly 0, so the pre-activation is exactly 0 (or exactly the residual, which is
    # planted to -1 / 0 / +1); 1 -- negative everywhere; 2 -- positive everywhere; the rest mix signs
    tmp[:, 0], rm[0], bet[0] = 0.0, 0.0, 0.0
    res[:, 0] = torch.randint(-1, 2, (n,), generator=g).float()
    bet[1], bet[2] = -1e4, 1e4
    tmp_d, gam_d, bet_d, rm_d, rv_d, res_d = (t.cuda() for t in (tmp, gam, bet, rm, rv, res))
    x = torch.empty((n, co), dtype=torch.float32, device="cuda")
    spf.check(L.ftx_spconv_reduce(tmp_d.data_ptr(), km.pos.data_ptr(), n, co, kvol, x.data_ptr(), spf.stream()), "ftx_spconv_reduce")
    x64 = x.cpu().double()
    for with_res in (False, True):
        for relu in (False, True):
            what = f"{name} res={with_res} relu={relu}"
            r_d = res_d if with_res else None
            two = spf.batch_norm(x, gam_d, bet_d, rm_d, rv_d, False, 0.1, EPS, residual=r_d, relu=relu)
            one = spf.spconv_reduce_bn_eval(tmp_d, km.pos, n, gam_d, bet_d, rm_d, rv_d, EPS, residual=r_d, relu=relu)
            assert torch.equal(one, two), what
            assert same(one, two), what + ": bit patterns differ"
            y = one.cpu()
            if relu:
                assert (y[:, 1] == 0).all() and (y[:, 2] > 0).all() and (y[:, 0] >= 0).all()
                assert (y[:, 0] == (res[:, 0].clamp_min(0) if with_res else 0)).all()
            else:
                assert (y[:, 1] < 0).all() and (y[:, 0] == (res[:, 0] if with_res else 0)).all()
            # against float64 on the float64 copy of the fp32 reduce output, norm_ref.bn_eval's own bound
            r64 = res.double() if with_res else None
            ref, pre, bound = R.bn_eval(x64, rm.double(), rv.double(), EPS, gam.double(), bet.double(), r64, relu)
            mu, var = R.bn_stats(x64)
            batch, _, _ = R.bn_apply(x64, mu, R.bn_invstd(var, EPS), gam.double(), bet.double(), r64, relu)
            if relu:    # one element's mask flipped: the most negative pre-activation passed through
                k = int(torch.argmin(pre.reshape(-1)))
                ix = (k // co, k % co)
                second = [(ix, pre[ix])]
            else:       # one row's normalised term dropped
                r = int(torch.argmax((x64[:, 5:] - rm.double()[5:]).abs().sum(1)))
                second = [((r,), -(x64[r] - rm.double()) * R.bn_invstd(rv.double(), EPS) * gam.double())]
            R.check("reduce_bn_eval", what, one, ref, bound, [whole(batch - ref), second])


def test_reduce_bn_eval_on_an_empty_map_and_empty_output(env):
    """No pair at all (every position is -1): the rows reduce to 0 and take the BatchNorm of 0, as reduce + bn_eval; n = 0 launches nothing."""
    spf, L = env
    g = gen(3)
    for kvol in (8, 27):
        n, co = 37, 32
        pos = torch.full((kvol, n), -1, dtype=torch.int32, device="cuda")
        tmp = torch.empty((0, co), dtype=torch.float32, device="cuda")
        gam, bet, rm, rv = (t.cuda() for t in (torch.rand(co, generator=g) + 0.5, randn(g, co), randn(g, co), torch.rand(co, generator=g) + 0.1))
        res = randn(g, n, co).cuda()
        one = spf.spconv_reduce_bn_eval(tmp, pos, n, gam, bet, rm, rv, EPS, residual=res, relu=True)
        two = spf.batch_norm(torch.zeros((n, co), device="cuda"), gam, bet, rm, rv, False, 0.1, EPS, residual=res, relu=True)
        assert same(one, two)
        out = spf.spconv_reduce_bn_eval(tmp, pos[:, :0].contiguous(), 0, gam, bet, rm, rv, EPS)
        assert out.shape == (0, co)


@pytest.mark.parametrize("transposed", [False, True])
def test_conv_bn_eval_matches_conv_then_bn_on_every_route(env, bench_maps, transposed):
    """functional.conv_bn_eval (what SPVCNN runs per layer with the switch on where the executor does not) against sparse_conv +
    batch_norm(eval): pairs, output-stationary, direct and empty routes."""
    spf, _ = env
    from fusiontransformer_amd.sparse import KernelMap
    g = gen(11)
    cases = [(("subm", 8), 64, 128), (("subm", 16), 32, 32), (("down", 8), 128, 128)] if not transposed else [(("down", 8), 128, 96)]
    for spec, ca, co in cases:
        km = get_map(bench_maps, spec)
        n_in, n_out = (km.n_out, km.n_in) if transposed else (km.n_in, km.n_out)
        feats = randn(g, n_in, ca).cuda()
        w = randn(g, km.kvol, ca, co, scale=(ca * km.kvol) ** -0.5).cuda()
        gam, bet, rm, rv = (t.cuda() for t in (torch.rand(co, generator=g) + 0.5, randn(g, co), randn(g, co), torch.rand(co, generator=g) + 0.1))
        res = randn(g, n_out, co).cuda()
        with torch.no_grad():
            two = spf.batch_norm(spf.sparse_conv(feats, w, km, transposed), gam, bet, rm, rv, False, 0.1, EPS, residual=res, relu=True)
            one = spf.conv_bn_eval(feats, w, km, transposed, gam, bet, rm, rv, EPS, residual=res, relu=True)
        assert same(one, two), (spec, ca, co, spf._conv_route(km, transposed, ca, co, km.kvol, n_out, False))
    if not transposed:      # a map without a single pair: the _EMPTY route
        n, ca, co, kvol = 50, 32, 64, 27
        neg = lambda *s: torch.full(s, -1, dtype=torch.int32, device="cuda")
        none = torch.empty((0,), dtype=torch.int32, device="cuda")
        km = KernelMap(neg(kvol, n), neg(kvol, n), neg(kvol, n), none, none, torch.zeros(kvol + 1, dtype=torch.int32, device="cuda"), 0, n, n, None)
        assert spf._conv_route(km, False, ca, co, kvol, n, False) == spf._EMPTY
        feats, w = randn(g, n, ca).cuda(), randn(g, kvol, ca, co).cuda()
        gam, bet, rm, rv = (t.cuda() for t in (torch.rand(co, generator=g) + 0.5, randn(g, co), randn(g, co), torch.rand(co, generator=g) + 0.1))
        with torch.no_grad():
            two = spf.batch_norm(spf.sparse_conv(feats, w, km, False), gam, bet, rm, rv, False, 0.1, EPS, relu=False)
            one = spf.conv_bn_eval(feats, w, km, False, gam, bet, rm, rv, EPS, relu=False)
        assert same(one, two) and (one == one[0]).all()


@pytest.mark.parametrize("n", [0, 1, 7, 81237])
def test_rows_concat_and_rows_add_equal_torch(env, n):
    spf, _ = env
    g = gen(n + 1)
    for ca, cb in ((96, 32), (4, 8), (256, 128)):
        a, b = randn(g, n, ca).cuda(), randn(g, n, cb).cuda()
        out = spf.rows_concat(a, b)
        assert out.shape == (n, ca + cb) and same(out, torch.cat([a, b], 1))
        c = randn(g, n, ca).cuda()
        assert same(spf.rows_add(a, c), a + c)


# ---------------------------------------------------------------- the executor
def _randomise_batchnorm(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            c = m.running_mean.shape[0]
            m.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(c, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(c, generator=g) * 0.2)


def _build(kind, seed=0):
    """(cfg, model on the GPU with randomised BatchNorm, its SPVCNN)."""
    from fusiontransformer_amd.config import lidar_cfg
    from fusiontransformer_amd.models.build import build_model
    cfg = lidar_cfg() if kind == "lidar" else small_cfg(kind)
    torch.manual_seed(seed)
    model = build_model(cfg)[0]
    _randomise_batchnorm(model, seed + 100)
    model = model.cuda()
    return cfg, model, _spvcnn(model, kind)


def _spvcnn(model, kind):
    return model.backbone if kind == "lidar" else (model.lidar_backbone.backbone if kind == "late" else model.lidar_backbone)


def _forward(model, batch, overlap=True):
    model.overlap_branches = overlap
    with torch.no_grad():
        out = model(product_inputs(batch))
    torch.cuda.synchronize()
    return out


def _assert_native_ran(net):
    from fusiontransformer_amd.native_eval import NativeEval
    assert isinstance(net._native, NativeEval) and net._native.arenas, "the executor did not run"


def _same_outputs(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert same(a[k], b[k]), (what, k, (a[k] - b[k]).abs().max().item())


@pytest.fixture(scope="module")
def batches():
    from fusiontransformer_amd.data.synth import make_batch
    return {"small": make_batch([0, 1], max_points=2500), "frames": make_batch([0, 1])}


@pytest.mark.parametrize("size", ["small", "frames"])
@pytest.mark.parametrize("kind", ["lidar", "middle", "early", "late"])
def test_native_logits_equal_the_python_path(kind, size, batches):
    cfg, model, net = _build(kind)
    model.eval()
    batch = batches[size]
    if size == "frames":
        assert batch["coords"].shape[0] > 32000
    assert cfg.MODEL.DUAL_HEAD or kind == "lidar"
    overlaps = (True,) if kind == "lidar" else (True, False)      # the two branches on two streams, and issued serially
    off = {o: _forward(model, batch, o) for o in overlaps}
    assert net._native is None
    net.set_native_eval(True)
    for o in overlaps:
        on = _forward(model, batch, o)
        _assert_native_ran(net)
        _same_outputs(on, off[o], (kind, size, "overlap" if o else "serial"))
        if kind != "lidar":
            assert "lidar_seg_logit2" in on
    li = net.last_index
    net.set_native_eval(False)
    again = _forward(model, batch, overlaps[0])
    _same_outputs(again, off[overlaps[0]], (kind, size, "switched off again"))
    for lvl in ("x0", "x1", "x2", "x3", "x4"):
        assert torch.equal(li[lvl].C, net.last_index[lvl].C), lvl


def test_native_eval_yields_the_fusion_tokens():
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.models._fusion_common import _Lazy
    for kind, need in (("middle", "need_middle"), ("early", "need_early"), ("late", None)):
        _, model, net = _build(kind)
        model.eval()
        net.set_native_eval(True)
        pin = product_inputs(make_batch([3], max_points=1500))
        lazy = _Lazy()
        with torch.no_grad():
            model.image_backbone(img=pin["img"], img_indices=pin["img_indices"], on_middle=lazy.set)
            steps = model.lidar_backbone.forward_steps(pin["lidar"], lazy) if kind != "late" else model.lidar_backbone.forward_steps(pin["lidar"])
            tokens = []
            while True:
                try:
                    tokens.append(next(steps))
                except StopIteration:
                    break
        toks = [t for t in tokens if t != "sync"]
        assert toks[0] == "voxelized" and toks[-1] == "up4" and ("need_early" in toks) == (need == "need_early") and ("need_middle" in toks) == (need == "need_middle")
        if need == "need_early":
            assert toks.index("need_early") < toks.index("stem")
        if need == "need_middle":
            assert toks.index("stem") < toks.index("need_middle") < toks.index("stage4")


def test_arena_grows_and_is_reused_across_alternating_batches():
    from fusiontransformer_amd.data.synth import make_batch
    a, b = make_batch([5], max_points=1200), make_batch([6, 7], max_points=4000)
    cfg, model, net = _build("middle", seed=3)
    model.eval()
    net.set_native_eval(True)
    outs = [_forward(model, x) for x in (a, b, a, b)]
    sizes = [buf.shape[0] for buf in net._native.arenas.values()]
    assert len(sizes) == 1, "one arena per (device, stream)"
    for x, idx in ((a, (0, 2)), (b, (1, 3))):
        _, fresh, fnet = _build("middle", seed=3)
        fresh.eval()
        fnet.set_native_eval(True)
        ref = _forward(fresh, x)
        for i in idx:
            _same_outputs(outs[i], ref, ("alternating", i))
        fnet.set_native_eval(False)
        _same_outputs(_forward(fresh, x), ref, "python path of the fresh model")


def test_tiny_cloud_with_one_voxel_on_the_deepest_levels():
    """A few points inside one 16-voxel cell: levels 8 and 16 hold a single voxel."""
    from fusiontransformer_amd.sparse import SparseTensor
    rng = np.random.default_rng(0)
    pts = np.unique(rng.integers(0, 8, size=(40, 3)), axis=0)
    coords = np.concatenate([pts, np.zeros((pts.shape[0], 1), dtype=pts.dtype)], 1).astype(np.int32)
    feats = rng.standard_normal((coords.shape[0], 4)).astype(np.float32)
    _, model, net = _build("lidar", seed=4)
    model.eval()

    def run():
        with torch.no_grad():
            return model({"lidar": SparseTensor(torch.from_numpy(feats).cuda(), torch.from_numpy(coords).cuda())})
    off = run()
    net.set_native_eval(True)
    on = run()
    _assert_native_ran(net)
    assert net.last_index["x4"].C.shape[0] == 1 and net.last_index["x3"].C.shape[0] == 1
    _same_outputs(on, off, "tiny cloud")


def empty_map_program(spf):
    """A two-op program of its own for the C entry point: a 3x3x3 Conv3d -> BatchNorm over a map with n_pairs == 0 (the empty route), then
    the devoxelize onto the points.  Returns (args of ftx_spvcnn_eval up to the arena, arena bytes, output shape, the per-op Python path's
    result, the tensors the tables point at)."""
    from fusiontransformer_amd import native_eval as ne
    g = gen(21)
    n, npts, ca, co, kvol = 24, 60, 32, 32, 27
    neg = torch.full((kvol, n), -1, dtype=torch.int32, device="cuda")
    koff = torch.zeros(kvol + 1, dtype=torch.int32, device="cuda")
    w = randn(g, kvol, ca, co).cuda()
    gam, bet, rm, rv = (t.cuda() for t in (torch.rand(co, generator=g) + 0.5, randn(g, co), randn(g, co), torch.rand(co, generator=g) + 0.1))
    feats = randn(g, n, ca).cuda()
    idx = torch.randint(-1, n, (npts, 8), generator=g).int().cuda()
    wts = torch.rand(npts, 8, generator=g).float().cuda()
    layers = np.zeros(1, dtype=ne.LAYER)
    l = layers[0]
    l["weight"], l["gamma"], l["beta"], l["mean"], l["var"] = (t.data_ptr() for t in (w, gam, bet, rm, rv))
    l["ca"], l["co"], l["kvol"], l["stride"], l["eps"], l["kind"] = ca, co, kvol, 1, EPS, ne.LAYER_CONV_BN
    ops = np.array([(ne.OP_CONV_BN, 0, 0, 0, ne.SLOT_INPUT, -1, 2, 1, 0, co, 0, 0), (ne.OP_DEVOXELIZE, 0, -1, 0, 2, -1, ne.SLOT_OUTPUT, 0, ne.POINTS, co, 0, 0)],
                   dtype=ne.OP)
    rows = np.array([n, 0, 0, 0, 0, npts], dtype=np.int64)
    maps = np.zeros(1, dtype=ne.MAP)
    m = maps[0]
    m["nbr"], m["pos"], m["pos_t"], m["koff"] = neg.data_ptr(), neg.data_ptr(), neg.data_ptr(), koff.data_ptr()
    m["n_in"], m["n_out"], m["kvol"] = n, n, kvol
    pvs = np.zeros(1, dtype=ne.PV)
    pvs[0]["devox_idx"], pvs[0]["devox_weights"], pvs[0]["n_vox"], pvs[0]["level"] = idx.data_ptr(), wts.data_ptr(), n, 0
    routes = np.array([ne.ROUTES[spf._EMPTY], 0], dtype=np.int32)
    need = ne.arena_bytes(layers, ops, rows, maps, pvs, routes)
    p = ne._ptr
    args = (p(layers), 1, p(ops), 2, p(rows), p(maps), 1, p(pvs), 1, p(routes), feats.data_ptr(), 0, 0, None, None)
    with torch.no_grad():
        y = spf.batch_norm(torch.zeros((n, co), device="cuda"), gam, bet, rm, rv, False, 0.1, EPS, relu=True)
        ref = spf.spdevoxelize(y, idx, wts)
    keep = (neg, koff, w, gam, bet, rm, rv, feats, idx, wts, layers, ops, rows, maps, pvs, routes)
    return args, need, (npts, co), ref, keep


def test_executor_runs_an_empty_map(env):
    """The C entry point on a two-op program of its own (empty_map_program) -- against the per-op Python path."""
    spf, L = env
    args, need, shape, ref, keep = empty_map_program(spf)
    arena = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.empty(shape, dtype=torch.float32, device="cuda")
    assert L.ftx_spvcnn_eval(*args, arena.data_ptr(), need - 256, out.data_ptr(), spf.stream()) == -3
    spf.check(L.ftx_spvcnn_eval(*args, arena.data_ptr(), need, out.data_ptr(), spf.stream()), "ftx_spvcnn_eval")
    assert same(out, ref)


@pytest.mark.parametrize("kind", ["middle", "early", "late"])
def test_native_logits_match_the_cpu_oracle(kind):
    """The native path directly against the oracle, the project's eval gate."""
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.models.build import build_model
    from oracle import ft_oracle as O
    cfg = small_cfg(kind)
    torch.manual_seed(0)
    oracle = O.build_model(dict(cfg.MODEL))
    model = build_model(cfg)[0]
    model.load_state_dict(oracle.state_dict())
    model = model.cuda()
    net = _spvcnn(model, kind).set_native_eval(True)
    batch = make_batch([0, 1], max_points=2500)
    oracle.eval(); model.eval()
    with torch.no_grad():
        ref = oracle(oracle_inputs(batch))
        out = model(product_inputs(batch))
    _assert_native_ran(net)
    for k in ref:
        err = (out[k].cpu() - ref[k]).abs().max().item()
        print(f"native vs oracle {kind} {k}: max |diff| = {err:.3g}")
        assert err <= TOL, (kind, k, err)
    lo = (oracle.lidar_backbone.backbone if kind == "late" else oracle.lidar_backbone).last_index
    for lvl in ("x0", "x1", "x2", "x3", "x4"):
        assert np.array_equal(net.last_index[lvl].C.cpu().numpy(), lo[lvl].C), lvl


@pytest.mark.parametrize("mode,kind", [("train", "middle"), ("train", "lidar"), ("eval_with_grad", "lidar")])
def test_switch_on_with_training_or_gradients_runs_the_existing_path(mode, kind, batches):
    """model.train(), or eval with gradients enabled: the executor must not run; logits and every gradient equal the switch-off run.
    (Eval with gradients is run on the LiDAR-only model: the image branch's fused sample-down has no eval-mode backward.)"""
    from fusiontransformer_amd.trainer import fusion_losses
    cfg, model, net = _build(kind, seed=5)
    pin = product_inputs(batches["small"])
    cw = torch.tensor(cfg.TRAIN.CLASS_WEIGHTS).cuda()

    def run(on):
        net.set_native_eval(on)
        model.train() if mode == "train" else model.eval()
        state = {k: v.clone() for k, v in model.state_dict().items()}
        model.zero_grad(set_to_none=True)
        torch.manual_seed(11)
        torch.cuda.manual_seed(11)
        out = model(pin)
        if kind == "lidar":
            loss = spf_seg_loss(out["lidar_seg_logit"], pin["seg_label"], cw)
        else:
            l2, l3 = fusion_losses(out, pin["seg_label"], cw, 0.1, True)
            loss = l2 + l3
        loss.backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        model.load_state_dict(state)       # running statistics back to where they were
        return {k: v.detach().clone() for k, v in out.items()}, grads
    out_off, g_off = run(False)
    out_on, g_on = run(True)
    assert net._native is None, "the executor must not be built, let alone run"
    _same_outputs(out_on, out_off, mode)
    assert g_on.keys() == g_off.keys() and len(g_on) > 50      # at least every Conv3d kernel
    for name in g_off:
        assert same(g_on[name], g_off[name]), (mode, kind, name)


def spf_seg_loss(logit, label, cw):
    from fusiontransformer_amd import functional as spf
    return spf.seg_loss(logit, label, cw)


def test_validate_batch_gives_the_same_confusion_matrices(batches):
    from fusiontransformer_amd.evaluate import Evaluator, validate_batch
    cfg, model, net = _build("middle", seed=6)
    model.eval()
    batch = batches["small"]
    frame = batch["coords"][:, 3]
    rng = np.random.default_rng(1)
    per = [int((frame == b).sum()) for b in range(2)]
    data = {"inverse_map": [rng.integers(0, n, size=n) for n in per], "orig_seg_label": [rng.integers(0, 20, size=n) for n in per],
            "sparse_orig_points_idx": [np.ones(n, dtype=bool) for n in per]}
    mats = []
    for on in (False, True):
        net.set_native_eval(on)
        preds = _forward(model, batch)
        ev = [Evaluator([str(i) for i in range(20)]) for _ in range(3)]
        res = validate_batch(preds, data, list(range(20)), ev[0], ev[1], ev[2], want_preds=True)
        assert int(res["bad_index_flag"].item()) == 0
        mats.append([e.mat.clone() for e in ev] + [res["pred_3d"], res["pred_2d"], res["pred_ensemble"]])
    _assert_native_ran(net)
    assert 0 < mats[0][0].sum().item() <= sum(per)       # every original point with a labelled class is counted once
    for a, b in zip(*mats):
        assert torch.equal(a, b)
