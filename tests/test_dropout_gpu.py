"""The library's Dropout on the GPU (include/ftx.h: ftx_dropout / ftx_dropout_mask, FTX_SPVCNN_OP_DROPOUT, SPVCNN.set_native_dropout).

The kernels are held to the numpy restatement of the random stream (tests/dropout_ref.py) bit for bit -- mask, forward, and the same
call on a second tensor as the backward -- on both of their paths, between guard bands; the wrappers to the autograd rule
dx = dy * mask * scale; the model with the switch on to the per-op path with the switch on (bit for bit), to itself after its
dropout_state is restored, and to the float64 oracle given the masks the step really used."""
import numpy as np
import pytest
import torch

from tests import dropout_ref as R
from tests import guard as G
from tests.helpers import product_inputs
from tests.nolaunch import NoLaunch

pytestmark = pytest.mark.gpu
U64 = (1 << 64) - 1
ELEM0 = (0, 4, 1, (1 << 34) - 8, (1 << 34) - 6)       # the last two: q crosses 2^32 inside the call, aligned and not
CALLS = (0, 1, 1 << 32, U64)
SEEDS = (0, 1, 1 << 32, U64)
PS = (0.0, 0.3, 0.5, 0.999999)
SMALL_N = (1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 4093)
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-40, -3e-42, 1.1754944e-38], dtype=np.float32)
BAND = 1024                                            # elements on either side of a buffer under test


@pytest.fixture(scope="module")
def env():
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return spf, _lib.load()


def bits(t):
    return t.contiguous().view(torch.int32)


def place(n, offset, data=None):
    """(whole, view): n float32 elements `offset` elements behind a 256-byte boundary, inside an allocation that holds the guard
    sentinel everywhere else; data None: an output, sentinel in the view too."""
    whole = torch.full((n + 2 * BAND,), G.SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    assert whole.data_ptr() % 256 == 0
    view = whole[BAND + offset:BAND + offset + n]
    if data is not None:
        view.copy_(torch.from_numpy(data))
    return whole, view


def outside_untouched(whole, view):
    start = view.storage_offset() - whole.storage_offset()
    return G.sentinel_only(whole[:start]) and G.sentinel_only(whole[start + view.numel():])


def same_values(got, want):
    """Bitwise where `want` is a number, NaN at the same places."""
    got, want = got.cpu(), want.cpu()
    nan = torch.isnan(want)
    return bool((torch.isnan(got) == nan).all()) and bool((bits(got)[~nan] == bits(want)[~nan]).all())


def planted(n, keep, seed):
    """Random data with NaN, +-Inf, -0.0 and denormals at kept and at dropped positions (where there are any)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n).astype(np.float32)
    for idx in (np.flatnonzero(keep), np.flatnonzero(~keep)):
        k = min(len(idx), len(SPECIALS))
        x[idx[:k]] = SPECIALS[:k]
    return x


def torch_rule(x, keep, p):
    """x * mask * scale in torch float32."""
    return torch.from_numpy(x) * torch.from_numpy(keep).float() * float(R.scale(np.float32(p)))


def run_case(L, spf, n, p, seed, call, elem0):
    keep = R.keep_mask(n, p, seed, call, elem0)
    st = spf.stream()
    what = (n, p, seed, call, elem0)
    # ---- the mask: at an aligned address and one byte behind it
    for off in (0, 1):
        whole = torch.full((n + 2 * BAND,), 0xA5, dtype=torch.uint8, device="cuda")
        view = whole[BAND + off:BAND + off + n]
        spf.check(L.ftx_dropout_mask(n, p, seed, call, elem0, view.data_ptr(), st), "ftx_dropout_mask")
        assert np.array_equal(view.cpu().numpy(), keep.astype(np.uint8)), (what, off)
        assert bool((whole[:BAND + off] == 0xA5).all()) and bool((whole[BAND + off + n:] == 0xA5).all()), (what, off, "mask wrote outside")
    # ---- forward, then the same call on a second tensor as the backward
    x, g = planted(n, keep, n + 1), planted(n, keep, n + 2)
    for data in (x, g):
        want = torch_rule(data, keep, p)
        assert same_values(torch.from_numpy(R.dropout(data, p, seed, call, elem0)), want), (what, "the restatement against torch's rule")
        if p == 0.0:
            finite = ~np.isnan(data)
            assert np.array_equal(want.numpy().view(np.int32)[finite], data.view(np.int32)[finite]), "p = 0 returns x bit for bit"
        for off in (0, 1):            # 16-byte aligned, and the same data 4 bytes further
            for inplace in (False, True):
                xin_whole, xin = place(n, off, data)
                out_whole, out = (xin_whole, xin) if inplace else place(n, off)
                spf.check(L.ftx_dropout(xin.data_ptr(), n, p, seed, call, elem0, out.data_ptr(), st), "ftx_dropout")
                assert same_values(out, want), (what, off, inplace)
                assert outside_untouched(out_whole, out), (what, off, inplace, "wrote outside its n elements")
                if not inplace:
                    assert bool((bits(xin) == bits(torch.from_numpy(data).cuda())).all()) and outside_untouched(xin_whole, xin), (what, "the input changed")
        # an output aligned otherwise than its input: the scalar path on an aligned input
        xin_whole, xin = place(n, 0, data)
        out_whole, out = place(n, 3)
        spf.check(L.ftx_dropout(xin.data_ptr(), n, p, seed, call, elem0, out.data_ptr(), st), "ftx_dropout")
        assert same_values(out, want) and outside_untouched(out_whole, out), (what, "input aligned, output not")


def table():
    """(n, elem0, p, seed, call): every n with every elem0; p, seed and call cycle so that each of their values meets every elem0 and
    every value of the other two (asserted below)."""
    rows = []
    for i, n in enumerate(SMALL_N):
        for e, elem0 in enumerate(ELEM0):
            k = 5 * i + e
            rows.append((n, elem0, PS[k % 4], SEEDS[(k // 4) % 4], CALLS[(e + k // 16) % 4]))
    return rows


@pytest.mark.parametrize("n", SMALL_N)
def test_kernels_reproduce_the_restatement_bit_for_bit(env, n):
    spf, L = env
    for _, elem0, p, seed, call in [r for r in table() if r[0] == n]:
        run_case(L, spf, n, p, seed, call, elem0)


def test_the_table_pairs_every_value_with_every_other():
    rows = table()
    axes = (SMALL_N, ELEM0, PS, SEEDS, CALLS)
    for a in range(5):
        for b in range(a + 1, 5):
            seen = {(r[a], r[b]) for r in rows}
            if a == 0 and b >= 2:       # 11 sizes x 5 rows each cannot meet all four values of three more axes: every value, not every pair
                assert {r[b] for r in rows} == set(axes[b])
            else:
                assert len(seen) == len(axes[a]) * len(axes[b]), (a, b, len(seen))


def test_one_sweep_of_the_capped_grid_and_five(env):
    """n just past what the capped grid covers in one sweep: the 16-byte path grid-strides once and ends in a scalar tail; the scalar path
    (the same data 4 bytes further) strides eight times."""
    spf, L = env
    n = int(L.ftx_dropout_sweep_elements()) + 5
    assert n == 2048 * 256 * 4 + 5
    run_case(L, spf, n, 0.3, 1 << 32, 1, 0)
    run_case(L, spf, n, 0.5, U64, 1 << 32, (1 << 34) - 6)


def test_bad_operands_are_refused_with_no_launch(env, monkeypatch):
    from fusiontransformer_amd import _lib
    spf, L = env
    x = torch.zeros(64, device="cuda")
    monkeypatch.setattr(_lib, "load", lambda: NoLaunch())
    ok = dict(p=0.3, seed=1, call=2, elem0=0)
    for bad_x in (x.cpu(), x.double(), x.half(), None, x.cpu().numpy()):
        with pytest.raises(ValueError):
            spf.dropout(bad_x, **ok)
    with pytest.raises(ValueError, match="contiguous"):
        spf.dropout(x[::2], inplace=True, **ok)
    for bad in (dict(p=1.0), dict(p=-1e-3), dict(p=float("nan")), dict(p="x"), dict(seed=-1), dict(seed=U64 + 1), dict(call=-1), dict(call=0.5),
                dict(elem0=U64 + 1), dict(seed=True)):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            spf.dropout(x, **kw)
        with pytest.raises(ValueError):
            spf.dropout_mask((64,), **kw)
    with pytest.raises(ValueError):
        spf.dropout_mask((4, -1), **ok)
    with pytest.raises(ValueError, match="CUDA"):
        spf.dropout_mask((4,), device="cpu", **ok)
    with pytest.raises(AssertionError, match="launched"):      # the stub is in place: a good call would have launched
        spf.dropout(x, **ok)
    monkeypatch.undo()
    # the entries themselves, on real buffers: refused, and nothing written
    whole, view = place(64, 0)
    for args in ((view.data_ptr(), 64, 1.0, 0, 0, 0, view.data_ptr()), (view.data_ptr(), -1, 0.3, 0, 0, 0, view.data_ptr()),
                 (view.data_ptr(), 32, 0.3, 0, 0, 0, view.data_ptr() + 16), (None, 64, 0.3, 0, 0, 0, view.data_ptr())):
        assert L.ftx_dropout(*args, spf.stream()) == -1
    assert L.ftx_dropout(view.data_ptr(), 0, 0.3, 0, 0, 0, view.data_ptr(), spf.stream()) == 0
    torch.cuda.synchronize()
    assert G.sentinel_only(whole)


@pytest.mark.parametrize("inplace", [False, True])
def test_autograd_node_gives_dy_times_mask_times_scale(env, inplace):
    spf, L = env
    p, seed, call, elem0 = 0.3, 0x1234567890ABCDEF, (1 << 32) + 3, 4
    g = torch.Generator().manual_seed(3)
    x = torch.randn(37, 24, generator=g).cuda().requires_grad_(True)
    dy = torch.randn(37, 24, generator=g).cuda()
    dy[0, :3] = torch.tensor([float("inf"), float("nan"), -0.0])
    h = x * 1.0 if inplace else x
    y = spf.dropout(h, p, seed, call, elem0, inplace=inplace)
    assert (y.data_ptr() == h.data_ptr()) == inplace and [n.name() for n in [y.grad_fn]] == ["_DropoutBackward"]
    y.backward(dy)
    torch.cuda.synchronize()
    keep = R.keep_mask(x.numel(), p, seed, call, elem0).reshape(37, 24)
    mask = spf.dropout_mask((37, 24), p, seed, call, elem0)
    assert mask.dtype == torch.bool and np.array_equal(mask.cpu().numpy(), keep)
    scale = float(R.scale(np.float32(p)))
    assert same_values(y.detach(), x.detach().cpu() * torch.from_numpy(keep).float() * scale)
    assert same_values(x.grad, dy.cpu() * torch.from_numpy(keep).float() * scale)
    # not in place: a view is taken as it is, and under no_grad the node is not recorded
    if not inplace:
        xt = x.detach().t()
        assert same_values(spf.dropout(xt, p, seed, call), xt.contiguous().cpu() * torch.from_numpy(R.keep_mask(xt.numel(), p, seed, call).reshape(24, 37)).float() * scale)
        assert same_values(spf.dropout(x.detach(), 0.0, seed, call), x.detach())


# ---------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def batches():
    from fusiontransformer_amd.data.synth import make_batch
    return {"a": make_batch([0, 1], max_points=2500), "b": make_batch([2], max_points=1700)}


def _both_on(kind, seed, drop_seed):
    """tests/test_native_train_gpu._pair: the model runs the executor with the Dropout op, the twin the per-op path with functional.dropout."""
    from tests.test_native_train_gpu import _pair
    cfg, model, twin, net, net_twin = _pair(kind, seed=seed)
    net.set_native_train(True).set_native_dropout(True, seed=drop_seed)
    net_twin.set_native_dropout(True, seed=drop_seed)
    assert net.dropout_state() == net_twin.dropout_state() == {"seed": drop_seed & U64, "forwards": 0}
    return cfg, model, twin, net, net_twin


def _assert_three_segments(net, preds, runs):
    from fusiontransformer_amd.native_train import NativeTrain
    from tests.test_native_train_gpu import _graph_nodes, _per_op, _segments
    assert isinstance(net._native_tr, NativeTrain) and net._native_tr.runs == runs and net._native_tr.tp.native_dropout
    names = _graph_nodes(preds["lidar_seg_logit"])
    assert _segments(names) == net._native_tr.tp.n_segments == 3
    left = _per_op(names)
    assert all(left[p] == 0 for p in ("_ConvBNTrain", "_RowsMatmul", "_SparseConv", "_Voxelize", "_Devoxelize")), left
    assert not [n for n in names if n.startswith("_DropoutBackward")], "Dropout is inside the segment"


@pytest.mark.parametrize("kind", ["lidar", "middle"])
def test_executor_with_the_dropout_op_equals_the_per_op_path(kind, batches):
    from fusiontransformer_amd.trainer import TrainStep
    from tests.test_native_eval_gpu import same
    from tests.test_native_train_gpu import _assert_same_state, _graph_nodes, _lidar_inputs, _segments, _twin_steps, _two_cell_cloud
    cfg, model, twin, net, net_twin = _both_on(kind, seed=21, drop_seed=(1 << 63) + 11)
    preds = _twin_steps(kind, cfg, model, twin, net, net_twin, [(batches["a"], None), (batches["b"], None)])
    _assert_three_segments(net, preds, 2)
    assert net.dropout_state()["forwards"] == net_twin.dropout_state()["forwards"] == 2
    twin_names = _graph_nodes(twin(product_inputs(batches["b"]))["lidar_seg_logit"])
    assert _segments(twin_names) == 0 and sum(n.startswith("_DropoutBackward") for n in twin_names) == 2
    assert net_twin.dropout_state()["forwards"] == 3
    if kind != "lidar":
        return
    # one step on a cloud whose stride-16 level holds two voxels: 2 x 256 = 512 elements at site 0
    model.load_state_dict(twin.state_dict())          # the twin's extra forward moved its running statistics ...
    net.set_dropout_state(net_twin.dropout_state())   # ... and its call counter
    step, step_twin = TrainStep(cfg, model), TrainStep(cfg, twin)
    tiny = _two_cell_cloud()
    preds, preds_twin = step(_lidar_inputs(tiny)), step_twin(_lidar_inputs(tiny))
    torch.cuda.synchronize()
    assert net.last_index["x4"].C.shape[0] == 2 and net.last_dropout_masks()["y1"].numel() == 512
    assert same(preds["lidar_seg_logit"], preds_twin["lidar_seg_logit"]) and same(step.last["loss_3d"], step_twin.last["loss_3d"])
    assert _assert_same_state(model, twin, "two voxels") > 150
    assert all(torch.equal(a, b) for a, b in zip(net.last_dropout_masks().values(), net_twin.last_dropout_masks().values()))


def _fwd_bwd(spf, cfg, model, pin):
    from tests.test_native_train_gpu import _manual_step
    out, loss = _manual_step(spf, cfg, model, pin)
    loss.backward()
    torch.cuda.synchronize()
    return out["lidar_seg_logit"].detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters()}


def test_restoring_the_dropout_state_reproduces_a_step(env, batches):
    spf, L = env
    from tests.test_native_eval_gpu import same
    cfg, model, twin, net, net_twin = _both_on("lidar", seed=22, drop_seed=5)
    b = batches["b"]
    weights = {k: v.clone() for k, v in model.state_dict().items()}
    state = net.dropout_state()
    logits0, grads0 = _fwd_bwd(spf, cfg, model, product_inputs(b))
    masks0 = net.last_dropout_masks()
    assert net.dropout_state() == {"seed": 5, "forwards": 1}
    # the masks are those of the restatement for (seed, 2 * forwards + site), over the rows of y1 and y3
    for site, (name, m) in enumerate(masks0.items()):
        assert m.dtype == torch.bool and m.shape[1] == (256, 128)[site] and m.shape[0] == net.last_index[("x4", "x2")[site]].C.shape[0]
        assert np.array_equal(m.cpu().numpy().reshape(-1), R.keep_mask(m.numel(), 0.3, 5, site)), name
    logits1, grads1 = _fwd_bwd(spf, cfg, model, product_inputs(b))
    masks1 = net.last_dropout_masks()
    assert net.dropout_state()["forwards"] == 2
    for name in masks0:
        assert masks0[name].shape == masks1[name].shape and not torch.equal(masks0[name], masks1[name]), "step 0 and step 1 draw different masks"
    k = min(masks0["y1"].numel(), masks0["y3"].numel())
    assert not torch.equal(masks0["y1"].reshape(-1)[:k], masks0["y3"].reshape(-1)[:k]), "sites 0 and 1 draw different masks"
    assert not same(logits0, logits1)
    model.load_state_dict(weights)
    net.set_dropout_state(state)
    logits2, grads2 = _fwd_bwd(spf, cfg, model, product_inputs(b))
    assert same(logits0, logits2) and all(same(grads0[n], grads2[n]) for n in grads0) and len(grads0) > 150
    assert all(torch.equal(masks0[n], m) for n, m in net.last_dropout_masks().items())


def test_step_with_both_switches_on_meets_the_train_step_gates_with_its_own_masks(batches):
    """The gates of tests/test_native_train_gpu.py::test_lidarseg_step_with_the_switch_on_meets_the_train_step_gates, the float64 oracle
    given the masks the step drew (last_dropout_masks).  The product multiplies by float32(1 / 0.7) where the oracle divides by 0.7:
    a relative 2^-25 at most, far inside the gates."""
    import torch.nn.functional as F
    from fusiontransformer_amd.config import lidar_cfg
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    from oracle import ft_oracle as O
    from tests.test_fullsize_train_gpu import _snapshot
    cfg = lidar_cfg()
    torch.manual_seed(9)
    model = build_model(cfg)[0].cuda().train()
    net = model.backbone.set_native_train(True).set_native_dropout(True, seed=2024)
    step = TrainStep(cfg, model)
    b = batches["a"]
    pre = _snapshot(model)
    preds = step(product_inputs(b))
    torch.cuda.synchronize()
    _assert_three_segments(net, preds, 1)
    masks = {k: v.cpu().double() for k, v in net.last_dropout_masks().items()}
    rates = {k: float(v.mean()) for k, v in masks.items()}
    assert all(0.6 < r < 0.8 for r in rates.values()), rates
    oracle = O.Net3DSegLate(20, False, dict(cfg.MODEL)).double().train()
    oracle.load_state_dict({k: (v.double() if v.dtype.is_floating_point else v) for k, v in pre.items()})
    oracle.backbone.dropout_masks = masks
    ref = oracle(O.SparseTensor(torch.from_numpy(b["feats"]).double(), b["coords"]))
    cw = torch.tensor(cfg.TRAIN.CLASS_WEIGHTS).double()
    F.cross_entropy(ref["lidar_seg_logit"], torch.from_numpy(b["seg_label"]).long(), weight=cw).backward()
    err = (preds["lidar_seg_logit"].detach().cpu().double() - ref["lidar_seg_logit"].detach()).abs().max().item()
    p64, gm = dict(oracle.named_parameters()), dict(model.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in p64.values() if p.grad is not None)
    rows = []
    for name, p in p64.items():
        assert p.grad is not None and gm[name].grad is not None, name
        floor = 1e-4 * gmax * p.numel() ** 0.5       # gradients that are 0 in exact arithmetic (Linear biases in front of a BatchNorm)
        rows.append(((gm[name].grad.cpu().double() - p.grad).norm().item() / max(p.grad.norm().item(), floor), name))
    rows.sort(reverse=True)
    print("native dropout vs float64 oracle: logits %.3g (gate 1e-3), worst gradient %.3g %s (gate 5e-2), keep rates %s" % (err, rows[0][0], rows[0][1], rates))
    assert err <= 1e-3, err
    assert rows[0][0] < 5e-2, rows[:5]


def test_guards_of_the_switch(env, batches):
    spf, L = env
    from tests.test_fullsize_train_gpu import _masks
    from tests.test_native_eval_gpu import same
    from tests.test_native_train_gpu import _graph_nodes, _pair, _segments, _twin_steps
    cfg, model, twin, net, net_twin = _pair("lidar", seed=23)
    net.set_native_dropout(True, seed=1)
    b = batches["b"]
    # injected masks and the switch: one or the other, on the per-op path and through the executor, before anything is counted
    masks = {k: v.float().cuda() for k, v in _masks(b["coords"], 3).items()}
    for native_train in (False, True):
        net.set_native_train(native_train)
        net.dropout_masks = masks
        with pytest.raises(ValueError, match="one or the other"):
            model(product_inputs(b))
        net.dropout_masks = None
    assert net.dropout_state()["forwards"] == 0
    # eval mode, and training mode without gradients (torch's Dropout, torch's stream): the outputs of the switch being off
    model.load_state_dict(twin.state_dict())
    for mode in ("eval", "no_grad"):
        outs = []
        for m in (model, twin):
            m.train(mode != "eval")
            torch.manual_seed(40)
            with torch.no_grad():
                outs.append(m(product_inputs(b))["lidar_seg_logit"])
        assert same(outs[0], outs[1]), mode
        model.load_state_dict(twin.state_dict())
    assert net.dropout_state()["forwards"] == 0 and (not net._native_tr or net._native_tr.runs == 0)
    # off again: five segments and torch's Dropout, bit for bit the twin that never had the switch on
    model.train(), twin.train()
    net.set_native_dropout(False)
    assert net._native_tr is None and net.lidar_native_train is True
    preds = _twin_steps("lidar", cfg, model, twin, net, net_twin, [(b, None)])
    assert _segments(_graph_nodes(preds["lidar_seg_logit"])) == 5 and not net._native_tr.tp.native_dropout
    assert net.dropout_state()["forwards"] == 0
