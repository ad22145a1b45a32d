"""The native training executor of the SPVCNN LiDAR branch on the GPU (include/ftx.h: ftx_spvcnn_train_fwd / _bwd,
SPVCNN.set_native_train): its row kernel against torch, and a model with the switch on against its twin with the switch off -- two
models from one seed, the same steps, compared on bit patterns: logits, losses, every gradient, every parameter after Adam, every
BatchNorm buffer."""
import numpy as np
import pytest
import torch

from tests.helpers import product_inputs, small_cfg
from tests.norm_ref import gen, randn
from tests.test_fullsize_train_gpu import _masks, _snapshot
from tests.test_native_eval_gpu import _randomise_batchnorm, _spvcnn, same

pytestmark = pytest.mark.gpu
PER_OP_NODES = ("_ConvBNTrain", "_BatchNormTrain", "_RowsLinear", "_RowsMatmul", "_SparseConv", "_Voxelize", "_Devoxelize")


@pytest.fixture(scope="module")
def spf():
    from fusiontransformer_amd import functional
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return functional


@pytest.fixture(scope="module")
def batches():
    from fusiontransformer_amd.data.synth import make_batch
    return {"a": make_batch([0, 1], max_points=2500), "b": make_batch([2], max_points=1700)}


# ---------------------------------------------------------------- the row kernel
@pytest.mark.parametrize("n", [0, 1, 7, 4099])
def test_rows_split_equals_torch_split_and_inverts_rows_concat(spf, n):
    g = gen(n + 5)
    for ca, cb in ((32, 32), (96, 32), (256, 128)):
        x = randn(g, n, ca + cb).cuda()
        a, b = spf.rows_split(x, ca)
        ta, tb = torch.split(x, [ca, cb], 1)
        assert a.shape == (n, ca) and b.shape == (n, cb) and a.is_contiguous() and b.is_contiguous()
        assert same(a, ta.contiguous()) and same(b, tb.contiguous())
        p, q = randn(g, n, ca).cuda(), randn(g, n, cb).cuda()
        a2, b2 = spf.rows_split(spf.rows_concat(p, q), ca)
        assert same(a2, p) and same(b2, q)


# ---------------------------------------------------------------- twins
def _pair(kind, seed=0, bn_seed=None):
    """(cfg, model, twin, their SPVCNNs): two models from one seed with randomised BatchNorm, on the GPU in training mode."""
    from fusiontransformer_amd.config import lidar_cfg
    from fusiontransformer_amd.models.build import build_model
    cfg = lidar_cfg() if kind == "lidar" else small_cfg(kind)
    torch.manual_seed(seed)
    model, twin = build_model(cfg)[0], build_model(cfg)[0]
    _randomise_batchnorm(model, seed + 100 if bn_seed is None else bn_seed)
    twin.load_state_dict(model.state_dict())
    model, twin = model.cuda().train(), twin.cuda().train()
    return cfg, model, twin, _spvcnn(model, kind), _spvcnn(twin, kind)


def _graph_nodes(t):
    """Names of the autograd nodes under tensor t."""
    seen, todo, names = set(), [t.grad_fn], []
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(f.name())
        todo += [g for g, _ in f.next_functions]
    return names


def _per_op(names):
    """{per-op node type: how many} of the graph."""
    return {p: sum(n.startswith(p + "Backward") for n in names) for p in PER_OP_NODES}


def _spvcnn_nodes(net):
    """{per-op node type: how many} the per-op path makes for the SPVCNN itself, counted from its program: the heads and the fusion
    transform, which are not the executor's, make _RowsLinear / _BatchNormTrain nodes of their own."""
    from fusiontransformer_amd import native_eval as ne
    P = ne.emit_program(net)
    count = dict.fromkeys(PER_OP_NODES, 0)
    for op in P.ops:
        if op[0] == ne.OP_CONV_BN and op[3] >= 0:
            count["_ConvBNTrain"] += 1
        elif op[0] == ne.OP_CONV_BN:
            count["_RowsMatmul"] += 1
            count["_BatchNormTrain"] += 1
        elif op[0] == ne.OP_LINEAR_BN:
            count["_RowsLinear"] += 1
            count["_BatchNormTrain"] += 1
        elif op[0] == ne.OP_VOXELIZE:
            count["_Voxelize"] += 1
        elif op[0] == ne.OP_DEVOXELIZE:
            count["_Devoxelize"] += 1
    return count


def _segments(names):
    return sum(n.startswith("_SegmentBackward") for n in names)


def _assert_same_state(model, twin, what):
    gt = dict(twin.named_parameters())
    n_grads = 0
    for n, p in model.named_parameters():
        assert (p.grad is None) == (gt[n].grad is None), (what, n)
        if p.grad is not None:
            assert same(p.grad, gt[n].grad), (what, "grad", n, (p.grad - gt[n].grad).abs().max().item())
            n_grads += 1
        assert same(p.detach(), gt[n].detach()), (what, "parameter", n)
    bt = dict(twin.named_buffers())
    for n, b in model.named_buffers():
        assert torch.equal(b, bt[n]) and (not b.dtype.is_floating_point or same(b, bt[n])), (what, "buffer", n)
    return n_grads


def _twin_steps(kind, cfg, model, twin, net, net_twin, plan, overlap=True, prefetch=False):
    """The steps of `plan` [(batch, masks or None)] through TrainStep on both models (Adam between the steps); everything they leave
    must agree bit for bit.  Returns the last predictions of the model."""
    from fusiontransformer_amd.trainer import TrainStep
    step, step_twin = TrainStep(cfg, model), TrainStep(cfg, twin)
    model.overlap_branches = twin.overlap_branches = overlap
    nxt = nxt_twin = None
    preds = None
    for s, (b, masks) in enumerate(plan):
        pin = nxt if nxt is not None else product_inputs(b)
        pin_twin = nxt_twin if nxt_twin is not None else product_inputs(b)
        nxt = nxt_twin = None
        if prefetch and s + 1 < len(plan):
            nxt, nxt_twin = product_inputs(plan[s + 1][0]), product_inputs(plan[s + 1][0])
        net.dropout_masks = net_twin.dropout_masks = None if masks is None else {k: v.float().cuda() for k, v in masks.items()}
        torch.manual_seed(100 + s)
        preds = step(pin, next_batch=nxt)
        torch.manual_seed(100 + s)
        preds_twin = step_twin(pin_twin, next_batch=nxt_twin)
        torch.cuda.synchronize()
        what = (kind, "step", s)
        assert preds.keys() == preds_twin.keys()
        for k in preds:
            assert same(preds[k], preds_twin[k]), (what, k, (preds[k] - preds_twin[k]).abs().max().item())
        assert step.last.keys() == step_twin.last.keys()
        for k in step.last:
            assert same(step.last[k], step_twin.last[k]), (what, k)
        n_grads = _assert_same_state(model, twin, what)
        assert n_grads > 150
    net.dropout_masks = net_twin.dropout_masks = None
    return preds


def _assert_executor_ran(net, preds, runs, twin_names=None):
    """The graph under the logits holds one node per segment and none of the SPVCNN's per-op nodes (`twin_names`: the twin's graph,
    which holds them all; what is left in both is the heads' and the fusion transform's)."""
    from fusiontransformer_amd.native_train import NativeTrain
    assert isinstance(net._native_tr, NativeTrain) and net._native_tr.runs == runs, "the training executor did not run"
    names = _graph_nodes(preds["lidar_seg_logit"])
    assert _segments(names) == net._native_tr.tp.n_segments == 5
    left = _per_op(names)
    assert all(left[p] == 0 for p in ("_ConvBNTrain", "_RowsMatmul", "_SparseConv", "_Voxelize", "_Devoxelize")), left
    if twin_names is not None:
        own, both = _spvcnn_nodes(net), _per_op(twin_names)
        assert own["_ConvBNTrain"] > 40 and own["_Voxelize"] == 3 and own["_Devoxelize"] == 4
        assert all(left[p] == both[p] - own[p] for p in PER_OP_NODES), (left, both, own)


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("kind,overlap", [("lidar", True), ("middle", True), ("middle", False), ("early", True), ("late", True)])
def test_training_steps_equal_the_twin_with_the_switch_off(kind, overlap, batches):
    """Two consecutive steps on two alternating batches of different size with torch's Dropout (seeded), a third with injected masks;
    then the switch goes off again and a fourth step runs the per-op path."""
    cfg, model, twin, net, net_twin = _pair(kind, seed=3)
    net.set_native_train(True)
    assert net_twin.lidar_native_train is False
    a, b = batches["a"], batches["b"]
    assert a["coords"].shape[0] != b["coords"].shape[0]
    preds = _twin_steps(kind, cfg, model, twin, net, net_twin, [(a, None), (b, None), (a, _masks(a["coords"], 7))], overlap=overlap)
    twin_names = _graph_nodes(twin(product_inputs(b))["lidar_seg_logit"])
    assert _segments(twin_names) == 0
    _assert_executor_ran(net, preds, 3, twin_names)
    if kind == "lidar":
        assert sum(_per_op(_graph_nodes(preds["lidar_seg_logit"])).values()) == 1, "the head's Linear alone"
    net.set_native_train(False)
    model.load_state_dict(twin.state_dict())          # the twin's extra forward moved its running statistics
    preds = _twin_steps(kind, cfg, model, twin, net, net_twin, [(b, None)], overlap=overlap)
    names = _graph_nodes(preds["lidar_seg_logit"])
    assert _per_op(names) == _per_op(twin_names) and _segments(names) == 0 and net._native_tr is None


def _two_cell_cloud(seed=0):
    """A few dozen points spread over exactly two cells of the coarsest level (stride 16)."""
    rng = np.random.default_rng(seed)
    pts = np.unique(rng.integers(0, 8, size=(40, 3)), axis=0)
    pts = np.concatenate([pts[: len(pts) // 2], pts[len(pts) // 2:] + 16], 0)
    coords = np.concatenate([pts, np.zeros((pts.shape[0], 1), dtype=pts.dtype)], 1).astype(np.int32)
    return {"feats": rng.standard_normal((coords.shape[0], 4)).astype(np.float32), "coords": coords,
            "seg_label": rng.integers(1, 20, size=coords.shape[0]).astype(np.int64)}


def _lidar_inputs(b):
    from fusiontransformer_amd.sparse import SparseTensor
    return {"lidar": SparseTensor(torch.from_numpy(b["feats"]).cuda(), torch.from_numpy(b["coords"]).int().cuda()),
            "seg_label": torch.from_numpy(b["seg_label"]).cuda()}


def test_two_voxels_on_the_deepest_level_alternating_with_a_larger_batch(batches):
    """Levels 8 and 16 hold two voxels (one would put 0/0 into the unbiased running variance of both paths): tiny and empty kernel
    maps, one-block BatchNorm hand-overs in both directions; the larger batch in between sizes another arena."""
    from fusiontransformer_amd.trainer import TrainStep
    cfg, model, twin, net, net_twin = _pair("lidar", seed=4)
    net.set_native_train(True)
    step, step_twin = TrainStep(cfg, model), TrainStep(cfg, twin)
    tiny, big = _two_cell_cloud(), batches["a"]
    sizes = []
    for s, b in enumerate((tiny, big, tiny)):
        torch.manual_seed(50 + s)
        preds = step(_lidar_inputs(b))
        torch.manual_seed(50 + s)
        preds_twin = step_twin(_lidar_inputs(b))
        torch.cuda.synchronize()
        if b is tiny:
            assert net.last_index["x4"].C.shape[0] == 2 and net.last_index["x3"].C.shape[0] == 2
        assert same(preds["lidar_seg_logit"], preds_twin["lidar_seg_logit"]), s
        assert same(step.last["loss_3d"], step_twin.last["loss_3d"]), s
        _assert_same_state(model, twin, ("two voxels", s))
        sizes.append(net._native_tr.last_arena_bytes)
    _assert_executor_ran(net, preds, 3)
    assert sizes[0] == sizes[2] < sizes[1]


# ---------------------------------------------------------------- composition with the other switches
@pytest.mark.parametrize("what", ["native_index", "prefetch", "bf16"])
def test_switch_composes_with_the_other_switches(what, batches):
    kind = "middle" if what == "bf16" else "lidar"
    cfg, model, twin, net, net_twin = _pair(kind, seed=5)
    for n in (net, net_twin):          # the same configuration on both, the training switch on one
        if what == "native_index":
            n.set_native_index(True)
        if what == "bf16":
            n.set_bf16(True)
    net.set_native_train(True)
    plan = [(batches["b"], None), (batches["a"], None)] if what == "prefetch" else [(batches["b"], None)]
    preds = _twin_steps(kind, cfg, model, twin, net, net_twin, plan, prefetch=what == "prefetch")
    _assert_executor_ran(net, preds, len(plan))
    if what == "bf16":
        assert all(int(r["bf16"]) == 1 for r in net._native_tr.layers)


def test_native_eval_in_bf16_mode_equals_the_python_bf16_path(batches):
    """The eval executor with the bf16-operand kernels (a gap its own tests left)."""
    from fusiontransformer_amd.native_eval import NativeEval
    for kind in ("lidar", "middle"):
        _, model, _, net, _ = _pair(kind, seed=6)
        model.eval()
        net.set_bf16(True)
        pin = product_inputs(batches["b"])
        with torch.no_grad():
            off = model(pin)
            net.set_native_eval(True)
            on = model(product_inputs(batches["b"]))
        torch.cuda.synchronize()
        assert isinstance(net._native, NativeEval) and net._native.arenas and all(int(r["bf16"]) == 1 for r in net._native.layers)
        for k in off:
            assert same(on[k], off[k]), (kind, k)
        net.set_bf16(False)
        with torch.no_grad():
            fp32 = model(product_inputs(batches["b"]))
        assert not torch.equal(fp32["lidar_seg_logit"], on["lidar_seg_logit"]), "the bf16 switch changed nothing"


# ---------------------------------------------------------------- whole frames
@pytest.mark.parametrize("kind", ["lidar", "middle"])
def test_one_step_on_whole_frames(kind):
    from fusiontransformer_amd.data.synth import make_batch
    b = make_batch([0, 1])
    assert b["coords"].shape[0] > 32000
    cfg, model, twin, net, net_twin = _pair(kind, seed=8)
    net.set_native_train(True)
    preds = _twin_steps(kind, cfg, model, twin, net, net_twin, [(b, None)])
    _assert_executor_ran(net, preds, 1)


# ---------------------------------------------------------------- against the float64 oracle
def test_lidarseg_step_with_the_switch_on_meets_the_train_step_gates(batches):
    """The project's train-step gates (tests/test_model_gpu.py::test_train_step_matches_oracle): logits within 1e-3, every gradient
    within 5e-2 L2-relative of the float64 oracle -- so that the two paths are not only compared with each other."""
    import torch.nn.functional as F
    from fusiontransformer_amd.config import lidar_cfg
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    from oracle import ft_oracle as O
    cfg = lidar_cfg()
    torch.manual_seed(9)
    model = build_model(cfg)[0].cuda().train()
    net = model.backbone.set_native_train(True)
    step = TrainStep(cfg, model)
    b = batches["a"]
    masks = _masks(b["coords"], 12)
    pre = _snapshot(model)
    net.dropout_masks = {k: v.float().cuda() for k, v in masks.items()}
    preds = step(product_inputs(b))
    torch.cuda.synchronize()
    _assert_executor_ran(net, preds, 1)
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
    print("native train vs float64 oracle: logits %.3g (gate 1e-3), worst gradient %.3g %s (gate 5e-2)" % (err, rows[0][0], rows[0][1]))
    assert err <= 1e-3, err
    assert rows[0][0] < 5e-2, rows[:5]


# ---------------------------------------------------------------- where the executor must not run
def _manual_step(spf, cfg, model, pin):
    cw = torch.tensor(cfg.TRAIN.CLASS_WEIGHTS).cuda()
    model.zero_grad(set_to_none=True)
    out = model(pin)
    loss = spf.seg_loss(out["lidar_seg_logit"], pin["seg_label"], cw)
    return out, loss


@pytest.mark.parametrize("mode", ["eval", "no_grad", "frozen"])
def test_switch_on_outside_its_conditions_runs_the_per_op_path(spf, mode, batches):
    cfg, model, twin, net, net_twin = _pair("lidar", seed=10)
    net.set_native_train(True)
    if mode == "eval":
        model.eval(), twin.eval()
    if mode == "frozen":
        net.stage2[1].net[1].bias.requires_grad_(False)
        net_twin.stage2[1].net[1].bias.requires_grad_(False)
    outs = []
    for m in (model, twin):
        torch.manual_seed(21)
        with torch.set_grad_enabled(mode != "no_grad"):
            out, loss = _manual_step(spf, cfg, m, product_inputs(batches["b"]))
            if mode != "no_grad":
                loss.backward()
        outs.append((out, loss))
    torch.cuda.synchronize()
    assert not net._native_tr or net._native_tr.runs == 0, "the executor ran"
    assert same(outs[0][0]["lidar_seg_logit"], outs[1][0]["lidar_seg_logit"]) and same(outs[0][1].detach(), outs[1][1].detach())
    if mode != "no_grad":
        names = _graph_nodes(outs[0][0]["lidar_seg_logit"])
        assert _segments(names) == 0
        assert mode == "eval" or _per_op(names)["_ConvBNTrain"] > 40
        # eval-mode BatchNorm gives its affine parameters no gradient: the Conv3d kernels, the point Linears and the head remain
        assert _assert_same_state(model, twin, mode) > (50 if mode == "eval" else 150)
        if mode == "frozen":
            assert net.stage2[1].net[1].bias.grad is None


def test_cpu_tensors_take_the_existing_path(batches):
    """The product path has no CPU fallback: with the switch on a CPU forward ends where it ends with the switch off."""
    cfg, model, twin, net, net_twin = _pair("lidar", seed=11)
    net.set_native_train(True)
    errors = []
    for m in (model, twin):
        with pytest.raises(Exception) as e:
            m(product_inputs(batches["b"], device="cpu"))
        errors.append((type(e.value), str(e.value)))
    assert errors[0] == errors[1] and net._native_tr is None


def test_a_second_backward_on_a_consumed_run_raises(spf, batches):
    cfg, model, _, net, _ = _pair("lidar", seed=12)
    net.set_native_train(True)
    pin = product_inputs(batches["b"])
    out, loss = _manual_step(spf, cfg, model, pin)
    loss.backward(retain_graph=True)
    first = {n: p.grad.clone() for n, p in model.named_parameters()}
    with pytest.raises(RuntimeError, match="a second backward needs a second forward"):
        loss.backward(retain_graph=True)
    out, loss = _manual_step(spf, cfg, model, pin)
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    torch.cuda.synchronize()
    assert len(first) > 150 and all(torch.isfinite(g).all() for g in first.values())
