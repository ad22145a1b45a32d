"""The single-head segmentation loss (csrc/ftx_loss.hip, ftx_seg_loss) through functional.seg_loss, against float64
F.cross_entropy autograd, and the validation loss of evaluate.validate_batch built on its forward-only form.

The gates are the project's own (tests/loss_metric_ref.py): loss |d| <= 2e-6 * max(1, |ref|); gradient per element rtol 1e-4 plus
grad_atol(max|logit|) * max|ref|; confusion matrix bit-exact.  The single-head arithmetic is the cross-entropy part of the fused
kernel those gates were measured on.  The kernel shares that kernel's launch geometry, which the sizes straddle: 256-point blocks,
at most 256 of them (reached from n = 65 281 on), a grid-stride loop whose second pass starts at n = 65 537, a 256-row finalize."""
import numpy as np
import pytest
import torch

from tests import loss_metric_ref as R
from tests.nolaunch import NoLaunch as _NoLaunch
from tests.seg_loss_ref import seg_oracle

pytestmark = pytest.mark.gpu

KEY = R.NAMES[0]


def _cfg_weights():
    from fusiontransformer_amd.config import _CLASS_WEIGHTS
    return np.array(_CLASS_WEIGHTS, dtype=np.float32)


def _logits(rng, n, c, scale=1.0, ties=0):
    return R.make_logits(rng, n, c, scale, dual=False, ties=ties)[KEY]


def _seg(x, label, cw, ignore_index=0, upstream=1.0, conf=None, grad=True):
    """One call through functional.seg_loss (+ backward): loss, gradient (None without), matrix."""
    from fusiontransformer_amd import functional as spf
    c = x.shape[1]
    t = torch.from_numpy(x).cuda().requires_grad_(grad)
    if conf is None:
        conf = torch.zeros((c, c), dtype=torch.int64, device="cuda")
    loss = spf.seg_loss(t, torch.from_numpy(np.asarray(label)).cuda(), None if cw is None else torch.from_numpy(cw).cuda(), conf=conf,
                        ignore_index=ignore_index)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    if grad:
        (upstream * loss).backward()
    return loss.item(), (t.grad.cpu().numpy() if grad else None), conf.cpu().numpy()


def _check(x, label, cw, ignore_index=0, upstream=1.0):
    got, gg, conf = _seg(x, label, cw, ignore_index, upstream)
    ref, rg = seg_oracle(x, label, cw, upstream)
    xmax = float(np.abs(x).max())
    R.assert_losses_close((got,), (ref,))
    R.assert_grads_close({KEY: gg}, {KEY: rg}, xmax)
    R.assert_confs_equal((conf,), (R.conf_ref(x, label, x.shape[1], ignore_index),))
    return R.loss_error((got,), (ref,)), R.grad_error({KEY: gg}, {KEY: rg}, xmax)


# ------------------------------------------------------------------------------------------------ sizes and class counts
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4000, 65280, 65281, 65536, 65537, 81237, 300000])
def test_seg_loss_sizes(n):
    rng = np.random.default_rng(n)
    x = _logits(rng, n, 20, 1.0, ties=min(n, 64))
    label = R.make_labels(rng, n, 20, "invalid") if n > 1 else np.array([5])      # one point: a label of non-zero weight
    _check(x, label, _cfg_weights())


@pytest.mark.parametrize("n", [5, 65537])
@pytest.mark.parametrize("c", [4, 8, 12, 16, 20, 24, 28, 32])
def test_seg_loss_every_class_count(c, n):
    rng = np.random.default_rng(100 * c + n)
    x = _logits(rng, n, c, 1.0, ties=min(n, 32))
    _check(x, R.make_labels(rng, n, c, "uniform"), R.spread_weights(rng, c))


# ------------------------------------------------------------------------------------------------ weights, labels, logits
@pytest.mark.parametrize("weights", ["none", "config", "spread"])
def test_seg_loss_weights(weights):
    rng = np.random.default_rng(7)
    n = 65537
    x = _logits(rng, n, 20, 1.0, ties=64)
    cw = {"none": None, "config": _cfg_weights(), "spread": R.spread_weights(rng, 20)}[weights]
    _check(x, R.make_labels(rng, n, 20, "uniform"), cw)


@pytest.mark.parametrize("ignore_index", [0, 3, 77])
@pytest.mark.parametrize("kind", ["uniform", "zero30", "single", "invalid"])
def test_seg_loss_label_mixes(kind, ignore_index):
    rng = np.random.default_rng(8)
    n = 65537
    x = _logits(rng, n, 20, 1.0, ties=64)
    _check(x, R.make_labels(rng, n, 20, kind), _cfg_weights(), ignore_index=ignore_index)


@pytest.mark.parametrize("scale", [1.0, 8.0, 40.0])
def test_seg_loss_logit_scales(scale, record_property):
    """N(0,1) * scale; the worst errors, as multiples of the gate, are recorded as test properties."""
    rng = np.random.default_rng(int(scale))
    n = 300000
    x = _logits(rng, n, 20, scale, ties=256)
    le, ge = _check(x, R.make_labels(rng, n, 20, "invalid"), _cfg_weights())
    record_property("loss_rel_err", le)
    record_property("grad_err_over_gate", ge)
    print("seg_loss scale %g: loss_rel_err %.3e (gate %.1e), grad_err_over_gate %.3f" % (scale, le, R.LOSS_RTOL, ge))


@pytest.mark.parametrize("labels", ["zeros_cfg_weights", "all_invalid", "valid_weighted"])
def test_seg_loss_is_nan_exactly_when_the_total_weight_is_zero(labels):
    rng = np.random.default_rng(9)
    n = 1000
    x = _logits(rng, n, 20)
    if labels == "zeros_cfg_weights":
        label, cw = R.make_labels(rng, n, 20, "zeros"), _cfg_weights()
    elif labels == "all_invalid":
        label, cw = np.full(n, -100, dtype=np.int64), None
        label[::3] = 255
    else:                      # one point of non-zero weight among zeros: finite
        label, cw = R.make_labels(rng, n, 20, "zeros"), _cfg_weights()
        label[n // 2] = 7
    ref, _ = seg_oracle(x, label, cw)
    assert np.isnan(ref) == (labels != "valid_weighted")
    got, _, conf = _seg(x, label, cw)
    R.assert_losses_close((got,), (ref,))
    assert np.isnan(got) == np.isnan(ref)
    got_fwd, _, _ = _seg(x, label, cw, grad=False)
    assert np.isnan(got_fwd) == np.isnan(ref)
    if labels == "all_invalid":
        assert not conf.any()


# ------------------------------------------------------------------------------------------------ matrix, upstream, determinism
def test_confusion_matrix_carries_and_accumulates():
    """Cells pre-filled with 2^40 and 2^32 - 1 (the 64-bit add must carry out of the low word), accumulated over two calls."""
    rng = np.random.default_rng(10)
    n = 81237
    x = _logits(rng, n, 20, 1.0, ties=64)
    label = R.make_labels(rng, n, 20, "invalid")
    base = np.zeros((20, 20), dtype=np.int64)
    base.flat[rng.choice(400, 60, replace=False)] = 1 << 40
    base.flat[rng.choice(400, 60, replace=False)] = (1 << 32) - 1
    conf = torch.from_numpy(base).cuda()
    _seg(x, label, _cfg_weights(), ignore_index=3, conf=conf)
    _seg(x, label, _cfg_weights(), ignore_index=3, conf=conf, grad=False)       # the forward-only kernel counts as well
    R.assert_confs_equal((conf.cpu().numpy(),), (base + 2 * R.conf_ref(x, label, 20, 3),))


def test_upstream_scalar_scales_the_gradient():
    rng = np.random.default_rng(11)
    n = 65537
    x = _logits(rng, n, 20, 1.0)
    _check(x, R.make_labels(rng, n, 20, "invalid"), _cfg_weights(), upstream=0.25)


@pytest.mark.parametrize("n", [65537, 300000])
def test_seg_loss_is_deterministic_and_forward_only_gives_the_same_loss(n):
    from fusiontransformer_amd import functional as spf
    rng = np.random.default_rng(13)
    x = _logits(rng, n, 20, 8.0, ties=64)
    label = R.make_labels(rng, n, 20, "invalid")
    t = torch.from_numpy(x).cuda()
    lab, cw = torch.from_numpy(label).cuda(), torch.from_numpy(_cfg_weights()).cuda()
    out = []
    for _ in range(2):
        a = t.clone().requires_grad_(True)
        conf = torch.zeros((20, 20), dtype=torch.int64, device="cuda")
        loss = spf.seg_loss(a, lab, cw, conf=conf)
        loss.backward()
        out.append((loss.detach(), a.grad, conf))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])
    conf = torch.zeros((20, 20), dtype=torch.int64, device="cuda")
    with torch.no_grad():
        fwd = spf.seg_loss(t.clone().requires_grad_(True), lab, cw, conf=conf)
    assert not fwd.requires_grad
    assert torch.equal(fwd, out[0][0]) and torch.equal(conf, out[0][2])
    assert torch.equal(spf.seg_loss(t, lab, cw), out[0][0])        # a logit that requires no gradient: forward-only as well


def test_no_grad_allocates_no_gradient_buffer():
    from fusiontransformer_amd import functional as spf
    n, c = 300000, 20
    rng = np.random.default_rng(14)
    t = torch.from_numpy(_logits(rng, n, c)).cuda().requires_grad_(True)
    lab, cw = torch.from_numpy(R.make_labels(rng, n, c, "uniform")).cuda(), torch.from_numpy(_cfg_weights()).cuda()
    spf.seg_loss(t, lab, cw).backward()       # warm: library loaded, allocator pools filled
    t.grad = None
    torch.cuda.synchronize()

    def peak(fn):
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, out

    def forward_only():
        with torch.no_grad():
            return spf.seg_loss(t, lab, cw)

    d0, _ = peak(forward_only)
    d1, _ = peak(lambda: spf.seg_loss(t.detach(), lab, cw))
    d2, keep = peak(lambda: spf.seg_loss(t, lab, cw))
    assert d0 < n * c * 4 and d1 < n * c * 4, (d0, d1)
    assert d2 >= n * c * 4, d2                # the measurement does see the buffer when there is one
    del keep


# ------------------------------------------------------------------------------------------------ the parent's kernel
@pytest.mark.parametrize("n,scale", [(81237, 1.0), (300000, 8.0), (257, 40.0)])
def test_seg_loss_agrees_with_the_fused_kernel_fed_one_tensor_twice(n, scale, record_property):
    """fusion_loss with the same values as both main heads, lambda_xm = 0, single head -- the only way the fused kernel gives this
    loss: both of its losses, the gradient of either head and both matrices, within the same gates."""
    from fusiontransformer_amd import functional as spf
    rng = np.random.default_rng(15 + n)
    x = _logits(rng, n, 20, scale, ties=64)
    label = R.make_labels(rng, n, 20, "invalid")
    got, gg, conf = _seg(x, label, _cfg_weights(), ignore_index=3)
    a = torch.from_numpy(x).cuda().requires_grad_(True)
    b = torch.from_numpy(x).cuda().requires_grad_(True)
    c3, c2 = (torch.zeros((20, 20), dtype=torch.int64, device="cuda") for _ in range(2))
    l2, l3 = spf.fusion_loss({"lidar_seg_logit": a, "img_seg_logit": b}, torch.from_numpy(label).cuda(), torch.from_numpy(_cfg_weights()).cuda(),
                             0.0, False, conf3d=c3, conf2d=c2, ignore_index=3)
    (l2 + l3).backward()
    xmax = float(np.abs(x).max())
    R.assert_losses_close((got, got), (l2.item(), l3.item()))
    for t in (a, b):
        R.assert_grads_close({KEY: gg}, {KEY: t.grad.cpu().numpy().astype(np.float64)}, xmax)
    R.assert_confs_equal((conf, conf), (c3.cpu().numpy(), c2.cpu().numpy()))
    record_property("bit_identical", bool(got == l3.item() and np.array_equal(gg, a.grad.cpu().numpy())))


# ------------------------------------------------------------------------------------------------ refusals
def test_c_abi_refuses_bad_sizes_before_any_launch(ftx_lib):
    """n = 0, C not a multiple of 4 or above 32, a short workspace: errors returned before the first launch."""
    L = ftx_lib
    n, c = 8, 20
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    logit, grad, loss = f(n, 40), f(n, 40), f(1)
    label = torch.zeros(n, dtype=torch.int64, device="cuda")
    need = int(L.ftx_seg_loss_workspace_bytes())
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream
    for nn, cc, ws_bytes, text in ((0, c, need, b"at least one point"), (n, 19, need, b"multiple of 4"), (n, 36, need, b"multiple of 4"),
                                   (n, c, need - 1, b"workspace too small")):
        assert L.ftx_seg_loss(p(logit), p(label), None, nn, cc, 0, p(loss), p(grad), None, p(ws), ws_bytes, s) != 0, (nn, cc, ws_bytes)
        assert text in L.ftx_last_error(), (nn, cc, ws_bytes)
    assert L.ftx_seg_loss(None, p(label), None, n, c, 0, p(loss), None, None, p(ws), need, s) != 0
    assert b"null pointer" in L.ftx_last_error()
    torch.cuda.synchronize()
    assert not loss.any() and not grad.any()


BAD_OPERANDS = ("cw_float64", "cw_cpu", "cw_short", "cw_long", "cw_2d", "cw_strided", "conf_int32", "conf_small", "conf_flat", "conf_cpu",
                "conf_transposed", "logit_float64", "logit_cpu", "logit_3d", "label_short", "label_2d", "label_float", "label_cpu")


def _bad_operands():
    n, c = 300, 20
    f = lambda *s, **kw: torch.zeros(s, dtype=kw.get("dtype", torch.float32), device=kw.get("device", "cuda"))
    good = dict(logit=f(n, c), label=f(n, dtype=torch.int64), cw=f(c), conf=f(c, c, dtype=torch.int64))
    bad = {
        "cw_float64": dict(cw=f(c, dtype=torch.float64)),
        "cw_cpu": dict(cw=f(c, device="cpu")),
        "cw_short": dict(cw=f(c - 4)),
        "cw_long": dict(cw=f(c + 1)),
        "cw_2d": dict(cw=f(1, c)),
        "cw_strided": dict(cw=f(2 * c)[::2]),
        "conf_int32": dict(conf=f(c, c, dtype=torch.int32)),
        "conf_small": dict(conf=f(c - 4, c - 4, dtype=torch.int64)),
        "conf_flat": dict(conf=f(c * c, dtype=torch.int64)),
        "conf_cpu": dict(conf=f(c, c, dtype=torch.int64, device="cpu")),
        "conf_transposed": dict(conf=f(c, c, dtype=torch.int64).t()),
        "logit_float64": dict(logit=f(n, c, dtype=torch.float64)),
        "logit_cpu": dict(logit=f(n, c, device="cpu")),
        "logit_3d": dict(logit=f(n, c, 1)),
        "label_short": dict(label=f(n - 1, dtype=torch.int64)),
        "label_2d": dict(label=f(n, 1, dtype=torch.int64)),
        "label_float": dict(label=f(n)),
        "label_cpu": dict(label=f(n, dtype=torch.int64, device="cpu")),
    }
    return good, bad


@pytest.mark.parametrize("with_grad", [True, False])
@pytest.mark.parametrize("case", BAD_OPERANDS)
def test_seg_loss_refuses_bad_operands_before_launch(case, with_grad, monkeypatch):
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    good, bad = _bad_operands()
    args = dict(good, **bad[case])
    monkeypatch.setattr(_lib, "load", lambda: _NoLaunch())
    with pytest.raises(ValueError):
        spf.seg_loss(args["logit"].requires_grad_(with_grad), args["label"], args["cw"], conf=args["conf"])
    # the good operands do reach the (stubbed) launch
    with pytest.raises(AssertionError, match="launched"):
        spf.seg_loss(good["logit"].requires_grad_(with_grad), good["label"], good["cw"], conf=good["conf"])


# ------------------------------------------------------------------------------------------------ TrainStep on the device
@pytest.mark.parametrize("mode", ["lidar", "image"])
def test_train_step_fused_and_host_paths_agree(mode, monkeypatch):
    from fusiontransformer_amd import config
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.models.metric import SegIoU
    from fusiontransformer_amd.trainer import TrainStep
    from tests.test_single_modality_host import MODES, _OneHead
    cfg_fn, key, loss_key, metric_name = MODES[mode]
    cfg = getattr(config, cfg_fn)()
    rng = np.random.default_rng(20)
    n = 4000
    x = _logits(rng, n, 20, 1.0, ties=64)
    label = R.make_labels(rng, n, 20, "zero30")
    calls = []
    real = spf.seg_loss
    monkeypatch.setattr(spf, "seg_loss", lambda *a, **kw: calls.append(kw.get("ignore_index")) or real(*a, **kw))
    out = {}
    for fused in (True, False):
        model = _OneHead(key, x).cuda()
        metric = SegIoU(20, 3, metric_name)
        step = TrainStep(cfg, model, optimizer=torch.optim.SGD(model.parameters(), lr=0.0), metrics=metric)
        step.fused_loss = fused
        step({"seg_label": torch.from_numpy(label).cuda()})
        assert set(step.last) == {loss_key}
        out[fused] = (step.last[loss_key].item(), model.head.grad.cpu().numpy(), metric.mat.cpu().numpy())
    assert calls == [3]
    R.assert_confs_equal((out[True][2], out[False][2]), (R.conf_ref(x, label, 20, 3),) * 2)
    R.assert_losses_close((out[True][0],), (out[False][0],))
    R.assert_grads_close({KEY: out[True][1]}, {KEY: out[False][1]}, float(np.abs(x).max()))


# ------------------------------------------------------------------------------------------------ validation loss
def _raw_frame(seed, n):
    rng = np.random.default_rng(seed)
    pts = (rng.uniform(-1, 1, size=(n, 3)) * np.array([40, 25, 2.5])).astype(np.float32)
    pts[:, 0] = np.abs(pts[:, 0])
    pts[: n // 3] = np.round(pts[: n // 3] * 4) / 4          # several points per voxel
    return dict(points=pts, feats=np.concatenate([pts, rng.uniform(0, 1, (n, 1)).astype(np.float32)], 1),
                seg_label=rng.integers(0, 20, n).astype(np.int64),
                img_indices=np.stack([rng.integers(0, 370, n), rng.integers(0, 1226, n)], 1).astype(np.int64),
                img=rng.standard_normal((3, 370, 1226)).astype(np.float32))


@pytest.mark.parametrize("heads", ["3d", "2d", "both"])
def test_validate_batch_adds_the_validation_losses(heads):
    from fusiontransformer_amd.data.voxelize import collate_device, voxelize_frames
    from fusiontransformer_amd.evaluate import Evaluator, validate_batch
    frames = voxelize_frames([{k: torch.from_numpy(v).cuda() for k, v in _raw_frame(s, n).items()} for s, n in ((5, 5000), (6, 3000))])
    batch = collate_device(frames, output_orig=True)
    n = batch["seg_label"].shape[0]
    rng = np.random.default_rng(30)
    lg = {k: _logits(rng, n, 20, 2.0) for k, on in (("lidar_seg_logit", heads != "2d"), ("img_seg_logit", heads != "3d")) if on}
    preds = {k: torch.from_numpy(v).cuda() for k, v in lg.items()}
    cw = _cfg_weights()
    labels = np.arange(20)

    def run(**kw):
        ev = [Evaluator([str(i) for i in range(20)], labels) for _ in range(3)]
        out = validate_batch(preds, batch, labels, evaluator_3d=ev[0] if heads != "2d" else None, evaluator_2d=ev[1] if heads != "3d" else None,
                             evaluator_ensemble=ev[2] if heads == "both" else None, want_preds=True, **kw)
        return out, [e.mat.clone() for e in ev]

    plain, mats0 = run()
    assert set(plain) == {"pred_3d", "pred_2d", "pred_ensemble", "bad_index_flag"}
    out, mats1 = run(seg_label=batch["seg_label"], class_weights=torch.from_numpy(cw).cuda())
    want = {"3d": {"seg_loss_3d"}, "2d": {"seg_loss_2d"}, "both": {"seg_loss_3d", "seg_loss_2d"}}[heads]
    assert set(out) == set(plain) | want
    for k in plain:
        assert (plain[k] is None and out[k] is None) or torch.equal(plain[k], out[k]), k
    for a, b in zip(mats0, mats1):
        assert torch.equal(a, b)
    lab = batch["seg_label"].cpu().numpy()
    for k, name in (("lidar_seg_logit", "seg_loss_3d"), ("img_seg_logit", "seg_loss_2d")):
        if k in lg:
            v = out[name]
            assert v.is_cuda and v.dim() == 0 and not v.requires_grad
            R.assert_losses_close((v.item(),), (seg_oracle(lg[k], lab, cw)[0],))
