"""The fused loss (csrc/ftx_loss.hip, ftx_fusion_loss_mix) and the evaluation scatter-back (csrc/ftx_eval.hip) at full size,
against float64 references (tests/loss_metric_ref.py), plus the operand checks in front of them.

Loss gates (tests/loss_metric_ref.py): losses |d| <= 2e-6 * max(1, |ref|); gradients per element rtol 1e-4 plus an absolute
part of grad_atol(max|logit|) * max|ref| per tensor (1e-6 for logits within +-4, growing with max|x| because the kernel's
float32 log-probabilities x - lse carry an absolute rounding error of about an ulp of max|x|); confusion matrices bit-exact.
The sizes straddle the kernel's launch geometry: 256-point blocks, at most 256 of them (reached from n = 65 281 on), a grid-stride
loop whose second pass starts at n = 65 537, and the 256-row finalize."""
import numpy as np
import pytest
import torch

from tests import loss_metric_ref as R
from tests.nolaunch import NoLaunch as _NoLaunch

pytestmark = pytest.mark.gpu

NAMES = R.NAMES


def _cfg_weights():
    from fusiontransformer_amd.config import _CLASS_WEIGHTS
    return np.array(_CLASS_WEIGHTS, dtype=np.float32)


def _fused(lg, label, cw, lam, dual, mix="additive", ignore_index=0, upstream=(1.0, 1.0), confs=None):
    """One call through functional.fusion_loss + backward: losses, gradients of every head (None if none), both matrices."""
    from fusiontransformer_amd import functional as spf
    preds = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in lg.items()}
    c = lg[NAMES[0]].shape[1]
    if confs is None:
        confs = tuple(torch.zeros((c, c), dtype=torch.int64, device="cuda") for _ in range(2))
    l2, l3 = spf.fusion_loss(preds, torch.from_numpy(np.asarray(label)).cuda(), None if cw is None else torch.from_numpy(cw).cuda(), lam,
                             dual, conf3d=confs[0], conf2d=confs[1], ignore_index=ignore_index, mix=mix)
    (l3 if upstream == (0.0, 1.0) else upstream[0] * l2 + upstream[1] * l3).backward()
    grads = {k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in preds.items()}
    return (l2.item(), l3.item()), grads, tuple(m.cpu().numpy() for m in confs)


def _check(lg, label, cw, lam, dual, mix="additive", ignore_index=0):
    got, gg, confs = _fused(lg, label, cw, lam, dual, mix, ignore_index)
    ref, rg = R.oracle_losses(lg, label, cw, lam, dual, mix)
    c = lg[NAMES[0]].shape[1]
    xmax = R.logit_max(lg)
    R.assert_losses_close(got, ref)
    R.assert_grads_close(gg, rg, xmax)
    R.assert_confs_equal(confs, (R.conf_ref(lg[NAMES[0]], label, c, ignore_index), R.conf_ref(lg[NAMES[1]], label, c, ignore_index)))
    return R.loss_error(got, ref), R.grad_error(gg, rg, xmax)


# ------------------------------------------------------------------------------------------------ sizes and class counts
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4000, 65280, 65281, 65536, 65537, 81237, 300000])
def test_fused_loss_sizes(n):
    rng = np.random.default_rng(n)
    lg = R.make_logits(rng, n, 20, 1.0, ties=min(n, 64))
    label = R.make_labels(rng, n, 20, "invalid") if n > 1 else np.array([5])      # one point: a label of non-zero weight
    _check(lg, label, _cfg_weights(), 0.1, True)


@pytest.mark.parametrize("n", [5, 65537])
@pytest.mark.parametrize("c", [4, 8, 12, 16, 20, 24, 28, 32])
def test_fused_loss_every_class_count(c, n):
    rng = np.random.default_rng(100 * c + n)
    lg = R.make_logits(rng, n, c, 1.0, ties=min(n, 32))
    _check(lg, R.make_labels(rng, n, c, "uniform"), R.spread_weights(rng, c), 0.1, True)


# ------------------------------------------------------------------------------------------------ modes, labels, logits
@pytest.mark.parametrize("weights", ["none", "config", "spread"])
@pytest.mark.parametrize("mix,lam", [("additive", 0.0), ("additive", 0.1), ("torchpack", 0.1), ("torchpack", 0.5)])
@pytest.mark.parametrize("dual", [True, False])
def test_fused_loss_modes(dual, mix, lam, weights):
    rng = np.random.default_rng(7)
    n = 65537
    lg = R.make_logits(rng, n, 20, 1.0, dual=dual, ties=64)
    cw = {"none": None, "config": _cfg_weights(), "spread": R.spread_weights(rng, 20)}[weights]
    _check(lg, R.make_labels(rng, n, 20, "uniform"), cw, lam, dual, mix)


@pytest.mark.parametrize("ignore_index", [0, 3, 77])
@pytest.mark.parametrize("kind", ["uniform", "zero30", "single", "invalid"])
def test_fused_loss_label_mixes(kind, ignore_index):
    rng = np.random.default_rng(8)
    n = 65537
    lg = R.make_logits(rng, n, 20, 1.0, ties=64)
    _check(lg, R.make_labels(rng, n, 20, kind), _cfg_weights(), 0.1, True, ignore_index=ignore_index)


@pytest.mark.parametrize("dual", [True, False])
@pytest.mark.parametrize("scale", [1.0, 8.0, 40.0])
def test_fused_loss_logit_scales(scale, dual, record_property):
    """N(0,1) * scale: at 40 most float32 probabilities underflow (the t > 0 guards of the KL terms).  The worst errors, as
    multiples of the gate, are recorded as test properties."""
    rng = np.random.default_rng(int(scale) + 10 * dual)
    n = 300000
    lg = R.make_logits(rng, n, 20, scale, dual=dual, ties=256)
    le, ge = _check(lg, R.make_labels(rng, n, 20, "invalid"), _cfg_weights(), 0.1, dual)
    record_property("loss_rel_err", le)
    record_property("grad_err_over_gate", ge)


@pytest.mark.parametrize("labels", ["zeros_cfg_weights", "all_invalid"])
def test_fused_loss_is_nan_when_the_total_weight_is_zero(labels):
    rng = np.random.default_rng(9)
    n = 1000
    lg = R.make_logits(rng, n, 20)
    if labels == "zeros_cfg_weights":
        label, cw = R.make_labels(rng, n, 20, "zeros"), _cfg_weights()
    else:
        label, cw = np.full(n, -100, dtype=np.int64), None
        label[::3] = 255
    ref, _ = R.oracle_losses(lg, label, cw, 0.1, True)
    assert np.isnan(ref[0]) and np.isnan(ref[1])
    got, _, confs = _fused(lg, label, cw, 0.1, True)
    R.assert_losses_close(got, ref)
    if labels == "all_invalid":
        assert not confs[0].any() and not confs[1].any()


# ------------------------------------------------------------------------------------------------ matrices, upstream, determinism
def test_confusion_matrices_carry_and_accumulate():
    """Cells pre-filled with 2^40 and 2^32 - 1 (the 64-bit add must carry out of the low word), accumulated over two calls."""
    rng = np.random.default_rng(10)
    n = 81237
    lg = R.make_logits(rng, n, 20, 1.0, ties=64)
    label = R.make_labels(rng, n, 20, "invalid")
    base = np.zeros((20, 20), dtype=np.int64)
    base.flat[rng.choice(400, 60, replace=False)] = 1 << 40
    base.flat[rng.choice(400, 60, replace=False)] = (1 << 32) - 1
    confs = (torch.from_numpy(base).cuda(), torch.from_numpy(base.copy()).cuda())
    for _ in range(2):
        _fused(lg, label, _cfg_weights(), 0.1, True, ignore_index=3, confs=confs)
    ref = (R.conf_ref(lg[NAMES[0]], label, 20, 3), R.conf_ref(lg[NAMES[1]], label, 20, 3))
    R.assert_confs_equal(tuple(m.cpu().numpy() for m in confs), (base + 2 * ref[0], base + 2 * ref[1]))


@pytest.mark.parametrize("upstream", [(0.25, 3.0), (0.0, 1.0)])
def test_dual_head_upstream_gradients(upstream):
    rng = np.random.default_rng(11)
    n = 65537
    lg = R.make_logits(rng, n, 20, 1.0)
    label = R.make_labels(rng, n, 20, "invalid")
    got, gg, _ = _fused(lg, label, _cfg_weights(), 0.1, True, upstream=upstream)
    ref, rg = R.oracle_losses(lg, label, _cfg_weights(), 0.1, True, upstream=upstream)
    R.assert_losses_close(got, ref)
    R.assert_grads_close(gg, rg, R.logit_max(lg))
    if upstream[0] == 0:     # l3.backward() on its own: nothing reaches the image heads
        assert not gg["img_seg_logit"].any() and not gg["img_seg_logit2"].any()


def test_single_head_upstream_gradients():
    from fusiontransformer_amd import functional as spf
    rng = np.random.default_rng(12)
    n = 4000
    lg = R.make_logits(rng, n, 20, 1.0, dual=False)
    label = R.make_labels(rng, n, 20, "uniform")
    got, gg, _ = _fused(lg, label, _cfg_weights(), 0.1, False, upstream=(0.5, 0.5))
    ref, rg = R.oracle_losses(lg, label, _cfg_weights(), 0.1, False, upstream=(0.5, 0.5))
    R.assert_losses_close(got, ref)
    R.assert_grads_close(gg, rg, R.logit_max(lg))
    preds = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in lg.items()}
    l2, l3 = spf.fusion_loss(preds, torch.from_numpy(label).cuda(), torch.from_numpy(_cfg_weights()).cuda(), 0.1, False)
    with pytest.raises(RuntimeError):
        (0.5 * l2 + l3).backward()


@pytest.mark.parametrize("n", [65537, 300000])
def test_fused_loss_is_deterministic(n):
    rng = np.random.default_rng(13)
    lg = R.make_logits(rng, n, 20, 8.0, ties=64)
    label = R.make_labels(rng, n, 20, "invalid")
    a = _fused(lg, label, _cfg_weights(), 0.1, True)
    b = _fused(lg, label, _cfg_weights(), 0.1, True)
    assert np.array_equal(np.array(a[0]), np.array(b[0]))
    for k in NAMES:
        assert np.array_equal(a[1][k], b[1][k]), k
    R.assert_confs_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------ refusals
def test_c_abi_refuses_bad_sizes_before_any_launch(ftx_lib):
    """n = 0, C not a multiple of 4 or above 32, a short workspace: FTX_REQUIRE errors, checked before the first launch."""
    L = ftx_lib
    n, c = 8, 20
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    l3, l2, l3b, l2b, g3, g2, g3b, g2b = (f(n, 40) for _ in range(8))
    label = torch.zeros(n, dtype=torch.int64, device="cuda")
    losses = f(2)
    need = int(L.ftx_fusion_loss_workspace_bytes())
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    s = torch.cuda.current_stream().cuda_stream

    def call(nn, cc, ws_bytes):
        return L.ftx_fusion_loss_mix(p(l3), p(l2), p(l3b), p(l2b), p(label), None, 1.0, 0.1, nn, cc, 0, p(losses), p(g3), p(g2), p(g3b),
                                     p(g2b), None, None, p(ws), ws_bytes, s)

    for nn, cc, ws_bytes, text in ((0, c, need, b"at least one point"), (n, 19, need, b"multiple of 4"), (n, 36, need, b"multiple of 4"),
                                   (n, c, need - 1, b"workspace too small")):
        assert call(nn, cc, ws_bytes) != 0, (nn, cc, ws_bytes)
        assert text in L.ftx_last_error(), (nn, cc, ws_bytes)
    torch.cuda.synchronize()


BAD_OPERANDS = ("cw_float64", "cw_cpu", "cw_short", "cw_long", "cw_2d", "cw_strided", "conf3d_int32", "conf2d_int32", "conf3d_small",
                "conf2d_small", "conf3d_flat", "conf2d_cpu", "conf3d_transposed", "lidar2_short", "img2_short", "img2_narrow", "img2_float64",
                "lidar2_cpu", "label_short", "label_2d")


def _bad_operands():
    n, c = 300, 20
    f = lambda *s, **kw: torch.zeros(s, dtype=kw.get("dtype", torch.float32), device=kw.get("device", "cuda"))
    good = dict(preds={k: f(n, c) for k in NAMES}, label=f(n, dtype=torch.int64), cw=f(c), conf3d=f(c, c, dtype=torch.int64),
                conf2d=f(c, c, dtype=torch.int64))
    bad = {
        "cw_float64": dict(cw=f(c, dtype=torch.float64)),
        "cw_cpu": dict(cw=f(c, device="cpu")),
        "cw_short": dict(cw=f(c - 4)),
        "cw_long": dict(cw=f(c + 1)),
        "cw_2d": dict(cw=f(1, c)),
        "cw_strided": dict(cw=f(2 * c)[::2]),
        "conf3d_int32": dict(conf3d=f(c, c, dtype=torch.int32)),
        "conf2d_int32": dict(conf2d=f(c, c, dtype=torch.int32)),
        "conf3d_small": dict(conf3d=f(c - 4, c - 4, dtype=torch.int64)),
        "conf2d_small": dict(conf2d=f(c - 4, c - 4, dtype=torch.int64)),
        "conf3d_flat": dict(conf3d=f(c * c, dtype=torch.int64)),
        "conf2d_cpu": dict(conf2d=f(c, c, dtype=torch.int64, device="cpu")),
        "conf3d_transposed": dict(conf3d=f(c, c, dtype=torch.int64).t()),
        "lidar2_short": dict(preds={**good["preds"], "lidar_seg_logit2": f(n - 1, c)}),
        "img2_short": dict(preds={**good["preds"], "img_seg_logit2": f(n - 1, c)}),
        "img2_narrow": dict(preds={**good["preds"], "img_seg_logit2": f(n, c - 4)}),
        "img2_float64": dict(preds={**good["preds"], "img_seg_logit2": f(n, c, dtype=torch.float64)}),
        "lidar2_cpu": dict(preds={**good["preds"], "lidar_seg_logit2": f(n, c, device="cpu")}),
        "label_short": dict(label=f(n - 1, dtype=torch.int64)),
        "label_2d": dict(label=f(n, 1, dtype=torch.int64)),
    }
    return good, bad


@pytest.mark.parametrize("case", BAD_OPERANDS)
def test_fusion_loss_refuses_bad_operands_before_launch(case, monkeypatch):
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    good, bad = _bad_operands()
    args = dict(good, **bad[case])
    monkeypatch.setattr(_lib, "load", lambda: _NoLaunch())
    with pytest.raises(ValueError):
        spf.fusion_loss(args["preds"], args["label"], args["cw"], 0.1, True, conf3d=args["conf3d"], conf2d=args["conf2d"])
    # the good operands do reach the (stubbed) launch
    with pytest.raises(AssertionError, match="launched"):
        spf.fusion_loss(good["preds"], good["label"], good["cw"], 0.1, True, conf3d=good["conf3d"], conf2d=good["conf2d"])


# ------------------------------------------------------------------------------------------------ TrainStep
class _Logits(torch.nn.Module):
    """A model whose four logit heads are its own parameters."""

    def __init__(self, lg):
        super().__init__()
        self.heads = torch.nn.ParameterDict({k: torch.nn.Parameter(torch.from_numpy(v.copy())) for k, v in lg.items()})

    def forward(self, batch):
        return {k: 1.0 * p for k, p in self.heads.items()}


def _train_step(lg, label, fused, metrics):
    from fusiontransformer_amd.config import fusion_cfg
    from fusiontransformer_amd.trainer import TrainStep
    cfg = fusion_cfg("middle")
    model = _Logits(lg).cuda()
    step = TrainStep(cfg, model, optimizer=torch.optim.SGD(model.parameters(), lr=0.0), metrics=metrics)
    step.fused_loss = fused
    step({"seg_label": torch.from_numpy(label).cuda()})
    losses = (step.last["loss_2d"].item(), step.last["loss_3d"].item())
    return losses, {k: p.grad.cpu().numpy() for k, p in model.heads.items()}


@pytest.mark.parametrize("ignore_index", [0, 3])
def test_train_step_fused_and_host_paths_agree(ignore_index, monkeypatch):
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.models.metric import SegIoU
    rng = np.random.default_rng(20 + ignore_index)
    n = 4000
    lg = R.make_logits(rng, n, 20, 1.0, ties=64)
    label = R.make_labels(rng, n, 20, "zero30")
    calls = []
    real = spf.fusion_loss
    monkeypatch.setattr(spf, "fusion_loss", lambda *a, **kw: calls.append(kw.get("ignore_index")) or real(*a, **kw))
    out = {}
    for fused in (True, False):
        metrics = (SegIoU(20, ignore_index, "seg_iou_2d"), SegIoU(20, ignore_index, "seg_iou_3d"))
        out[fused] = _train_step(lg, label, fused, metrics) + (tuple(m.mat.cpu().numpy() for m in metrics),)
    assert calls == [ignore_index]
    R.assert_confs_equal(out[True][2], out[False][2])
    R.assert_confs_equal(out[True][2], (R.conf_ref(lg[NAMES[1]], label, 20, ignore_index), R.conf_ref(lg[NAMES[0]], label, 20, ignore_index)))
    R.assert_losses_close(out[True][0], out[False][0])
    R.assert_grads_close(out[True][1], out[False][1], R.logit_max(lg))


def test_train_step_takes_the_host_path_for_mismatched_metrics(monkeypatch):
    """A metric of another class count, or two metrics with different ignore indices, cannot share the kernel's matrices: the
    step falls back to the host loss + update_dict, and nothing is written past the small metric's matrix."""
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.models.metric import SegIoU
    rng = np.random.default_rng(30)
    n = 4000
    lg = R.make_logits(rng, n, 20, 1.0)
    label = R.make_labels(rng, n, 20, "uniform")
    monkeypatch.setattr(spf, "fusion_loss", lambda *a, **kw: (_ for _ in ()).throw(AssertionError("fused path taken")))
    k = 16
    buf = torch.zeros(20 * 20 + 64, dtype=torch.int64, device="cuda")
    small = SegIoU(k, 0, "seg_iou_3d")
    small.mat = buf[:k * k].view(k, k)
    other = SegIoU(20, 0, "seg_iou_2d")
    _train_step(lg, label, True, (other, small))
    assert not buf[k * k:].any()
    preds = {k_: torch.from_numpy(v).cuda() for k_, v in lg.items()}
    expect = SegIoU(k, 0, "seg_iou_3d")
    expect.update_dict(preds, {"seg_label": torch.from_numpy(label).cuda()})
    assert torch.equal(small.mat, expect.mat)
    R.assert_confs_equal((other.mat.cpu().numpy(),), (R.conf_ref(lg[NAMES[1]], label, 20, 0),))
    # differing ignore indices
    m2, m3 = SegIoU(20, 0, "seg_iou_2d"), SegIoU(20, 3, "seg_iou_3d")
    _train_step(lg, label, True, (m2, m3))
    R.assert_confs_equal((m2.mat.cpu().numpy(), m3.mat.cpu().numpy()),
                         (R.conf_ref(lg[NAMES[1]], label, 20, 0), R.conf_ref(lg[NAMES[0]], label, 20, 3)))


# ------------------------------------------------------------------------------------------------ evaluation scatter-back
EV_CAPPED_M = 2048 * 256 * 8 + 1000      # past the 2 048-block grid cap: the stride loop takes a second pass
EV_ROWS = 81237


def _class_labels(c, with_c):
    """KITTI-like original ids, 0 first.  with_c: id C is among them, so gt id 0 (re-labelled C by the evaluator) is counted."""
    lab = [0] + [i for i in R.KITTI_IDS if i != c][:c - 1]
    if with_c:
        lab[min(5, c - 1)] = c
    return np.array(lab, dtype=np.int32)


def _separated_logits(rng, n, c, ties=32):
    """Logits whose float64 softmax-sum ensemble has a top-two margin >= 1e-3 (rows that fall short are redrawn), so every
    argmax is exact; the first `ties` rows repeat the 3-D maximum exactly, the next `ties` the 2-D one."""
    l3 = (rng.standard_normal((n, c)) * 2).astype(np.float32)
    l2 = (rng.standard_normal((n, c)) * 2).astype(np.float32)
    if c == 1:
        return l3, l2
    for t, (tie, strong) in enumerate(((l3, l2), (l2, l3))):
        for i in range(t * ties, (t + 1) * ties):
            a, b = sorted(rng.choice(c, 2, replace=False))
            tie[i, a] = tie[i, b] = tie[i].max() + np.float32(0.5)
            strong[i, b] = strong[i].max() + np.float32(6)

    def sm(x):
        e = np.exp(x - x.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)

    rows = np.arange(2 * ties, n)
    while len(rows):
        e = np.sort(sm(l3[rows].astype(np.float64)) + sm(l2[rows].astype(np.float64)), 1)
        rows = rows[e[:, -1] - e[:, -2] < 1e-3]
        l3[rows] = (rng.standard_normal((len(rows), c)) * 2).astype(np.float32)
        l2[rows] = (rng.standard_normal((len(rows), c)) * 2).astype(np.float32)
    return l3, l2


def _eval_inputs(rng, shape, c):
    if shape == "frames":      # 4 frames of ~120 k original points onto 81 237 model rows
        n_vox = np.array([20011, 20735, 19876, EV_ROWS - 20011 - 20735 - 19876])
        offs = np.concatenate([[0], np.cumsum(n_vox)[:-1]])
        inverse = np.concatenate([rng.integers(0, nv, int(rng.integers(115000, 125000))) + o for nv, o in zip(n_vox, offs)])
    else:
        inverse = rng.integers(0, EV_ROWS, EV_CAPPED_M)
    return inverse.astype(np.int64), rng.integers(0, c, len(inverse)).astype(np.int32)


def _eval(l3, l2, inverse, gt, labels, confs):
    from fusiontransformer_amd import functional as spf
    p3, p2, pe, bad = spf.eval_scatter_back(torch.from_numpy(l3).cuda(), torch.from_numpy(l2).cuda(), torch.from_numpy(inverse).cuda(),
                                            torch.from_numpy(gt).cuda(), torch.from_numpy(labels), *confs)
    return [p.cpu().numpy() for p in (p3, p2, pe)], int(bad.item())


@pytest.mark.parametrize("with_c", [True, False])
@pytest.mark.parametrize("c", [1, 3, 19, 20, 32])
@pytest.mark.parametrize("shape", ["frames", "capped"])
def test_eval_scatter_back_is_exact(shape, c, with_c):
    rng = np.random.default_rng(1000 * c + 10 * with_c + (shape == "capped"))
    l3, l2 = _separated_logits(rng, EV_ROWS, c)
    inverse, gt = _eval_inputs(rng, shape, c)
    labels = _class_labels(c, with_c)
    preds, mats = R.eval_ref(l3, l2, inverse, gt, labels)
    base = [rng.integers(0, 1 << 40, (c, c)) for _ in range(3)]
    confs = [torch.from_numpy(b).cuda() for b in base]
    got, bad = _eval(l3, l2, inverse, gt, labels, confs)
    assert bad == 0
    for a, b in zip(got, preds):
        assert np.array_equal(a, b)
    _eval(l3, l2, inverse, gt, labels, confs)
    for m, b, r in zip(confs, base, mats):
        assert np.array_equal(m.cpu().numpy(), b + 2 * r)
    assert (sum(r.sum() for r in mats) > 0) == (with_c or c > 1)     # C = 1 without id C: every gt is id 0 and dropped


@pytest.mark.parametrize("shape", ["frames", "capped"])
def test_eval_scatter_back_flags_and_skips_bad_entries(shape):
    rng = np.random.default_rng(77 + (shape == "capped"))
    c = 20
    l3, l2 = _separated_logits(rng, EV_ROWS, c)
    inverse, gt = _eval_inputs(rng, shape, c)
    m = len(inverse)
    pos = rng.choice(m, 40, replace=False)
    inverse[pos[:10]] = -1
    inverse[pos[10:20]] = EV_ROWS + rng.integers(0, 1000, 10)
    gt[pos[20:30]] = -rng.integers(1, 5, 10)
    gt[pos[30:]] = c + rng.integers(0, 5, 10)
    labels = _class_labels(c, True)
    preds, mats = R.eval_ref(l3, l2, inverse, gt, labels)
    confs = [torch.zeros((c, c), dtype=torch.int64, device="cuda") for _ in range(3)]
    got, bad = _eval(l3, l2, inverse, gt, labels, confs)
    assert bad == 1
    ok = np.ones(m, dtype=bool)
    ok[pos] = False
    for a, b in zip(got, preds):
        assert np.array_equal(a[ok], b[ok])      # predictions at the bad positions are unspecified
    for t, r in zip(confs, mats):
        assert np.array_equal(t.cpu().numpy(), r)


def test_eval_scatter_back_refusals():
    from fusiontransformer_amd import functional as spf
    rng = np.random.default_rng(5)
    inverse, gt = torch.zeros(100, dtype=torch.int64, device="cuda"), torch.zeros(100, dtype=torch.int32, device="cuda")
    l33 = torch.from_numpy(rng.standard_normal((10, 33)).astype(np.float32)).cuda()
    with pytest.raises(RuntimeError, match="num_classes"):
        spf.eval_scatter_back(l33, l33, inverse, gt, torch.arange(33))
    l20 = l33[:, :20].contiguous()
    for bad in (torch.zeros((19, 19), dtype=torch.int64, device="cuda"), torch.zeros((20, 20), dtype=torch.int32, device="cuda"),
                torch.zeros(400, dtype=torch.int64, device="cuda")):
        with pytest.raises(ValueError):
            spf.eval_scatter_back(l20, l20, inverse, gt, torch.arange(20), conf3d=bad)
