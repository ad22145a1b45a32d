"""CPU half of the single-modality training path (LidarSeg / ImageSegBilinear): the train step's two single-head modes on stub
models, the model-side pieces (prefetch reaches LidarSeg's SPVCNN, the frozen second head of the image-only model, the two
configurations), validate_batch's unchanged default result, and the strength of the gates tests/test_seg_loss_gpu.py applies to
the single-head loss kernel (csrc/ftx_loss.hip, ftx_seg_loss): a float64 restatement of that kernel with one planted mistake at a
time must fail them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_metric_ref as R
from tests.seg_loss_ref import host_seg, seg_oracle


class _OneHead(torch.nn.Module):
    """A model whose only output is one logits tensor, its own parameter."""

    def __init__(self, key, logits):
        super().__init__()
        self.key = key
        self.head = torch.nn.Parameter(torch.from_numpy(logits.copy()))

    def forward(self, batch):
        return {self.key: 1.0 * self.head}


def _case(rng, n=4000, c=20, scale=1.0, kind="invalid"):
    x = R.make_logits(rng, n, c, scale, dual=False, ties=40)[R.NAMES[0]]
    return x, R.make_labels(rng, n, c, kind), R.spread_weights(rng, c)


MODES = {"lidar": ("lidar_cfg", "lidar_seg_logit", "loss_3d", "seg_iou_3d"), "image": ("image_cfg", "img_seg_logit", "loss_2d", "seg_iou_2d")}


@pytest.mark.parametrize("mode", ["lidar", "image"])
def test_train_step_single_head_on_a_stub_model(mode):
    from fusiontransformer_amd import config
    from fusiontransformer_amd.models.metric import SegIoU
    from fusiontransformer_amd.trainer import TrainStep
    cfg_fn, key, loss_key, metric_name = MODES[mode]
    cfg = getattr(config, cfg_fn)()
    rng = np.random.default_rng(3 + (mode == "image"))
    x, label, _ = _case(rng, kind="zero30")
    model = _OneHead(key, x)
    metric = SegIoU(20, 0, metric_name)                      # bare, as build_model returns it for these types
    step = TrainStep(cfg, model, optimizer=torch.optim.SGD(model.parameters(), lr=0.0), metrics=metric)
    preds = step({"seg_label": torch.from_numpy(label)})
    assert set(preds) == {key}
    assert set(step.last) == {loss_key}
    cw = torch.tensor(cfg.TRAIN.CLASS_WEIGHTS, dtype=torch.float32)
    ref_x = torch.from_numpy(x).requires_grad_(True)
    ref = F.cross_entropy(ref_x, torch.from_numpy(label), weight=cw)
    ref.backward()
    assert abs(step.last[loss_key].item() - ref.item()) <= 1e-6 * max(1.0, abs(ref.item()))
    assert model.head.grad is not None
    np.testing.assert_allclose(model.head.grad.numpy(), ref_x.grad.numpy(), rtol=1e-5, atol=1e-9)
    R.assert_confs_equal((metric.mat.numpy(),), (R.conf_ref(x, label, 20, 0),))
    # the same through a tuple that also carries the other modality's metric: only the head that exists is counted
    other = SegIoU(20, 0, "seg_iou_2d" if mode == "lidar" else "seg_iou_3d")
    mine = SegIoU(20, 0, metric_name)
    TrainStep(cfg, model, optimizer=torch.optim.SGD(model.parameters(), lr=0.0), metrics=(other, mine))({"seg_label": torch.from_numpy(label)})
    assert other.mat is None
    R.assert_confs_equal((mine.mat.numpy(),), (R.conf_ref(x, label, 20, 0),))


def test_single_modes_ignore_lambda_and_dual_head_and_take_torchpack_default_weights():
    """lambda_xm and DUAL_HEAD play no part outside fusion; loss_mix="torchpack" changes the default class weights only."""
    from fusiontransformer_amd import config
    from fusiontransformer_amd.trainer import TrainStep, default_class_weights
    rng = np.random.default_rng(5)
    x, label, _ = _case(rng, n=500, kind="uniform")
    cfg = config.lidar_cfg()
    cfg.TRAIN.FusionTransformer.lambda_xm, cfg.MODEL.DUAL_HEAD, cfg.TRAIN.CLASS_WEIGHTS = 0.3, True, []
    model = _OneHead("lidar_seg_logit", x)
    step = TrainStep(cfg, model, optimizer=torch.optim.SGD(model.parameters(), lr=0.0), loss_mix="torchpack")
    step({"seg_label": torch.from_numpy(label)})
    ref = F.cross_entropy(torch.from_numpy(x), torch.from_numpy(label), weight=default_class_weights(20))
    assert abs(step.last["loss_3d"].item() - ref.item()) <= 1e-6


def test_train_step_mode_follows_the_reference_order_and_refuses_no_modality():
    from fusiontransformer_amd import config
    from fusiontransformer_amd.trainer import TrainStep
    model = _OneHead("lidar_seg_logit", np.zeros((4, 20), np.float32))
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    cfg = config.get_cfg_defaults()
    with pytest.raises(ValueError):
        TrainStep(cfg, model, optimizer=opt)
    assert TrainStep(config.lidar_cfg(), model, optimizer=opt).mode == "lidar"
    assert TrainStep(config.image_cfg(), model, optimizer=opt).mode == "image"
    assert TrainStep(config.fusion_cfg("late"), model, optimizer=opt).mode == "fusion"
    cfg.MODEL.USE_LIDAR = cfg.MODEL.USE_IMAGE = True         # USE_LIDAR is asked first
    assert TrainStep(cfg, model, optimizer=opt).mode == "lidar"


def test_single_modality_configs_carry_the_baseline_values():
    from fusiontransformer_amd import config
    for cfg, typ in ((config.lidar_cfg(), "LidarSeg"), (config.image_cfg(), "ImageSegBilinear")):
        m = cfg.MODEL
        assert m.TYPE == typ and m.NUM_CLASSES == 20 and m.DUAL_HEAD is False and m.USE_FUSION is False
        assert (m.USE_LIDAR, m.USE_IMAGE) == ((True, False) if typ == "LidarSeg" else (False, True))
        assert cfg.TRAIN.FusionTransformer.lambda_xm == 0.0
        assert list(cfg.TRAIN.CLASS_WEIGHTS) == list(config.fusion_cfg().TRAIN.CLASS_WEIGHTS)
        assert (cfg.OPTIMIZER.TYPE, cfg.OPTIMIZER.BASE_LR, cfg.OPTIMIZER.WEIGHT_DECAY) == ("Adam", 1e-4, 5e-4)
    assert config.image_cfg().MODEL.late_feat_block_number == 11


def test_image_only_model_freezes_its_second_head():
    from fusiontransformer_amd import config
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.models.metric import SegIoU
    keys = {}
    for dual in (True, False):
        cfg = config.image_cfg()
        cfg.MODEL.DUAL_HEAD = dual
        model, metric = build_model(cfg)
        assert isinstance(metric, SegIoU)
        keys[dual] = set(model.state_dict())
        if dual:
            lin2 = model.image_backbone.linear2
            assert lin2.weight.requires_grad is False and lin2.bias.requires_grad is False
            assert model.image_backbone.linear.weight.requires_grad
    assert keys[True] == keys[False] | {"image_backbone.linear2.weight", "image_backbone.linear2.bias"}


def test_prepare_batch_reaches_the_spvcnn_of_lidarseg():
    from fusiontransformer_amd import config
    from fusiontransformer_amd.models._fusion_common import prepare_batch
    from fusiontransformer_amd.models.build import build_model
    model, _ = build_model(config.lidar_cfg())
    seen = []
    model.backbone.prepare = lambda x, ready=None, wait=True: seen.append((x, ready, wait))
    lidar = object()
    batch = {"lidar": lidar}
    assert prepare_batch(model, batch, ready="event", wait=False) is batch
    assert seen == [(lidar, "event", False)]


@pytest.mark.parametrize("heads", ["3d", "2d", "both"])
def test_validate_batch_keeps_its_result_without_the_new_arguments(heads, monkeypatch):
    from fusiontransformer_amd import evaluate
    l = torch.zeros(6, 20)
    preds = {k: l for k, on in (("lidar_seg_logit", heads != "2d"), ("img_seg_logit", heads != "3d")) if on}
    batch = {"inverse_map_packed": torch.zeros(9, dtype=torch.int64), "orig_seg_label_packed": torch.zeros(9, dtype=torch.int32)}
    monkeypatch.setattr(evaluate.spf, "eval_scatter_back", lambda *a, **kw: ("p3", "p2", "pe", "bad"))
    calls = []
    monkeypatch.setattr(evaluate.spf, "seg_loss", lambda logit, label, cw=None: calls.append((logit, label, cw)) or "loss")
    out = evaluate.validate_batch(preds, batch, np.arange(20))
    assert out == {"pred_3d": "p3", "pred_2d": "p2", "pred_ensemble": "pe", "bad_index_flag": "bad"} and not calls
    label, cw = torch.zeros(6, dtype=torch.int64), torch.ones(20)
    out = evaluate.validate_batch(preds, batch, np.arange(20), seg_label=label, class_weights=cw)
    want = {"3d": {"seg_loss_3d"}, "2d": {"seg_loss_2d"}, "both": {"seg_loss_3d", "seg_loss_2d"}}[heads]
    assert set(out) == {"pred_3d", "pred_2d", "pred_ensemble", "bad_index_flag"} | want
    assert len(calls) == len(want) and all(c[1] is label and c[2] is cw for c in calls)


# ------------------------------------------------------------------------------------------------ gate strength
@pytest.mark.parametrize("weights", ["none", "spread"])
def test_single_head_restatement_passes_the_gates(weights):
    rng = np.random.default_rng(21)
    x, label, cw = _case(rng)
    cw = cw if weights == "spread" else None
    ref, rg = seg_oracle(x, label, cw)
    got, gg, conf = host_seg(x, label, cw, ignore_index=3)
    R.assert_losses_close((got,), (ref,))
    R.assert_grads_close({"g": gg}, {"g": rg}, float(np.abs(x).max()))
    R.assert_confs_equal((conf,), (R.conf_ref(x, label, 20, 3),))


@pytest.mark.parametrize("scale", [1.0, 40.0])
@pytest.mark.parametrize("n", [4000, 65537])
@pytest.mark.parametrize("mistake", ["drop_rows", "w_all_labels", "grad_by_n"])
def test_single_head_loss_and_gradient_gates_catch_planted_mistakes(mistake, n, scale):
    rng = np.random.default_rng(22)
    x, label, cw = _case(rng, n=n, scale=scale)
    label[-1], cw[1] = 1, 10.0          # the last row counts (at n = 65 537 it is the only row of the last block)
    ref, rg = seg_oracle(x, label, cw)
    kw = {mistake: (n % 256 or 256) if mistake == "drop_rows" else True}
    got, gg, _ = host_seg(x, label, cw, **kw)
    if mistake != "grad_by_n":          # that one leaves the loss right
        with pytest.raises(AssertionError):
            R.assert_losses_close((got,), (ref,))
    with pytest.raises(AssertionError):
        R.assert_grads_close({"g": gg}, {"g": rg}, float(np.abs(x).max()))


@pytest.mark.parametrize("mistake", ["last_max", "no_ignore"])
def test_single_head_matrix_gate_catches_planted_mistakes(mistake):
    rng = np.random.default_rng(23)
    x, label, cw = _case(rng)
    _, _, conf = host_seg(x, label, cw, ignore_index=3, **{mistake: True})
    with pytest.raises(AssertionError):
        R.assert_confs_equal((conf,), (R.conf_ref(x, label, 20, 3),))
