"""Train-mode parity of the single-modality baselines on whole SemanticKITTI-shaped frames, modelled on
tests/test_fullsize_train_gpu.py: LidarSeg (SPVCNN + one head, the index prefetch of the next batch running) and ImageSegBilinear
(the full 12-block trunk tapped after block 11, replayed as a HIP graph), the single-head loss kernel and the one-launch Adam,
three steps over two ALTERNATING batches (reference: modules/SemanticTrainer.py:180-200).

Every step is checked against the CPU oracle run in float64 from the SAME pre-step state: per-point logits, the loss, BatchNorm
running statistics, every parameter gradient (L2-relative, with the floor of the fusion test).  A twin runs the same steps --
without the prefetch (LidarSeg) or with the eager trunk (ImageSegBilinear) -- and must agree bit for bit.

The gates are the fusion test's: they were set at three times the worst value measured on an MI355X for the same layers, the same
two batches and the float64 oracle (profiles/r03_grad_parity_fullsize.json).  The measured single-modality values are written to
$FTX_TEST_REPORT_DIR/single_modality_parity.json (committed as profiles/single_modality_parity.json).  Measured on an MI355X:
LidarSeg logits 1.5e-5, loss 1.5e-7, BatchNorm buffers 2.5e-7, worst gradient 1.4e-3 / 4.6e-3 / 5.3e-3 over the three steps (BatchNorm
biases of the first convolution of the deep residual blocks: above a third of the 1e-2 gate, which was not moved); ImageSegBilinear
logits 1.8e-5, loss 2.0e-7, buffers 8.1e-8, gradients 5.3e-6."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import product_inputs
from tests.test_fullsize_train_gpu import TOL_GRAD, TOL_LOGIT, TOL_LOSS, _masks, _snapshot

pytestmark = pytest.mark.gpu
TOL_BN = 1e-4
_REPORT = {}


def _write_report(name, rows):
    _REPORT[name] = rows
    d = os.environ.get("FTX_TEST_REPORT_DIR")
    if d:    # optional diagnostic, written where the caller asks
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, "single_modality_parity.json")
        merged = json.load(open(path)) if os.path.exists(path) else {}
        merged.update(_REPORT)
        json.dump(merged, open(path, "w"), indent=1)


def _judge(name, s, which, batch, model, step, loss_key, logit, ref_logit, ref_loss, oracle, prefix, report):
    """Logits, loss, gradients and BatchNorm buffers of one step against the float64 oracle (which has run its backward)."""
    err = (logit.detach().cpu().double() - ref_logit.detach()).abs().max().item()
    loss = step.last[loss_key].item()
    gm = dict(model.named_parameters())
    p64 = dict(oracle.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in p64.values() if p.grad is not None)
    rows = []
    for pname, p in p64.items():
        mine = gm[prefix + pname]
        if p.grad is None:
            assert mine.grad is None or mine.grad.abs().max().item() == 0, (s, pname)
            continue
        assert mine.grad is not None, (s, pname)
        gp = mine.grad.cpu().double()
        floor = 1e-4 * gmax * p.numel() ** 0.5       # gradients that are 0 in exact arithmetic (Linear biases in front of a BatchNorm) are rounding noise
        rows.append(((gp - p.grad).norm().item() / max(p.grad.norm().item(), floor), pname))
    rows.sort(reverse=True)
    bo, bp = dict(oracle.named_buffers()), dict(model.named_buffers())
    worst_bn = max([(bp[prefix + k].cpu().double() - v).abs().max().item() for k, v in bo.items() if v.dtype.is_floating_point] or [0.0])
    report.append({"step": s, "batch": which, "points": int(batch["coords"].shape[0]), "worst_logit_err": err, "loss": loss,
                   "oracle_loss": ref_loss, "loss_err": abs(loss - ref_loss), "worst_bn_buffer_err": worst_bn, "worst_grad_rel_l2": rows[:8]})
    print("%s step %d: logit %.3e (gate %.0e) loss %.3e (gate %.0e) grad %.3e %s (gate %.0e) bn %.3e (gate %.0e)"
          % (name, s, err, TOL_LOGIT, abs(loss - ref_loss), TOL_LOSS, rows[0][0], rows[0][1], TOL_GRAD, worst_bn, TOL_BN))
    _write_report(name, report)
    assert err <= TOL_LOGIT, (s, err)
    assert abs(loss - ref_loss) < TOL_LOSS, (s, loss, ref_loss)
    assert rows[0][0] < TOL_GRAD, (s, rows[:5])
    assert worst_bn < TOL_BN, (s, worst_bn)
    for k, v in bo.items():
        if not v.dtype.is_floating_point:
            assert int(bp[prefix + k].item()) == int(v.item()), (s, k)


def _same_bits(s, preds, preds_twin, model, twin, step, step_twin, loss_key):
    for k in preds:
        assert torch.equal(preds[k], preds_twin[k]), (s, k)
    gt = dict(twin.named_parameters())
    for n, p in model.named_parameters():
        assert (p.grad is None) == (gt[n].grad is None), (s, n)
        if p.grad is not None:
            assert torch.equal(p.grad, gt[n].grad), (s, n)
    assert torch.equal(step.last[loss_key], step_twin.last[loss_key])


def test_lidarseg_three_steps_against_the_float64_oracle_and_a_twin_without_prefetch():
    from fusiontransformer_amd.config import lidar_cfg
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.models import _fusion_common
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    from oracle import ft_oracle as O

    cfg = lidar_cfg()
    torch.manual_seed(41)
    model, metric = build_model(cfg)
    twin, _ = build_model(cfg)
    twin.load_state_dict(model.state_dict())
    model, twin = model.cuda().train(), twin.cuda().train()
    step, step_twin = TrainStep(cfg, model, metrics=metric), TrainStep(cfg, twin)
    assert step.mode == "lidar" and step.fused_loss and type(step.optimizer).__module__.endswith("optim"), \
        "the single-head loss kernel and the one-launch Adam are expected"

    oracle = O.Net3DSegLate(20, False, dict(cfg.MODEL)).double().train()
    cw = torch.tensor(cfg.TRAIN.CLASS_WEIGHTS).double()
    batches = [make_batch([0, 1]), make_batch([2, 3])]            # whole frames, no point cap
    assert all(b["coords"].shape[0] > 32000 for b in batches)
    started = []
    real_prepare = model.backbone.prepare
    model.backbone.prepare = lambda x, **kw: started.append(x) or real_prepare(x, **kw)

    report = []
    for s, which in enumerate((0, 1, 0)):
        b = batches[which]
        pin, pin_twin, pin_next = product_inputs(b), product_inputs(b), product_inputs(batches[1 - which])
        if s > 0:
            pin = nxt                      # the batch whose index build was started during the previous step
        masks = _masks(b["coords"], 50 + s)
        pre = _snapshot(model)
        for m in (model, twin):
            m.backbone.dropout_masks = {k: v.float().cuda() for k, v in masks.items()}
        preds = step(pin, next_batch=pin_next)
        nxt = pin_next
        preds_twin = step_twin(pin_twin)
        torch.cuda.synchronize()
        if s < 2:      # (after two polls in a row that ran out the step pauses its prefetch: TrainStep.__call__)
            assert len(started) == s + 1 and started[-1] is pin_next["lidar"], "the index prefetch of the next batch did not start"
        assert set(step.last) == {"loss_3d"}
        _same_bits(s, preds, preds_twin, model, twin, step, step_twin, "loss_3d")

        oracle.load_state_dict({k: (v.double() if v.dtype.is_floating_point else v) for k, v in pre.items()})
        oracle.train()
        oracle.zero_grad(set_to_none=True)
        oracle.backbone.dropout_masks = masks
        ref = oracle(O.SparseTensor(torch.from_numpy(b["feats"]).double(), b["coords"]))
        ref_loss = F.cross_entropy(ref["lidar_seg_logit"], torch.from_numpy(b["seg_label"]).long(), weight=cw)
        ref_loss.backward()
        _judge("LidarSeg", s, which, b, model, step, "loss_3d", preds["lidar_seg_logit"], ref["lidar_seg_logit"], ref_loss.item(), oracle, "", report)

    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), n
    assert int(metric.mat.sum().item()) > 0


def test_imagesegbilinear_three_steps_against_the_float64_oracle_and_the_eager_twin():
    from fusiontransformer_amd.config import image_cfg
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    from oracle import ft_oracle as O

    cfg = image_cfg()                    # depth 12, late tap 11
    torch.manual_seed(43)
    model, metric = build_model(cfg)
    twin, _ = build_model(cfg)
    twin.load_state_dict(model.state_dict())
    model, twin = model.cuda().train(), twin.cuda().train()
    trunk = model.image_backbone.backbone
    assert len(trunk.blocks) == 12 and trunk.graph_taps == [11], "the graphed trunk is expected to be the default in training"
    twin.image_backbone.backbone.use_graphs = False     # eager trunk, same segment structure
    step, step_twin = TrainStep(cfg, model, metrics=metric), TrainStep(cfg, twin)
    assert step.mode == "image" and step.fused_loss and type(step.optimizer).__module__.endswith("optim")

    oracle = O.Net2DBillinear(20, False, dict(cfg.MODEL)).double().train()
    cw = torch.tensor(cfg.TRAIN.CLASS_WEIGHTS).double()
    batches = [make_batch([0, 1]), make_batch([2, 3])]
    pins = [product_inputs(b) for b in batches]
    prefix = "image_backbone."

    report = []
    for s, which in enumerate((0, 1, 0)):
        b, pin = batches[which], pins[which]
        pre = _snapshot(model)
        preds = step(pin, next_batch=pins[1 - which])       # ignored: there is no index to build ahead
        preds_twin = step_twin(pin)
        torch.cuda.synchronize()
        assert getattr(pins[1 - which]["lidar"], "prepared", None) is None
        assert set(step.last) == {"loss_2d"}
        _same_bits(s, preds, preds_twin, model, twin, step, step_twin, "loss_2d")

        oracle.load_state_dict({k[len(prefix):]: (v.double() if v.dtype.is_floating_point else v) for k, v in pre.items()})
        oracle.train()
        oracle.zero_grad(set_to_none=True)
        ref = oracle(torch.from_numpy(b["img"]).double(), b["img_indices"])
        ref_loss = F.cross_entropy(ref["img_seg_logit"], torch.from_numpy(b["seg_label"]).long(), weight=cw)
        ref_loss.backward()
        _judge("ImageSegBilinear", s, which, b, model, step, "loss_2d", preds["img_seg_logit"], ref["img_seg_logit"], ref_loss.item(), oracle,
               prefix, report)

    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), n
    cache = trunk.__dict__.get("_graph_cache")
    assert cache and all(v is not None for v in cache.values()), "the trunk did not run as HIP graphs"
    assert int(metric.mat.sum().item()) > 0
