"""Train-mode parity of the workload bench.py times: whole SemanticKITTI-shaped frames, the full 12-block DeiT trunk replayed
as four HIP-graph segments, image / LiDAR branches on two HIP streams, train-mode BatchNorm, the fused loss kernel and the
one-launch Adam, three steps over two ALTERNATING batches (reference: modules/SemanticTrainer.py:141-209 around
models/middle_fusion.py:100-112).

Every step is checked against the CPU oracle run in float64 from the SAME pre-step state (parameters and BatchNorm buffers
are copied to the oracle before each step, so step 2 and 3 -- the graph REPLAYS -- are judged on their own and not through
the noise Adam's sign-like first updates put on near-zero gradients): per-point logits within 1e-3, both losses within
1e-4, BatchNorm running statistics, every parameter gradient.  The same three steps also run on a twin model with the eager
trunk and serial branch issue: logits, gradients and the parameters after the third Adam step must agree bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from tests.helpers import oracle_inputs, product_inputs

pytestmark = pytest.mark.gpu
TOL_LOGIT, TOL_LOSS = 1e-3, 1e-4
# worst per-parameter L2-relative gradient error against float64 measured on MI355X for this workload (profiles/r03_grad_parity_fullsize.json):
# 1.9e-3, 3.2e-3, 1.1e-3 over the three steps (BatchNorm biases of the deep levels; 36-46 k points average the rounding noise down
# from the 5e-3 .. 1.5e-2 of the 2-3 k-point tests); the bound is 3x the worst measured.  A wrong or missing term, or a replay that
# reads a stale buffer, shows up as O(1)
TOL_GRAD = 1e-2


def _level_rows(coords, stride):
    c = np.concatenate([coords[:, :3] // stride, coords[:, 3:]], 1)
    return len(np.unique(c, axis=0))


def _masks(coords, seed):
    g = torch.Generator().manual_seed(seed)
    return {"y1": (torch.rand(_level_rows(coords, 16), 256, generator=g) > 0.3).double(),
            "y3": (torch.rand(_level_rows(coords, 4), 128, generator=g) > 0.3).double()}


def _snapshot(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}


def test_three_bench_steps_against_the_float64_oracle_and_the_eager_twin():
    from fusiontransformer_amd.config import fusion_cfg
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    from oracle import ft_oracle as O

    cfg = fusion_cfg("middle")           # depth 12, taps 5 / 11, dual head: configs/semantic_kitti/middlefusion.yaml
    torch.manual_seed(31)
    model, _, _ = build_model(cfg)
    twin, _, _ = build_model(cfg)
    twin.load_state_dict(model.state_dict())
    model, twin = model.cuda().train(), twin.cuda().train()
    trunk = model.image_backbone.backbone
    assert trunk.graph_taps, "the graphed trunk is expected to be the default in training"
    twin.image_backbone.backbone.use_graphs = False     # eager trunk, same segment structure
    model.overlap_branches, twin.overlap_branches = True, False
    step, step_twin = TrainStep(cfg, model), TrainStep(cfg, twin)
    assert step.fused_loss and type(step.optimizer).__module__.endswith("optim"), "bench.py's loss kernel and one-launch Adam are expected"

    oracle = O.build_model(dict(cfg.MODEL)).double().train()
    cw = torch.tensor(cfg.TRAIN.CLASS_WEIGHTS).double()
    batches = [make_batch([0, 1]), make_batch([2, 3])]            # whole frames, no point cap
    assert all(b["coords"].shape[0] > 32000 for b in batches)      # 45 523 and 35 714 points
    assert batches[0]["coords"].shape[0] != batches[1]["coords"].shape[0]
    pins = [product_inputs(b) for b in batches]

    report = []
    for s, which in enumerate((0, 1, 0)):
        b, pin = batches[which], pins[which]
        masks = _masks(b["coords"], 50 + s)
        pre = _snapshot(model)
        for m in (model, twin):
            m.lidar_backbone.dropout_masks = {k: v.float().cuda() for k, v in masks.items()}
        preds = step(pin)
        preds_twin = step_twin(pin)
        torch.cuda.synchronize()

        # ---- the eager, serially issued twin: bit for bit
        for k in preds:
            assert torch.equal(preds[k], preds_twin[k]), (s, k)
        gm, gt = dict(model.named_parameters()), dict(twin.named_parameters())
        for n, p in gm.items():
            assert (p.grad is None) == (gt[n].grad is None), (s, n)
            if p.grad is not None:
                assert torch.equal(p.grad, gt[n].grad), (s, n)
        assert torch.equal(step.last["loss_2d"], step_twin.last["loss_2d"]) and torch.equal(step.last["loss_3d"], step_twin.last["loss_3d"])

        # ---- the float64 oracle from the same pre-step state
        oracle.load_state_dict({k: (v.double() if v.dtype.is_floating_point else v) for k, v in pre.items()})
        oracle.train()
        oracle.zero_grad(set_to_none=True)
        oracle.lidar_backbone.dropout_masks = masks
        i64 = oracle_inputs(b)
        i64["img"], i64["lidar"].F = i64["img"].double(), i64["lidar"].F.double()
        ref = oracle(i64)
        a, c = O.fusion_losses(ref, torch.from_numpy(b["seg_label"]), cw, 0.1, True)
        (a + c).backward()
        worst_logit = 0.0
        for k in ref:
            err = (preds[k].detach().cpu().double() - ref[k].detach()).abs().max().item()
            worst_logit = max(worst_logit, err)
            assert err <= TOL_LOGIT, (s, k, err)
        l2, l3 = step.last["loss_2d"].item(), step.last["loss_3d"].item()
        assert abs(l2 - a.item()) < TOL_LOSS and abs(l3 - c.item()) < TOL_LOSS, (s, l2, a.item(), l3, c.item())
        p64 = dict(oracle.named_parameters())
        gmax = max(p.grad.abs().max().item() for p in p64.values() if p.grad is not None)
        rows = []
        for name, p in p64.items():
            if p.grad is None:
                assert gm[name].grad is None or gm[name].grad.abs().max().item() == 0, (s, name)
                continue
            assert gm[name].grad is not None, (s, name)
            gp = gm[name].grad.cpu().double()
            floor = 1e-4 * gmax * p.numel() ** 0.5       # gradients that are 0 in exact arithmetic (Linear biases in front of a BatchNorm) are rounding noise
            rows.append(((gp - p.grad).norm().item() / max(p.grad.norm().item(), floor), name))
        rows.sort(reverse=True)
        report.append({"step": s, "batch": which, "points": int(b["coords"].shape[0]), "worst_logit_err": worst_logit,
                       "loss_2d": l2, "loss_3d": l3, "oracle_loss_2d": a.item(), "oracle_loss_3d": c.item(), "worst_grad_rel_l2": rows[:8]})
        if os.environ.get("FTX_TEST_REPORT_DIR"):    # optional diagnostic, written where the caller asks
            os.makedirs(os.environ["FTX_TEST_REPORT_DIR"], exist_ok=True)
            json.dump(report, open(os.path.join(os.environ["FTX_TEST_REPORT_DIR"], "grad_parity_fullsize.json"), "w"), indent=1)
        assert rows[0][0] < TOL_GRAD, (s, rows[:5])
        # BatchNorm running statistics after this step's forward (the buffers are not touched by Adam)
        bo, bp = dict(oracle.named_buffers()), dict(model.named_buffers())
        for name, buf in bo.items():
            if buf.dtype.is_floating_point:
                assert (bp[name].cpu().double() - buf).abs().max().item() < 1e-4, (s, name)
            else:
                assert int(bp[name].item()) == int(buf.item()), (s, name)

    # after three Adam steps the graphed two-stream model and the eager serial twin hold the same bits
    for (n, p), (_, q) in zip(model.named_parameters(), twin.named_parameters()):
        assert torch.equal(p, q), n
    cache = trunk.__dict__.get("_graph_cache")
    assert cache and all(v is not None for v in cache.values()), "the trunk did not run as HIP graphs"
    assert all(len(v) == 4 for v in cache.values()), "12 blocks with taps 5 / 11 are expected to be four graph segments"


def test_nuscenes_shaped_batch_of_four_in_eval_mode():
    """BASELINE configs[2] at its stated batch: four 900x1600 / ~27 k-point frames through the full model, eval mode, against the
    oracle (per-point logits within 1e-3)."""
    from fusiontransformer_amd.config import fusion_cfg
    from fusiontransformer_amd.data.synth import SHAPES, make_batch
    from fusiontransformer_amd.models.build import build_model
    from oracle import ft_oracle as O
    hw = (SHAPES["nuscenes"]["H"], SHAPES["nuscenes"]["W"])
    cfg = fusion_cfg("middle")
    cfg.MODEL.lift_size = hw
    torch.manual_seed(8)
    oracle = O.build_model(dict(cfg.MODEL)).eval()
    model, _, _ = build_model(cfg)
    model.load_state_dict(oracle.state_dict())
    model = model.cuda().eval()
    batch = make_batch([10, 11, 12, 13], shape="nuscenes")
    assert batch["coords"].shape[0] > 90000 and batch["img"].shape == (4, 3) + hw
    with torch.no_grad():
        ref = oracle(oracle_inputs(batch))
        out = model(product_inputs(batch))
    for k in ref:
        err = (out[k].cpu() - ref[k]).abs().max().item()
        assert err <= TOL_LOGIT, (k, err)
    lo, lp = oracle.lidar_backbone.last_index, model.lidar_backbone.last_index
    for lvl in ("x0", "x1", "x2", "x3", "x4"):
        assert np.array_equal(lp[lvl].C.cpu().numpy(), lo[lvl].C), lvl
