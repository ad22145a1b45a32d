"""The gradient reducer under the single-modality train steps, on ONE GPU over the real backend (pattern of
tests/test_dist_gpu.py): one fresh child process, a one-rank RCCL communicator, all-reduces issued from the post-accumulate hooks.
An all-reduce over one rank is the identity, so LidarSeg and ImageSegBilinear (DUAL_HEAD=True: its second head is frozen, the
reducer must not wait for a gradient that never comes) must end three steps with gradients and parameters bit-identical to a twin
stepped without a reducer, and every trainable parameter must have received a gradient.  The parent process does not touch the
GPU."""
import os
import socket

import pytest

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(port, q):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        from fusiontransformer_amd.config import image_cfg, lidar_cfg
        from fusiontransformer_amd.data.synth import make_batch
        from fusiontransformer_amd.dist import GradReducer, init_process_group
        from fusiontransformer_amd.models.build import build_model
        from fusiontransformer_amd.trainer import TrainStep
        from tests.helpers import product_inputs, small_cfg
        init_process_group("nccl", force=True)
        assert dist.is_initialized() and dist.get_backend() == "nccl" and dist.get_world_size() == 1
        small = small_cfg("late")          # depth-2 trunk, late tap 1
        out = {}
        for name, cfg in (("LidarSeg", lidar_cfg()), ("ImageSegBilinear", image_cfg())):
            if name == "ImageSegBilinear":
                cfg.MODEL.DUAL_HEAD = True
                cfg.MODEL.vit_depth, cfg.MODEL.late_feat_block_number = small.MODEL.vit_depth, small.MODEL.late_feat_block_number
            torch.manual_seed(5)
            model, _ = build_model(cfg)
            twin, _ = build_model(cfg)
            twin.load_state_dict(model.state_dict())
            model, twin = model.cuda().train(), twin.cuda().train()
            red = GradReducer(model, bucket_mb=8.0, force_collectives=True)
            assert red.active
            step, step_twin = TrainStep(cfg, model, grad_reducer=red), TrainStep(cfg, twin)
            assert step.mode == ("lidar" if name == "LidarSeg" else "image") and step.fused_loss
            same_grads, all_received, missing = True, True, []
            for s in range(3):
                pin = product_inputs(make_batch([30 + 2 * s, 31 + 2 * s], max_points=1800))
                torch.manual_seed(9 + s)
                step(pin)
                torch.manual_seed(9 + s)
                step_twin(pin)
                torch.cuda.synchronize()
                for (n, p), (_, t) in zip(model.named_parameters(), twin.named_parameters()):
                    if p.requires_grad:
                        if t.grad is None or p.grad is None:
                            all_received = False
                            missing.append(n)
                        else:
                            same_grads = same_grads and torch.equal(p.grad, t.grad)
            same_params = all(torch.equal(p, t) for p, t in zip(model.parameters(), twin.parameters()))
            frozen_head = name != "ImageSegBilinear" or not any(p.requires_grad for p in model.image_backbone.linear2.parameters())
            out[name] = (same_grads, same_params, all_received, missing[:8], frozen_head, len(red.buckets))
        q.put(("ok", out))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put(("error", traceback.format_exc()))
        raise


def test_one_rank_rccl_reducer_is_the_identity_for_the_single_modality_steps():
    import multiprocessing as mp
    ctx = mp.get_context("forkserver")
    q = ctx.Queue()
    p = ctx.Process(target=_worker, args=(_free_port(), q))
    p.start()
    status, out = q.get(timeout=600)
    p.join(timeout=120)
    assert status == "ok", out
    assert set(out) == {"LidarSeg", "ImageSegBilinear"}
    for name, (same_grads, same_params, all_received, missing, frozen_head, nb) in out.items():
        assert all_received, (name, "trainable parameters without a gradient", missing)
        assert same_grads, (name, "gradients after the one-rank RCCL all-reduce differ from the local ones")
        assert same_params, (name, "parameters after three steps differ from the twin without a reducer")
        assert frozen_head and nb >= 1, (name, frozen_head, nb)
    assert p.exitcode == 0
