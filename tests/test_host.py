"""Host logic that needs no GPU: config loader, model factory / state_dict naming, synthetic
generator, collate, and the refusal to run the product path without the GPU."""
import os

import numpy as np
import pytest
import torch

from fusiontransformer_amd.config import CfgNode, fusion_cfg, get_cfg_defaults
from tests.helpers import small_cfg


def test_config_loads_reference_style_yaml(tmp_path):
    y = tmp_path / "middlefusion.yaml"
    y.write_text("MODEL:\n  TYPE: \"MiddleFusionTransformer\"\n  DUAL_HEAD: True\n  NUM_CLASSES: 20\n  middle_feat_block_number: 5\n"
                 "  late_feat_block_number: 11\n  USE_IMAGE: True\n  USE_LIDAR: True\n  USE_FUSION: True\nOPTIMIZER:\n  TYPE: \"Adam\"\n"
                 "  BASE_LR: 1e-4\n  WEIGHT_DECAY: 0.0005\nTRAIN:\n  BATCH_SIZE: 10\n  FusionTransformer:\n    lambda_xm: 0.1\n")
    cfg = get_cfg_defaults()
    cfg.merge_from_file(str(y))
    cfg.merge_from_list(["TRAIN.BATCH_SIZE", "4"])
    assert cfg.MODEL.TYPE == "MiddleFusionTransformer" and cfg.MODEL.middle_feat_block_number == 5
    assert cfg.TRAIN.BATCH_SIZE == 4 and cfg.TRAIN.FusionTransformer.lambda_xm == 0.1
    assert dict(**cfg.MODEL)["NUM_CLASSES"] == 20 and cfg.MODEL.get("cr", 1.0) == 1.0   # SPVCNN(**cfg.MODEL) contract
    ref = fusion_cfg("middle")
    assert ref.MODEL.TYPE == cfg.MODEL.TYPE and len(ref.TRAIN.CLASS_WEIGHTS) == 20 and ref.TRAIN.CLASS_WEIGHTS[0] == 0.0


@pytest.mark.parametrize("kind,cls", [("middle", "MiddleFusionTransformer"), ("early", "EarlyFusionTransformer"), ("late", "LateFusionTransformer")])
def test_build_model_dispatch_and_state_dict_names(kind, cls):
    from fusiontransformer_amd.models.build import build_model
    from oracle import ft_oracle as O
    cfg = small_cfg(kind)
    model, m2d, m3d = build_model(cfg)
    assert type(model).__name__ == cls and m2d.name == "seg_iou_2d" and m3d.name == "seg_iou_3d"
    oracle = O.build_model(dict(cfg.MODEL))
    sd, so = model.state_dict(), oracle.state_dict()
    assert set(sd) == set(so)
    assert all(sd[k].shape == so[k].shape for k in sd)
    names = set(sd)
    prefix = "lidar_backbone.backbone." if kind == "late" else "lidar_backbone."
    for k in ("stem.0.kernel", "stage1.1.net.1.running_mean", "up1.0.net.0.kernel", "point_transforms.0.0.weight"):
        assert prefix + k in names, k
    for k in ("image_backbone.backbone.blocks.0.attn.qkv.weight", "image_backbone.sample_down.stem.0.weight", "image_backbone.linear.weight"):
        assert k in names, k
    # strided 2^3 conv: (8, inc, inc); the residual shortcut exists only where the channel count changes (spvcnn.py:66-72)
    assert sd[prefix + "stage1.0.net.0.kernel"].shape == (8, 32, 32)
    assert prefix + "stage1.1.downsample.0.kernel" not in names
    assert sd[prefix + "stage2.1.downsample.0.kernel"].shape == (32, 64)
    assert sd[prefix + "up1.1.0.net.0.kernel"].shape == (27, 256 + 128, 256)
    # parameters that never get a gradient are frozen (DDP without find_unused_parameters)
    assert not any(p.requires_grad for p in model.image_backbone.backbone.norm.parameters())
    if kind in ("middle", "early"):   # the fused tap reaches the LiDAR branch detached: its lift module never gets a gradient
        assert not any(p.requires_grad for p in model.image_backbone.up["0"].parameters())
    assert all(p.requires_grad for p in model.image_backbone.up[str(cfg.MODEL.late_feat_block_number)].parameters())


def test_build_model_lidar_and_image_only_and_errors():
    from fusiontransformer_amd.models.build import build_model
    cfg = small_cfg("middle")
    cfg.MODEL.USE_FUSION, cfg.MODEL.USE_IMAGE, cfg.MODEL.TYPE = False, False, "LidarSeg"
    m, met = build_model(cfg)
    assert type(m).__name__ == "LidarSeg"
    cfg.MODEL.USE_LIDAR, cfg.MODEL.USE_IMAGE, cfg.MODEL.TYPE = False, True, "ImageSegBilinear"
    m, met = build_model(cfg)
    assert type(m).__name__ == "ImageSegBilinear"
    cfg.MODEL.TYPE = "ImageSeg"
    with pytest.raises(NotImplementedError):
        build_model(cfg)


def test_synthetic_frames_are_deterministic_and_well_formed():
    from fusiontransformer_amd.data.synth import make_batch, make_frame
    a, b = make_frame(3), make_frame(3)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert 8000 < a["coords"].shape[0] < 40000 and a["img"].shape == (3, 370, 1226)
    assert a["img_indices"][:, 0].max() < 370 and a["img_indices"][:, 1].max() < 1226 and a["img_indices"].min() >= 0
    assert len(np.unique(a["coords"], axis=0)) == len(a["coords"])          # deduped: one point per voxel
    assert a["coords"].min() >= 0 and a["coords"].max() < 4096
    batch = make_batch([0, 1], max_points=500)
    assert batch["coords"].shape == (1000, 4) and set(batch["coords"][:, 3]) == {0, 1} and len(batch["img_indices"]) == 2
    n = make_frame(0, "nuscenes")
    assert n["img"].shape == (3, 900, 1600)


def test_collate_matches_reference_layout():
    from fusiontransformer_amd.data.collate import get_collate_scn
    from fusiontransformer_amd.data.synth import make_frame
    frames = [make_frame(i, max_points=300) for i in range(2)]
    out = get_collate_scn(True)(frames)
    assert out["lidar"].C.shape == (600, 4) and out["lidar"].C[:, 3].tolist() == [0] * 300 + [1] * 300
    assert out["lidar"].F.shape == (600, 4) and out["seg_label"].shape == (600,) and out["img"].shape == (2, 3, 370, 1226)
    assert len(out["img_indices"]) == 2 and out["img_indices"][0].shape == (300, 2)


def test_product_path_refuses_cpu_tensors():
    from fusiontransformer_amd import functional as spf
    with pytest.raises(ValueError, match="no CPU fallback"):
        spf.sphash(torch.zeros((4, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        spf.spvoxelize(torch.zeros(4, 4), torch.zeros(4, dtype=torch.int32), torch.ones(2, dtype=torch.int32))


def test_scan_file_round_trip_and_untrusted_pickles_are_refused(tmp_path):
    """The reference's per-scan pickle (preprocess.py:150-163) reads back; anything else in a .pkl is refused."""
    import pickle
    from fusiontransformer_amd.data.preprocess import read_scan, write_scan
    rng = np.random.default_rng(0)
    scan = {"points": rng.standard_normal((50, 3)).astype(np.float32), "feats": rng.standard_normal((50, 4)).astype(np.float32),
            "seg_labels": rng.integers(0, 20, 50).astype(np.int16), "points_img": rng.uniform(0, 300, (50, 2)).astype(np.float32),
            "lidar_path": "sequences/08/velodyne/000000.bin", "camera_path": "sequences/08/image_2/000000.png", "image_size": (1226, 370)}
    p = tmp_path / "0.pkl"
    write_scan(p, scan)
    back = read_scan(p)
    for k in ("points", "feats", "seg_labels", "points_img"):
        assert back[k].dtype == scan[k].dtype and np.array_equal(back[k], scan[k])
    assert back["image_size"] == (1226, 370) and back["lidar_path"] == scan["lidar_path"]
    with open(p, "rb") as f:                          # a file written the reference's way (plain pickle.dump) is the same bytes
        assert pickle.load(f).keys() == back.keys()
    evil = tmp_path / "evil.pkl"
    with open(evil, "wb") as f:
        pickle.dump({"points": print}, f)            # a global that is not a numpy constructor
    with pytest.raises(pickle.UnpicklingError):
        read_scan(evil)
    bad = tmp_path / "bad.pkl"
    write_scan(bad, dict(scan, points=scan["points"][:10]))
    with pytest.raises(ValueError):
        read_scan(bad)


def test_adam_on_cpu_parameters_is_torch_adam():
    """fusiontransformer_amd.optim.Adam hands anything its kernel does not cover (here: CPU parameters) to torch.optim.Adam.step, and
    keeps torch's state_dict layout."""
    import torch
    from fusiontransformer_amd.optim import Adam
    torch.manual_seed(0)
    a = [torch.nn.Parameter(torch.randn(7, 3)), torch.nn.Parameter(torch.randn(5))]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oa, ob = Adam(a, lr=1e-2, weight_decay=1e-3), torch.optim.Adam(b, lr=1e-2, weight_decay=1e-3)
    for _ in range(3):
        for p, q in zip(a, b):
            g = torch.randn_like(p)
            p.grad, q.grad = g.clone(), g.clone()
        oa.step(); ob.step()
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa["state"].keys() == sb["state"].keys()
    for k in sa["state"]:
        assert sa["state"][k].keys() == sb["state"][k].keys()
        assert float(sa["state"][k]["step"]) == float(sb["state"][k]["step"]) == 3.0


def test_prepare_batch_is_a_no_op_off_the_gpu():
    """prepare_batch / SPVCNN.prepare build coordinate structures ahead only for device tensors; a CPU batch passes through untouched
    (the forward would fail loudly later: the product has no CPU path)."""
    import torch
    from fusiontransformer_amd.models._fusion_common import prepare_batch
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.sparse import SparseTensor
    from tests.helpers import small_cfg
    model, _, _ = build_model(small_cfg("middle"))
    lidar = SparseTensor(torch.zeros(4, 4), torch.zeros(4, 4, dtype=torch.int32))
    d = {"lidar": lidar}
    assert prepare_batch(model, d) is d and lidar.prepared is None


def test_bench_self_launch_command_is_the_drivers_launcher_line():
    """`python bench.py --gpus N` without WORLD_SIZE becomes the launcher itself: children under torch.distributed.run, one per GPU,
    rendezvous on 127.0.0.1 (the reference: torchpack_run.sh:3 `torchpack dist-run -np N python train.py ...`)."""
    import bench
    cmd = bench.launch_command(4, ["--gpus", "4", "--steps", "3", "--warmup", "1"], port=29511)
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29511"
    i = cmd.index(os.path.abspath(bench.__file__))
    assert cmd[i + 1:] == ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    auto = bench.launch_command(2, [])
    assert 1024 < int(auto[auto.index("--master-port") + 1]) < 65536


def test_bench_dump_outputs_is_bounded_and_repeatable(tmp_path, monkeypatch):
    """--dump-outputs: one float .npy per array; the parameter / gradient sample sits at the same positions in every run; over the
    size budget, large arrays are cut to a seeded sample of rows and the whole stays within it."""
    import bench
    torch.manual_seed(0)
    m = torch.nn.Linear(64, 32)
    m(torch.randn(4, 64)).sum().backward()
    preds = {"lidar_seg_logit": torch.randn(5000, 20), "img_seg_logit": torch.randn(5000, 20)}
    losses = {"loss_2d": torch.tensor(1.5), "loss_3d": torch.tensor(2.5)}
    a, b = bench.capture_outputs(preds, losses, m), bench.capture_outputs(preds, losses, m)
    assert set(a) == {"lidar_seg_logit", "img_seg_logit", "loss_2d", "loss_3d", "param_sample", "grad_sample"}
    assert all(torch.equal(a[k], b[k]) for k in a)
    bench.dump_outputs(a, str(tmp_path / "whole"))
    for k, v in a.items():
        arr = np.load(tmp_path / "whole" / (k + ".npy"))
        assert arr.dtype == np.float32 and np.array_equal(arr, v.numpy())
    monkeypatch.setattr(bench, "DUMP_BYTES", 256 << 10)
    bench.dump_outputs(a, str(tmp_path / "cut"))
    assert sum(f.stat().st_size for f in (tmp_path / "cut").iterdir()) <= (256 << 10) + 4096     # + the .npy headers
    rows = np.load(tmp_path / "cut" / "lidar_seg_logit_rows.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "cut" / "lidar_seg_logit.npy"), a["lidar_seg_logit"].numpy()[rows])


def test_carve_refuses_to_run_under_stream_capture(monkeypatch):
    """functional._carve returns raw addresses into the stream's scratch buffer; under HIP-graph capture that buffer would be a
    fresh pool allocation freed on return, so the call must fail loudly instead."""
    from fusiontransformer_amd import functional as Fn
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        Fn._carve(torch.zeros(1), 1024, 4096)
