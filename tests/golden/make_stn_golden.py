"""Writes tests/golden/stn.npz: the reference's own `SpatialTransformer` and `ScaleUpModule` (models/transformers.py:102-156) run in
float64 on the CPU with seeded, non-identity parameters.

  st_*   SpatialTransformer(3) on (2, 3, 40, 52) -> 24 x 24
  su_*   ScaleUpModule(16, 8, 4, 4) on (2, 16, 6, 6) -> (8, 30, 44), and the rows 200 picked points take out of that map as the
         reference's get_img_feats picks them (models/image_models_stn.py:91-98)
Stored per case: parameter names (in state_dict order) and arrays (parameters, inputs and g are float32-representable), outputs,
and the gradients of a seeded linear functional sum(out * g) with respect to every parameter and the input.  The closed-form
restatement the tests use (tests/stn_ref.py) is checked against the reference here too.

The reference's transformers.py imports `timm` only to subclass / register the ViT; empty placeholder modules carrying no arithmetic
satisfy those import lines (as in make_golden.py), the two classes exercised here are pure torch.

`PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_stn_golden.py` from the repository root."""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
from tests import stn_ref as R  # noqa: E402


def _placeholder_timm():
    """Import-line placeholders only: no arithmetic, never called by the code under test."""
    timm = types.ModuleType("timm")
    models = types.ModuleType("timm.models")
    helpers = types.ModuleType("timm.models.helpers")
    vt = types.ModuleType("timm.models.vision_transformer")
    registry = types.ModuleType("timm.models.registry")
    helpers.overlay_external_default_cfg = lambda *a, **k: None
    vt.VisionTransformer = type("VisionTransformer", (torch.nn.Module,), {})
    vt.default_cfgs, vt.build_model_with_cfg, vt.checkpoint_filter_fn = {}, None, None
    registry.register_model = lambda f: f
    timm.models = models
    for name, mod in [("timm", timm), ("timm.models", models), ("timm.models.helpers", helpers),
                      ("timm.models.vision_transformer", vt), ("timm.models.registry", registry)]:
        sys.modules[name] = mod


def _seed_parameters(module, gen):
    """Non-identity parameters: every tensor redrawn, the regressor's last layer a perturbed identity so the samples stay mostly inside."""
    with torch.no_grad():
        for name, p in module.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen, dtype=p.dtype) * (0.3 / max(1, p[0].numel()) ** 0.5))
        for name, p in module.named_parameters():
            if name.endswith("fc_loc.2.bias"):
                p.add_(torch.tensor([1.1, 0.15, 0.05, -0.1, 0.9, -0.08], dtype=p.dtype))
        for p in module.parameters():
            p.copy_(p.float().double())     # float32-representable: stored at half the size, loaded exactly by a float32 module


def _store(out, tag, module, tensors):
    names = [n for n, _ in module.named_parameters()]
    out[tag + "_names"] = np.array(names)
    for n, p in module.named_parameters():
        out["%s_param_%s" % (tag, n)] = p.detach().numpy().astype(np.float32)
        out["%s_grad_%s" % (tag, n)] = p.grad.numpy()
    for k, v in tensors.items():
        out["%s_%s" % (tag, k)] = v.detach().numpy() if torch.is_tensor(v) else v


def main():
    _placeholder_timm()
    from FusionTransformer.models.transformers import ScaleUpModule, SpatialTransformer
    gen = torch.Generator().manual_seed(20261018)
    out = {}

    st = SpatialTransformer(3).double()
    _seed_parameters(st, gen)
    x = torch.randn((2, 3, 40, 52), generator=gen, dtype=torch.float32).double().requires_grad_(True)
    g = torch.randn((2, 3, 24, 24), generator=gen, dtype=torch.float32).double() / 256   # gradients of order 1
    y = st(x, (3, 24, 24))
    (y * g).sum().backward()
    params = {n: p.detach() for n, p in st.named_parameters()}
    assert (R.spatial_transformer(params, "", x.detach(), (24, 24)) - y).abs().max().item() < 1e-12
    # d/d theta jumps where a source coordinate is an integer: the case must not sit on such a kink (float32 coordinates of these
    # sources are good to ~1e-5 px)
    th = R.theta_of(params, "", x.detach())
    assert R.kink_distance(th, *R.dense_pixels(2, 24, 24), 24, 24, 40, 52).min().item() >= 1e-4
    _store(out, "st", st, {"x": x, "g": g, "y": y, "grad_x": x.grad, "theta": R.theta_of(params, "", x.detach())})

    su = ScaleUpModule(16, 8, 4, 4).double()
    _seed_parameters(su, gen)
    H, W, n = 30, 44, 200
    x = torch.randn((2, 16, 6, 6), generator=gen, dtype=torch.float32).double().requires_grad_(True)
    idx = torch.stack([torch.randint(0, H, (n,), generator=gen), torch.randint(0, W, (n,), generator=gen)], 1)
    idx[7] = idx[3]                                        # a duplicate pixel
    counts = [120, 80]                                     # points per frame, frame-major as the reference's loop concatenates them
    frame = torch.repeat_interleave(torch.arange(2), torch.tensor(counts))
    g = torch.randn((n, 8), generator=gen, dtype=torch.float32).double() / 256
    dense = su(x, (8, H, W))
    feats, first = [], 0
    for i, c in enumerate(counts):                         # the statements of image_models_stn.py:91-98
        img_indices_i = idx[first:first + c]
        feats.append(dense.permute(0, 2, 3, 1)[i][img_indices_i[:, 0], img_indices_i[:, 1]])
        first += c
    feats = torch.cat(feats, 0)
    (feats * g).sum().backward()
    params = {n_: p.detach() for n_, p in su.named_parameters()}
    assert (R.scale_up(params, "", x.detach(), (H, W), 4) - dense).abs().max().item() < 1e-12
    assert (R.scale_up_points(params, "", x.detach(), idx, frame, H, W, 4) - feats).abs().max().item() < 1e-12
    m = R.up_conv(params, "", x.detach(), 4)
    th = R.theta_of(params, "up_stn.", m)
    assert R.kink_distance(th, frame, idx[:, 0], idx[:, 1], H, W, 24, 24).min().item() >= 1e-4
    _store(out, "su", su, {"x": x, "g": g, "dense": dense, "feats": feats, "grad_x": x.grad, "idx": idx.numpy().astype(np.int64),
                           "frame": frame.numpy().astype(np.int32), "size": np.array([H, W], dtype=np.int32)})

    path = os.path.join(ROOT, "tests", "golden", "stn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, torch", torch.__version__)


if __name__ == "__main__":
    main()
