"""The affine-sampling kernels (csrc/ftx_stn.hip), the spatial-transformer modules and the ImageSeg model on the GPU.

Bars.  No tolerance here is a number.  The truth is the float64 closed form (tests/stn_ref.py).  The yardstick is torch's own float32
affine_grid + grid_sample on the CPU, forward and autograd, on the same inputs; bar = BAR_FACTOR x the yardstick's worst error for that
case and quantity: the kernel's closed form and torch's base-grid product order their roundings differently, so the kernel may sit a
small multiple of torch's own error away, not orders of magnitude.  Forward and grad_src: absolute error.  grad_theta: relative L2
per frame.  Where the truth is exactly 0 (every sample outside the source) the kernel's result must be exactly 0.

Kinks.  d/d theta jumps where a source coordinate is an integer, so the cases that compare grad_theta pick their inputs on the CPU
with the float64 closed form alone: dense cases draw theta by seed until every coordinate is >= 1e-3 px from an integer (sources
<= 64 px: float32 coordinates are good to ~1e-5 px), point cases reject candidate points inside the margin (4e-3 px at the 384 px
source) and assert that under 4 % of the candidates go.  Nothing that was kept is left out of a comparison.  Forward and grad_src
are continuous in the coordinate and need no selection.

With FTX_TEST_REPORT_DIR set, every measured error and its bar is written to <dir>/stn_accuracy.txt."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import stn_ref as R

pytestmark = pytest.mark.gpu
BAR_FACTOR = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stn.npz")
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    d = os.environ.get("FTX_TEST_REPORT_DIR")
    if d and REPORT:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "stn_accuracy.txt"), "w") as f:
            f.write("case | quantity | kernel error | yardstick error (torch float32 on the CPU) | bar = %d x yardstick\n" % BAR_FACTOR)
            f.write("\n".join(REPORT) + "\n")


def inside_bar(case, quantity, got, yard, truth, relative=False):
    """Prints the figures, then asserts the kernel's error against BAR_FACTOR x the yardstick's."""
    if relative:
        ek, ey = R.rel_l2_per_frame(got, truth), R.rel_l2_per_frame(yard, truth)
    else:
        ek, ey = (got.double() - truth).abs().max().item(), (yard.double() - truth).abs().max().item()
    line = "%s | %s | %.3e | %.3e | %.3e" % (case, quantity, ek, ey, BAR_FACTOR * ey)
    REPORT.append(line)
    print(line)
    if truth.abs().max().item() == 0:
        assert got.abs().max().item() == 0, (case, quantity, "the truth is exactly 0, the kernel's result is not")
    assert ek <= BAR_FACTOR * ey, line


def source(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def on_device(src, layout):
    """NCHW, or the same values with channels-last strides."""
    d = src.cuda()
    return d if layout == "nchw" else d.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------------ dense form
def run_dense(case, src, theta, size, layout, with_theta_grad):
    from fusiontransformer_amd import functional as spf
    go = source((src.shape[0], src.shape[1]) + tuple(size), 99)
    t64 = theta.double().requires_grad_(True)
    truth = R.sample(src.double(), t64, size)
    t32 = theta.clone().requires_grad_(True)
    yard = R.torch_dense(src, t32, size)
    td = theta.cuda().requires_grad_(True)
    got = spf.affine_sample(on_device(src, layout), td, size)
    assert got.shape == truth.shape and got.is_contiguous()
    inside_bar(case, "forward", got.detach().cpu(), yard.detach(), truth.detach())
    if with_theta_grad:
        (truth * go.double()).sum().backward()
        (yard * go).sum().backward()
        (got * go.cuda()).sum().backward()
        inside_bar(case, "grad_theta", td.grad.cpu(), t32.grad, t64.grad, relative=True)
    return got


DENSE_FWD = [((1, 1, 1, 1), (1, 1), "identity", "nchw"), ((2, 3, 5, 7), (7, 5), "rotate", "nchw"), ((3, 5, 23, 37), (16, 16), "scale", "nhwc"),
             ((2, 3, 48, 48), (33, 65), "flip", "nchw"), ((1, 96, 64, 33), (7, 5), "rotate", "nhwc"), ((2, 1, 64, 33), (33, 65), "scale", "nchw"),
             ((2, 5, 5, 7), (1, 1), "identity", "nhwc"), ((2, 3, 23, 37), (16, 16), "outside", "nchw"), ((3, 96, 5, 7), (16, 16), "flip", "nchw")]


@pytest.mark.parametrize("shape,size,kind,layout", DENSE_FWD)
def test_dense_forward(shape, size, kind, layout):
    run_dense("dense %s -> %s %s %s" % (shape, size, kind, layout), source(shape, 1), R.theta_case(kind, shape[0]), size, layout, False)


DENSE_THETA = [((2, 3, 48, 48), (16, 16), k, "nchw") for k in ("identity", "scale", "rotate", "flip", "outside")] + [
    ((3, 5, 23, 37), (7, 5), "rotate", "nhwc"), ((1, 96, 64, 33), (16, 16), "scale", "nhwc"), ((2, 1, 5, 7), (16, 16), "flip", "nchw"),
    ((2, 3, 1, 1), (1, 1), "rotate", "nchw"), ((3, 3, 64, 33), (7, 5), "identity", "nchw")]   # targets <= 16 x 16: a 33 x 65 target has no draw clear of every kink


@pytest.mark.parametrize("shape,size,kind,layout", DENSE_THETA)
def test_dense_theta_gradient(shape, size, kind, layout):
    theta, draws = R.draw_dense_theta(kind, shape[0], size, shape[2], shape[3], seed=7)
    run_dense("dense-theta %s -> %s %s %s (draw %d)" % (shape, size, kind, layout, draws), source(shape, 2), theta, size, layout, True)


def test_dense_full_size_forward():
    src = source((2, 3, 370, 1226), 3)
    run_dense("dense full size (2, 3, 370, 1226) -> (384, 384)", src, R.theta_case("rotate", 2, np.random.default_rng(1)), (384, 384), "nchw", False)


def test_dense_refuses_a_source_that_needs_a_gradient():
    from fusiontransformer_amd import functional as spf
    with pytest.raises(RuntimeError):
        spf.affine_sample(source((1, 3, 5, 7), 0).cuda().requires_grad_(True), R.theta_case("identity", 1).cuda(), (4, 4))


# ------------------------------------------------------------------------------------------------------------------ point form
def points(b, H, W, n, seed, theta, ih, iw, margin, empty_frame=None, extras=True):
    """n seeded points (row, col, frame) of a (b, H, W) target that are `margin` px clear of every kink of theta, frame-major like
    pack_img_indices, with a duplicate pixel; the last four (extras, n >= 8) are three out-of-range img_idx rows and one
    out-of-range frame."""
    extras = extras and n >= 8
    total, n = n, n - 4 if extras else n
    g = torch.Generator().manual_seed(seed)
    m = 2 * n + 8
    idx = torch.stack([torch.randint(0, H, (m,), generator=g), torch.randint(0, W, (m,), generator=g)], 1)
    frames = [f for f in range(b) if f != empty_frame] or [0]
    frame = torch.tensor(frames, dtype=torch.int32)[torch.randint(0, len(frames), (m,), generator=g)]
    keep, share = R.select_points(theta, idx, frame, H, W, ih, iw, margin)
    assert share > 0.96, "the margin drops %.1f %% of the candidates" % (100 * (1 - share))
    idx, frame = idx[keep][:n], frame[keep][:n]
    assert idx.shape[0] == n
    if n > 2:
        idx[n // 2] = idx[0]
        frame[n // 2] = frame[0]
    order = torch.argsort(frame, stable=True)
    idx, frame = idx[order], frame[order]
    if extras:
        idx = torch.cat([idx, torch.tensor([[-1, 0], [H, 0], [0, W], [0, 0]])])
        frame = torch.cat([frame, torch.tensor([0, 0, 0, b], dtype=torch.int32)])
    assert idx.shape[0] == total
    return idx.contiguous(), frame.contiguous()


def run_points(case, src, theta, idx, frame, H, W, layout):
    from fusiontransformer_amd import functional as spf
    n, c = idx.shape[0], src.shape[1]
    go = source((n, c), 98)
    inr = (frame >= 0) & (frame < src.shape[0])                  # the yardstick and the truth take the in-range frames; the rest are zero rows
    s64, t64 = src.double().requires_grad_(True), theta.double().requires_grad_(True)
    truth = R.sample_points(s64, t64, idx, frame, H, W)
    (truth * go.double()).sum().backward()
    s32, t32 = src.clone().requires_grad_(True), theta.clone().requires_grad_(True)
    yard = torch.zeros((n, c)).index_add(0, torch.nonzero(inr).view(-1), R.torch_points(s32, t32, idx[inr], frame[inr], H, W))
    (yard * go).sum().backward()
    sd, td = on_device(src, layout).requires_grad_(True), theta.cuda().requires_grad_(True)
    got = spf.affine_lift(sd, td, idx.cuda(), frame.cuda(), H, W)
    (got * go.cuda()).sum().backward()
    assert sd.grad.stride() == sd.stride()
    inside_bar(case, "forward", got.detach().cpu(), yard.detach(), truth.detach())
    inside_bar(case, "grad_src", sd.grad.cpu(), s32.grad if s32.grad is not None else torch.zeros_like(src), s64.grad if s64.grad is not None else torch.zeros_like(src).double())
    inside_bar(case, "grad_theta", td.grad.cpu(), t32.grad, t64.grad, relative=True)
    # out-of-range rows are exactly zero
    bad = ~(inr & (idx[:, 0] >= 0) & (idx[:, 0] < H) & (idx[:, 1] >= 0) & (idx[:, 1] < W))
    assert got.detach().cpu()[bad].abs().max().item() == 0 if bad.any() else True
    return sd, td, got


POINTS = [((1, 1, 1, 1), (4, 6), 1, "identity", "nchw", None), ((2, 3, 5, 7), (30, 44), 63, "rotate", "nchw", None),
          ((3, 5, 23, 37), (37, 50), 64, "scale", "nhwc", 1), ((2, 96, 48, 48), (40, 60), 65, "flip", "nchw", None),
          ((3, 96, 64, 33), (50, 30), 1000, "rotate", "nhwc", None), ((2, 5, 23, 37), (37, 50), 1000, "outside", "nchw", None),
          ((3, 3, 48, 48), (37, 50), 1000, "scale", "nchw", 0), ((1, 5, 64, 33), (30, 44), 65, "identity", "nhwc", None)]


@pytest.mark.parametrize("shape,size,n,kind,layout,empty", POINTS)
def test_lift_forward_and_gradients(shape, size, n, kind, layout, empty):
    theta = R.theta_case(kind, shape[0], np.random.default_rng(12))
    idx, frame = points(shape[0], size[0], size[1], n, 5, theta, shape[2], shape[3], 1e-3, empty_frame=empty)
    run_points("lift %s at %d of %s %s %s" % (shape, n, size, kind, layout), source(shape, 4), theta, idx, frame, size[0], size[1], layout)


def test_lift_full_size():
    """The model's shape: (2, 96, 384, 384) sampled at 20 000 points of 370 x 1226; forward, grad_src and grad_theta."""
    theta = R.theta_case("rotate", 2, np.random.default_rng(2)) * torch.tensor([[[0.9], [0.9]]])
    idx, frame = points(2, 370, 1226, 20000, 6, theta, 384, 384, 4e-3, extras=False)
    run_points("lift full size (2, 96, 384, 384) at 20000 of (370, 1226)", source((2, 96, 384, 384), 5), theta, idx, frame, 370, 1226, "nchw")


# ------------------------------------------------------------------------------------------------------------------ structure
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("kind", ["scale", "rotate"])
def test_lift_equals_the_dense_form_bit_for_bit(kind, layout):
    from fusiontransformer_amd import functional as spf
    src, theta = on_device(source((3, 5, 23, 37), 6), layout), R.theta_case(kind, 3, np.random.default_rng(3)).cuda()
    H, W = 37, 50
    f, r, c = R.dense_pixels(3, H, W)                       # every pixel of the target as a point
    idx, frame = torch.stack([r, c], 1).cuda(), f.int().cuda()
    dense = spf.affine_sample(src, theta, (H, W))
    rows = spf.affine_lift(src, theta, idx, frame, H, W)
    assert torch.equal(rows, dense[frame.long(), :, idx[:, 0], idx[:, 1]])
    assert rows.abs().max().item() > 0 and (rows == 0).any().item()       # samples inside and outside


def test_every_backward_output_repeats_bit_for_bit():
    from fusiontransformer_amd import functional as spf
    theta = R.theta_case("rotate", 3, np.random.default_rng(4))
    src = source((3, 96, 48, 48), 7)
    idx, frame = points(3, 40, 60, 1000, 8, theta, 48, 48, 0.0)
    runs = []
    for _ in range(3):
        sd, td = src.cuda().requires_grad_(True), theta.cuda().requires_grad_(True)
        (spf.affine_lift(sd, td, idx.cuda(), frame.cuda(), 40, 60) * source((1000, 96), 9).cuda()).sum().backward()
        t2 = theta.cuda().requires_grad_(True)
        (spf.affine_sample(src.cuda(), t2, (33, 65)) * source((3, 96, 33, 65), 10).cuda()).sum().backward()
        runs.append((sd.grad.clone(), td.grad.clone(), t2.grad.clone()))
        torch.empty(1 << 22, device="cuda").normal_()        # disturb the allocator and the caches between runs
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


GUARD = 256
SENTINEL = 0x7FA5A5A5         # a NaN with a payload: an output element that was never written is not finite, a band that was is changed


def _banded(shape, data=None, strides=None):
    """A tensor of `shape` as a view into the middle of a larger allocation: (whole, view).  With data: NaN bands around a copy of it (an
    operand).  Without: the sentinel everywhere (an output)."""
    n = int(np.prod(shape))
    if data is None:
        whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    else:
        whole = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
    view = whole[GUARD:GUARD + n].view(shape) if strides is None else torch.as_strided(whole, shape, strides, GUARD)
    if data is not None:
        view.copy_(data.cuda())
    return whole, view


def _bands_intact(whole):
    w = whole.view(torch.int32)
    return bool((w[:GUARD] == SENTINEL).all() and (w[-GUARD:] == SENTINEL).all())


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
@pytest.mark.parametrize("shape,size,n", [((1, 1, 1, 1), (1, 1), 1), ((2, 5, 5, 7), (7, 5), 65), ((3, 96, 23, 37), (16, 16), 1000)])
def test_guard_bands(shape, size, n, layout):
    """Every float operand sits between NaN bands, every output and the workspace between sentinel bands, inside larger allocations: a
    read outside an operand poisons the result, a write outside an output changes a band, an element never written stays a NaN."""
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd._lib import check, ptr, stream
    L = _lib.load()
    b, c, ih, iw = shape
    H, W = size
    st = (c * ih * iw, ih * iw, iw, 1) if layout == "nchw" else (ih * iw * c, 1, iw * c, c)
    strides = (ctypes.c_int64 * 4)(*st)
    theta = R.theta_case("scale", b, np.random.default_rng(12))
    idx, frame = points(b, H, W, n, 13, theta, ih, iw, 0.0)
    n = idx.shape[0]
    _, src = _banded(shape, source(shape, 14), st)
    _, th = _banded((b, 2, 3), theta)
    _, go_d = _banded((b, c, H, W), source((b, c, H, W), 15))
    _, go_p = _banded((n, c), source((n, c), 16))
    idx_d, frame_d = idx.cuda(), frame.cuda()
    ws_bytes = int(L.ftx_affine_theta_workspace_bytes(b))
    ws_whole = torch.full((ws_bytes // 4 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    ws = ws_whole[GUARD:]
    outs = {k: _banded(s, strides=(st if k == "grad_src" else None)) for k, s in
            dict(out=(b, c, H, W), rows=(n, c), gt_dense=(b, 2, 3), gt_lift=(b, 2, 3), grad_src=shape).items()}
    cells = torch.empty((n,), dtype=torch.int32, device="cuda")
    check(L.ftx_affine_sample_fwd(ptr(src), strides, b, c, ih, iw, ptr(th), H, W, ptr(outs["out"][1]), stream()), "fwd")
    check(L.ftx_affine_sample_bwd_theta(ptr(src), strides, b, c, ih, iw, ptr(th), ptr(go_d), H, W, ptr(outs["gt_dense"][1]), ptr(ws), ws_bytes,
                                        stream()), "bwd_theta")
    check(L.ftx_affine_lift_fwd(ptr(src), strides, b, c, ih, iw, ptr(th), ptr(idx_d), ptr(frame_d), n, H, W, ptr(outs["rows"][1]), stream()), "lift")
    check(L.ftx_affine_lift_cells(ptr(th), ptr(idx_d), ptr(frame_d), n, b, ih, iw, H, W, ptr(cells), stream()), "cells")
    from fusiontransformer_amd.functional import Segments
    seg = Segments(cells, b * (ih + 1) * (iw + 1))
    check(L.ftx_affine_lift_bwd(ptr(src), strides, b, c, ih, iw, ptr(th), ptr(idx_d), ptr(frame_d), ptr(go_p), n, H, W, ptr(seg.order),
                                ptr(seg.seg_off), ptr(outs["grad_src"][1]), ptr(outs["gt_lift"][1]), ptr(ws), ws_bytes, stream()), "lift_bwd")
    torch.cuda.synchronize()
    for k, (whole, view) in outs.items():
        assert _bands_intact(whole), "a guard band of %s was written" % k
        assert bool(torch.isfinite(view).all()), "%s: an element was not written, or something outside an operand was read" % k
    w = ws_whole
    assert bool((w[:GUARD] == SENTINEL).all() and (w[GUARD + ws_bytes // 4:] == SENTINEL).all()), "the workspace's bands were written"
    # the keys: -1 exactly for the points that contribute nothing, inside the key space otherwise
    cells_h, rows_h = cells.cpu(), outs["rows"][1].cpu()
    assert int(cells_h.max()) < b * (ih + 1) * (iw + 1) and int(cells_h.min()) >= -1
    assert n < 8 or bool((cells_h[-4:] == -1).all())
    assert bool((rows_h[cells_h == -1] == 0).all())
    # and the direct calls computed what the wrappers compute
    from fusiontransformer_amd import functional as spf
    assert torch.equal(outs["out"][1], spf.affine_sample(src, th.contiguous(), (H, W)))


# ------------------------------------------------------------------------------------------------------------------ modules
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _load(mod, golden, tag):
    mod.load_state_dict({str(n): torch.from_numpy(golden["%s_param_%s" % (tag, n)]) for n in golden[tag + "_names"]})
    return mod


def _param_grad_errors(mod, golden, tag):
    """Worst relative L2 error of a parameter's gradient against the golden's."""
    worst = 0.0
    for n, p in mod.named_parameters():
        want = torch.from_numpy(golden["%s_grad_%s" % (tag, n)])
        assert p.grad is not None, n
        worst = max(worst, ((p.grad.detach().cpu().double() - want).norm() / want.norm()).item())
    return worst


def _module_bar(case, quantity, ek, ey):
    line = "%s | %s | %.3e | %.3e | %.3e" % (case, quantity, ek, ey, BAR_FACTOR * ey)
    REPORT.append(line)
    print(line)
    assert ek <= BAR_FACTOR * ey, line


def test_spatial_transformer_module_against_the_golden(golden):
    """Yardstick: the same module in float32 on the CPU, where it runs torch's affine_grid + grid_sample."""
    from fusiontransformer_amd.models.transformers import SpatialTransformer
    x, g = torch.from_numpy(golden["st_x"]).float(), torch.from_numpy(golden["st_g"]).float()
    want, want_gx = torch.from_numpy(golden["st_y"]), torch.from_numpy(golden["st_grad_x"])
    cpu = _load(SpatialTransformer(3), golden, "st")
    y32 = cpu(x, (3, 24, 24))
    (y32 * g).sum().backward()
    dev = _load(SpatialTransformer(3), golden, "st").cuda()
    y = dev(x.cuda(), (3, 24, 24))
    (y * g.cuda()).sum().backward()
    _module_bar("SpatialTransformer(3) golden", "output", (y.detach().cpu().double() - want).abs().max().item(), (y32.detach().double() - want).abs().max().item())
    _module_bar("SpatialTransformer(3) golden", "parameter gradients (worst rel L2)", _param_grad_errors(dev, golden, "st"), _param_grad_errors(cpu, golden, "st"))
    assert want_gx.shape == x.shape     # the dense form gives the image no gradient; the golden's is checked through ScaleUpModule.lift


def test_scale_up_module_against_the_golden(golden):
    from fusiontransformer_amd.models.transformers import ScaleUpModule
    x, g = torch.from_numpy(golden["su_x"]).float(), torch.from_numpy(golden["su_g"]).float()
    idx, frame = torch.from_numpy(golden["su_idx"]), torch.from_numpy(golden["su_frame"])
    H, W = (int(v) for v in golden["su_size"])
    want, want_gx, want_dense = torch.from_numpy(golden["su_feats"]), torch.from_numpy(golden["su_grad_x"]), torch.from_numpy(golden["su_dense"])
    cpu = _load(ScaleUpModule(16, 8, 4, 4), golden, "su")
    xc = x.clone().requires_grad_(True)
    d32 = cpu(xc, (8, H, W))
    f32 = R.pick(d32, idx, frame)
    (f32 * g).sum().backward()
    dev = _load(ScaleUpModule(16, 8, 4, 4), golden, "su").cuda()
    xd = x.cuda().requires_grad_(True)
    feats = dev.lift(xd, idx.cuda(), frame.cuda(), H, W)
    (feats * g.cuda()).sum().backward()
    with torch.no_grad():
        dense = dev(xd, (8, H, W))
    case = "ScaleUpModule(16, 8, 4, 4) golden"
    _module_bar(case, "dense output", (dense.cpu().double() - want_dense).abs().max().item(), (d32.detach().double() - want_dense).abs().max().item())
    _module_bar(case, "picked rows", (feats.detach().cpu().double() - want).abs().max().item(), (f32.detach().double() - want).abs().max().item())
    _module_bar(case, "input gradient", (xd.grad.cpu().double() - want_gx).abs().max().item(), (xc.grad.double() - want_gx).abs().max().item())
    _module_bar(case, "parameter gradients (worst rel L2)", _param_grad_errors(dev, golden, "su"), _param_grad_errors(cpu, golden, "su"))
    # lift == forward then pick, bit for bit
    assert torch.equal(feats.detach(), R.pick(dense, idx.cuda(), frame.cuda()))
    with pytest.raises(RuntimeError):
        dev(xd, (8, H, W))               # the dense form refuses a map that needs a gradient: lift is the training path


# ------------------------------------------------------------------------------------------------------------------ model
TOL = 1e-3          # tests/test_model_gpu.py: per-point logits within 1e-3 of the reference CPU path
GRAD_REL_L2 = 5e-2  # tests/test_model_gpu.py: worst relative L2 of a parameter gradient against the float64 oracle, with its floor


def _small_model(seed):
    from fusiontransformer_amd.models.image_models_stn import Net2DSeg
    torch.manual_seed(seed)
    model = Net2DSeg(num_classes=20, dual_head=False, backbone_2d_kwargs=dict(vit_depth=2, late_feat_block_number=1, stn_feat_channels=8))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():     # off the identity initialisation, so that the localisation nets take part in the gradient
        for st in (model.stn_down, model.up["1"].up_stn):
            st.fc_loc[2].weight.copy_(torch.randn(st.fc_loc[2].weight.shape, generator=g) * 0.02)
    return model


def test_net2dseg_train_mode_matches_the_float64_restatement():
    import torch.nn.functional as F
    from oracle import ft_oracle as O
    model = _small_model(21)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    B, H, W, n = 2, 48, 80, 300
    g = torch.Generator().manual_seed(22)
    img = torch.randn((B, 3, H, W), generator=g)
    idx_all = torch.stack([torch.randint(0, H, (B * n,), generator=g), torch.randint(0, W, (B * n,), generator=g)], 1)
    frame = torch.repeat_interleave(torch.arange(B), n).int()
    label = torch.randint(0, 20, (B * n,), generator=g)
    cw = torch.rand(20, generator=g) + 0.5

    # float64 restatement: oracle trunk + stn_ref
    trunk = O.Image2DTransformer(depth=2).double()
    trunk.load_state_dict({k[len("backbone."):]: v.double() for k, v in sd.items() if k.startswith("backbone.")})
    p64 = {k: v.double().requires_grad_(True) for k, v in sd.items() if not k.startswith("backbone.")}
    x = R.spatial_transformer(p64, "stn_down.", img.double(), (384, 384))
    tokens = trunk.forward_blocks(x)["1"]
    tmap = tokens.transpose(1, 2).reshape(B, 768, 24, 24)
    feats = R.scale_up_points(p64, "up.1.", tmap, idx_all, frame, H, W, 16)
    ref = F.linear(feats, p64["linear.weight"], p64["linear.bias"])
    F.cross_entropy(ref, label, weight=cw.double()).backward()
    want = {k: v.grad for k, v in p64.items()}
    want.update({"backbone." + k: v.grad for k, v in trunk.named_parameters()})

    model = model.cuda().train()
    per_frame = [idx_all[i * n:(i + 1) * n].numpy() for i in range(B)]
    out = model(img.cuda(), per_frame)
    F.cross_entropy(out["img_seg_logit"], label.cuda(), weight=cw.cuda()).backward()
    err = (out["img_seg_logit"].detach().cpu().double() - ref.detach()).abs().max().item()
    print("Net2DSeg logits: max abs error %.3e (gate %.1e)" % (err, TOL))
    assert err <= TOL
    gmax = max(v.abs().max().item() for v in want.values() if v is not None)
    report = []
    for name, p in model.named_parameters():
        w = want[name]
        if w is None:
            assert p.grad is None or p.grad.abs().max().item() == 0, name
            continue
        assert p.grad is not None, name
        floor = 1e-4 * gmax * p.numel() ** 0.5
        report.append(((p.grad.cpu().double() - w).norm().item() / max(w.norm().item(), floor), name))
    report.sort(reverse=True)
    print("Net2DSeg gradients: worst relative L2", report[:3])
    assert report[0][0] < GRAD_REL_L2, report[:5]
    for name, p in model.named_parameters():
        if name.startswith(("stn_down.", "up.1.up_stn.")):
            assert p.grad is not None and p.grad.abs().max().item() > 0, name


def test_train_step_of_the_imageseg_model_runs_and_repeats():
    """build_model(image_stn_cfg()) through TrainStep's image mode.  A narrow model on a small picture: the library's first-use search
    for each new convolution shape of the localisation nets takes seconds at full size (20 s measured), and this test is about the
    plumbing -- mode, loss, optimizer, repeatability -- not about those shapes."""
    from fusiontransformer_amd.config import image_stn_cfg
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    cfg = image_stn_cfg()
    cfg.MODEL.vit_depth, cfg.MODEL.late_feat_block_number, cfg.MODEL.stn_feat_channels = 2, 1, 8
    torch.manual_seed(31)
    first, _ = build_model(cfg)
    state = {k: v.clone() for k, v in first.state_dict().items()}
    B, H, W, n = 2, 48, 80, 300
    g = torch.Generator().manual_seed(32)
    idx = torch.stack([torch.randint(0, H, (B * n,), generator=g), torch.randint(0, W, (B * n,), generator=g)], 1)
    batch = {"img": torch.randn((B, 3, H, W), generator=g).cuda(), "img_indices": [idx[i * n:(i + 1) * n].numpy() for i in range(B)],
             "seg_label": torch.randint(0, 20, (B * n,), generator=g).cuda()}
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True      # the localisation nets' convolutions are the library's: ask it for its repeatable algorithms
    try:
        results = []
        for _ in range(2):
            model, metric = build_model(cfg)
            model.load_state_dict(state)
            model = model.cuda().train()
            step = TrainStep(cfg, model, metrics=metric)
            assert step.mode == "image"
            step(batch)
            loss = step.last["loss_2d"]
            assert bool(torch.isfinite(loss))
            results.append((loss.clone(), {k: v.detach().clone() for k, v in model.state_dict().items()}))
    finally:
        torch.backends.cudnn.deterministic = was
    moved = [k for k, v in results[0][1].items() if v.dtype.is_floating_point and not torch.equal(v.cpu(), state[k])]
    trainable = [n_ for n_, p in first.named_parameters() if p.requires_grad]
    assert set(trainable) <= set(moved), sorted(set(trainable) - set(moved))[:5]
    assert torch.equal(results[0][0], results[1][0])
    for k, v in results[0][1].items():
        assert torch.equal(v, results[1][1][k]), k
