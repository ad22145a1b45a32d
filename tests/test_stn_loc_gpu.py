"""The fused localisation-net kernels (csrc/ftx_stn_loc.hip), functional.loc_conv_pool_relu and the "ftx" localisation path of the
spatial-transformer modules and of the ImageSeg model, on the GPU.

Bars.  No tolerance here is a number.  Truth: F.conv2d / max_pool2d / relu in float64 on the CPU (tests/loc_ref.py).  Yardstick: the
same in float32 on the CPU on the same inputs.  Bar = BAR_FACTOR (4, as tests/test_stn_gpu.py) x the yardstick's worst error for that
case and quantity: absolute for the pooled output, the mean and dX, relative L2 per tensor for dW and db.  Where the truth is exactly
0 the kernel's result must be exactly 0.

Routing is a kink, so the forward's routing and the backward's arithmetic are judged apart.  Forward: sel must equal the truth's
everywhere except in ambiguous windows (float64 top-two gap < 2 x that case's forward bar, or |maximum| < 1 x that bar: two values
each within the bar of the truth cannot swap order or sign otherwise); the ambiguous share is asserted < 0.5 % on the CPU first.
Backward: the C entries are called with the TRUTH's sel; given the routing they are linear, and they are compared with float64
autograd against a float32 CPU yardstick that uses the same routing.  Nothing is left out of these comparisons.

With FTX_TEST_REPORT_DIR set, every measured error and its bar is written to <dir>/stn_loc_accuracy.txt."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import loc_ref as LR
from tests import stn_ref as R

pytestmark = pytest.mark.gpu
BAR_FACTOR = LR.BAR_FACTOR
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    d = os.environ.get("FTX_TEST_REPORT_DIR")
    if d and REPORT:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "stn_loc_accuracy.txt"), "w") as f:
            f.write("case | quantity | kernel error | yardstick error (torch float32 on the CPU) | bar = %d x yardstick\n" % BAR_FACTOR)
            f.write("\n".join(REPORT) + "\n")


def inside_bar(case, quantity, got, yard, truth, relative=False):
    """Prints the figures, then asserts the kernel's error against BAR_FACTOR x the yardstick's."""
    if relative:
        ek, ey = LR.rel_l2(got, truth), LR.rel_l2(yard, truth)
    else:
        ek, ey = (got.double() - truth).abs().max().item(), (yard.double() - truth).abs().max().item()
    line = "%s | %s | %.3e | %.3e | %.3e" % (case, quantity, ek, ey, BAR_FACTOR * ey)
    REPORT.append(line)
    print(line)
    if truth.abs().max().item() == 0:
        assert got.abs().max().item() == 0, (case, quantity, "the truth is exactly 0, the kernel's result is not")
    assert ek <= BAR_FACTOR * ey, line


def on_device(x, layout):
    d = x.cuda()
    return d if layout == "nchw" else d.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def strides_of(t):
    return (ctypes.c_int64 * 4)(*t.stride())


def backward_entries(xd, wd, sel_d, g_d, gstrides, shape, want_dx=True):
    """The two backward C entries under a given routing -> (dX with x's strides or None, dW, db)."""
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd._lib import check, ptr, stream
    L = _lib.load()
    b, c, ih, iw, k, co = shape
    dw, db = torch.empty_like(wd), torch.empty((co,), device="cuda")
    ws_bytes = int(L.ftx_loc_conv_pool_relu_bwd_weight_workspace_bytes(b, c, ih, iw, k, co))
    assert ws_bytes > 0
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    check(L.ftx_loc_conv_pool_relu_bwd_weight(ptr(xd), strides_of(xd), b, c, ih, iw, ptr(sel_d), ptr(g_d), gstrides, k, co, ptr(dw), ptr(db),
                                              ptr(ws), ws_bytes, stream()), "bwd_weight")
    dx = None
    if want_dx:
        dx = torch.empty_strided(xd.shape, xd.stride(), dtype=torch.float32, device="cuda")
        check(L.ftx_loc_conv_pool_relu_bwd_data(ptr(wd), ptr(sel_d), ptr(g_d), gstrides, b, c, ih, iw, k, co, ptr(dx), strides_of(dx), stream()),
              "bwd_data")
    return dx, dw, db


def run_case(shape, layout, mean_backward):
    from fusiontransformer_amd import functional as spf
    cs = LR.case(shape)
    name = "loc %s %s" % (shape, layout)
    b, c, ih, iw, k, co = shape
    ph, pw = LR.pooled_size(ih, iw, k)
    assert cs["ambiguous_share"] < LR.AMBIGUOUS_CAP, "%s: %.3f %% of the windows are ambiguous" % (name, 100 * cs["ambiguous_share"])
    xd, wd, bd = on_device(cs["x"], layout), cs["w"].cuda(), cs["bias"].cuda()

    # forward: the pooled map and its routing
    got, sel = spf.loc_conv_pool_relu(xd, wd, bd, return_sel=True)
    assert got.shape == cs["truth"].shape and got.is_contiguous() and sel.dtype == torch.int8 and sel.shape == got.shape
    inside_bar(name, "forward", got.cpu(), cs["yard"], cs["truth"])
    differs = sel.cpu() != cs["sel"]
    line = "%s | routing | %d of %d windows differ from the truth's, %d ambiguous" % (name, int(differs.sum()), differs.numel(), int(cs["ambiguous"].sum()))
    REPORT.append(line)
    print(line)
    assert not bool((differs & ~cs["ambiguous"]).any()), line
    # the mean form: same routing bytes, the spatial mean in place of the map
    gmean, sel_m = spf.loc_conv_pool_relu(xd, wd, bd, mean=True, return_sel=True)
    assert gmean.shape == (b, co) and torch.equal(sel_m, sel)
    inside_bar(name, "mean", gmean.cpu(), cs["yard_mean"], cs["truth_mean"])

    # backward under the truth's routing
    sel_d = cs["sel"].cuda()
    g = torch.randn((b, co, ph, pw), generator=torch.Generator().manual_seed(99))
    truth, yard = LR.backward_truth(shape, g, mean=False)
    g_d = g.cuda()
    dx, dw, db = backward_entries(xd, wd, sel_d, g_d, strides_of(g_d), shape)
    assert dx.stride() == xd.stride()
    inside_bar(name, "dX", dx.cpu(), yard[0], truth[0])
    inside_bar(name, "dW", dw.cpu(), yard[1], truth[1], relative=True)
    inside_bar(name, "db", db.cpu(), yard[2], truth[2], relative=True)
    if mean_backward:   # the mean's backward: g[b, co] / (ph pw) read with zero strides, no tensor behind it
        gm = torch.randn((b, co), generator=torch.Generator().manual_seed(98))
        truth, yard = LR.backward_truth(shape, gm, mean=True)
        gm_d = (gm / (ph * pw)).cuda()
        dx, dw, db = backward_entries(xd, wd, sel_d, gm_d, (ctypes.c_int64 * 4)(co, 1, 0, 0), shape)
        inside_bar(name, "dX (mean)", dx.cpu(), yard[0], truth[0])
        inside_bar(name, "dW (mean)", dw.cpu(), yard[1], truth[1], relative=True)
        inside_bar(name, "db (mean)", db.cpu(), yard[2], truth[2], relative=True)


@pytest.mark.parametrize("shape,layout", LR.SMALL)
def test_forward_mean_and_gradients(shape, layout):
    run_case(shape, layout, mean_backward=True)


@pytest.mark.parametrize("shape", LR.FULL)
def test_full_size_forward_and_backward(shape):
    """The model's sizes at b = 1: the up-convolved 96 x 384 x 384 map, the second layer with its dropped 185th row and column, and the
    370 x 1226 picture."""
    run_case(shape, "nchw", mean_backward=False)


def test_autograd_function_matches_its_own_entries():
    """functional.loc_conv_pool_relu's backward is the C entries under the forward's own routing, map and mean form."""
    from fusiontransformer_amd import functional as spf
    shape = (2, 8, 21, 30, 5, 90)
    cs = LR.case(shape)
    ph, pw = LR.pooled_size(21, 30, 5)
    for mean in (False, True):
        xd, wd, bd = (t.cuda().requires_grad_(True) for t in (cs["x"], cs["w"], cs["bias"]))
        out, sel = spf.loc_conv_pool_relu(xd, wd, bd, mean=mean, return_sel=True)
        g = torch.randn(out.shape, generator=torch.Generator().manual_seed(97)).cuda()
        (out * g).sum().backward()
        if mean:
            g_d, gs = (g * (1.0 / (ph * pw))).contiguous(), (ctypes.c_int64 * 4)(90, 1, 0, 0)
        else:
            g_d, gs = g, strides_of(g)
        dx, dw, db = backward_entries(xd.detach(), wd.detach(), sel, g_d, gs, shape)
        assert torch.equal(xd.grad, dx) and torch.equal(wd.grad, dw) and torch.equal(bd.grad, db)
    # an input that needs no gradient gets none, and the parameters' are the same bits
    out = spf.loc_conv_pool_relu(cs["x"].cuda(), wd, bd, mean=True)
    gw, gb = torch.autograd.grad((out * g).sum(), (wd, bd))
    assert torch.equal(gw, dw) and torch.equal(gb, db)


def test_refusals():
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    x, w, bias = LR.inputs((1, 3, 7, 12, 7, 8))
    with pytest.raises(ValueError):
        spf.loc_conv_pool_relu(x.cuda(), w.cuda(), bias.cuda())          # ih = 7 at k = 7: ph = 0, torch's pool refuses it too
    L = _lib.load()
    xd, wd, sel = x.cuda(), w.cuda(), torch.empty((8,), dtype=torch.int8, device="cuda")
    out = torch.empty((8,), device="cuda")
    rc = L.ftx_loc_conv_pool_relu_fwd(xd.data_ptr(), strides_of(xd), 1, 3, 7, 12, wd.data_ptr(), 0, 7, 8, out.data_ptr(), sel.data_ptr(), 0, 0, 0, 0)
    assert rc == -1 and b"no pooled pixel" in L.ftx_last_error()
    x, w, bias = LR.inputs((1, 3, 9, 12, 7, 8))
    with pytest.raises(ValueError):
        spf.loc_conv_pool_relu(x, w, bias)                               # CPU tensors
    with pytest.raises(ValueError):
        spf.loc_conv_pool_relu(x.cuda(), w.cuda()[:, :, :5, :5].contiguous(), bias.cuda())   # a (k, co) that is not served
    with pytest.raises(ValueError):
        spf.loc_conv_pool_relu(x.cuda().expand(2, 3, 9, 12), w.cuda(), bias.cuda())          # aliasing strides


def test_every_backward_output_repeats_bit_for_bit():
    from fusiontransformer_amd import functional as spf
    runs = []
    for _ in range(3):
        outs = []
        for shape, mean in (((2, 96, 23, 37, 7, 8), False), ((3, 8, 40, 70, 5, 90), True), ((1, 3, 48, 80, 7, 8), False)):
            cs = LR.case(shape)
            xd, wd, bd = (t.cuda().requires_grad_(True) for t in (cs["x"], cs["w"], cs["bias"]))
            out, sel = spf.loc_conv_pool_relu(xd, wd, bd, mean=mean, return_sel=True)
            (out * torch.randn(out.shape, generator=torch.Generator().manual_seed(96)).cuda()).sum().backward()
            outs += [out.detach().clone(), sel.clone(), xd.grad.clone(), wd.grad.clone(), bd.grad.clone()]
        runs.append(outs)
        torch.empty(1 << 22, device="cuda").normal_()        # disturb the allocator and the caches between runs
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


GUARD = 256
SENTINEL = 0x7FA5A5A5         # a NaN with a payload: an output element that was never written is not finite, a band that was is changed
SENTINEL8 = 0x5A              # for the routing bytes: not a position


def _banded(shape, data=None, strides=None):
    """A float32 tensor of `shape` as a view into the middle of a larger allocation: (whole, view).  With data: NaN bands around a copy
    of it (an operand).  Without: the sentinel everywhere (an output)."""
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
@pytest.mark.parametrize("shape", [(2, 3, 9, 12, 7, 8), (2, 8, 21, 30, 5, 90)])
def test_guard_bands(shape, layout):
    """Every float operand sits between NaN bands, every output, sel and the workspaces between sentinel bands, inside larger allocations:
    a read outside an operand poisons the result, a write outside an output changes a band, an element never written stays a sentinel."""
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd._lib import check, ptr, stream
    L = _lib.load()
    cs = LR.case(shape)
    b, c, ih, iw, k, co = shape
    ph, pw = LR.pooled_size(ih, iw, k)
    st = (c * ih * iw, ih * iw, iw, 1) if layout == "nchw" else (ih * iw * c, 1, iw * c, c)
    xs = (ctypes.c_int64 * 4)(*st)
    _, x = _banded((b, c, ih, iw), cs["x"], st)
    _, w = _banded(cs["w"].shape, cs["w"])
    _, bias = _banded((co,), cs["bias"])
    _, g = _banded((b, co, ph, pw), torch.randn((b, co, ph, pw), generator=torch.Generator().manual_seed(95)))
    _, gm = _banded((b, co), torch.randn((b, co), generator=torch.Generator().manual_seed(94)))
    outs = {kk: _banded(s, strides=(st if kk.startswith("dx") else None)) for kk, s in
            dict(out=(b, co, ph, pw), mean=(b, co), dw=cs["w"].shape, db=(co,), dx=(b, c, ih, iw), dw_m=cs["w"].shape, db_m=(co,),
                 dx_m=(b, c, ih, iw)).items()}
    sels = {}
    for kk in ("sel", "sel_m"):
        whole = torch.full((b * co * ph * pw + 2 * GUARD,), SENTINEL8, dtype=torch.int8, device="cuda")
        sels[kk] = (whole, whole[GUARD:-GUARD].view(b, co, ph, pw))
    fws, bws = int(L.ftx_loc_conv_pool_relu_fwd_workspace_bytes(b, co, ph, pw)), int(L.ftx_loc_conv_pool_relu_bwd_weight_workspace_bytes(b, c, ih, iw, k, co))
    assert fws > 0 and bws > 0 and fws % 4 == 0 and bws % 4 == 0
    ws_whole = {kk: torch.full((n // 4 + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for kk, n in (("fwd", fws), ("bwd", bws))}
    ws = {kk: v[GUARD:] for kk, v in ws_whole.items()}
    check(L.ftx_loc_conv_pool_relu_fwd(ptr(x), xs, b, c, ih, iw, ptr(w), ptr(bias), k, co, ptr(outs["out"][1]), ptr(sels["sel"][1]), 0, 0, 0, stream()), "fwd")
    check(L.ftx_loc_conv_pool_relu_fwd(ptr(x), xs, b, c, ih, iw, ptr(w), ptr(bias), k, co, 0, ptr(sels["sel_m"][1]), ptr(outs["mean"][1]), ptr(ws["fwd"]), fws,
                                       stream()), "fwd mean")
    sel = sels["sel"][1]
    for tag, gp, gs in (("", g, strides_of(g)), ("_m", gm, (ctypes.c_int64 * 4)(co, 1, 0, 0))):
        check(L.ftx_loc_conv_pool_relu_bwd_weight(ptr(x), xs, b, c, ih, iw, ptr(sel), ptr(gp), gs, k, co, ptr(outs["dw" + tag][1]), ptr(outs["db" + tag][1]),
                                                  ptr(ws["bwd"]), bws, stream()), "bwd_weight")
        check(L.ftx_loc_conv_pool_relu_bwd_data(ptr(w), ptr(sel), ptr(gp), gs, b, c, ih, iw, k, co, ptr(outs["dx" + tag][1]), xs, stream()), "bwd_data")
    torch.cuda.synchronize()
    for kk, (whole, view) in outs.items():
        assert _bands_intact(whole), "a guard band of %s was written" % kk
        assert bool(torch.isfinite(view).all()), "%s: an element was not written, or something outside an operand was read" % kk
    for kk, (whole, view) in sels.items():
        assert bool((whole[:GUARD] == SENTINEL8).all() and (whole[-GUARD:] == SENTINEL8).all()), "a guard band of %s was written" % kk
        assert int(view.min()) >= -1 and int(view.max()) <= 3, "%s: an element was not written" % kk
    for kk, n in (("fwd", fws), ("bwd", bws)):
        wv = ws_whole[kk]
        assert bool((wv[:GUARD] == SENTINEL).all() and (wv[GUARD + n // 4:] == SENTINEL).all()), "the %s workspace's bands were written" % kk
    # and the direct calls computed what the wrapper computes
    from fusiontransformer_amd import functional as spf
    assert torch.equal(outs["out"][1], spf.loc_conv_pool_relu(x, w.contiguous(), bias.contiguous()))
    assert torch.equal(sels["sel_m"][1], sel)


# ------------------------------------------------------------------------------------------------------------------ modules, model
def test_spatial_transformer_theta_on_the_fused_path():
    """SpatialTransformer(96).theta with "ftx" against the float64 chain, the module's own float32 CPU result as the yardstick."""
    from fusiontransformer_amd.models.transformers import SpatialTransformer
    torch.manual_seed(41)
    mod = SpatialTransformer(8)
    with torch.no_grad():
        mod.fc_loc[2].weight.copy_(torch.randn(mod.fc_loc[2].weight.shape) * 0.02)
    x = torch.randn((2, 8, 48, 80), generator=torch.Generator().manual_seed(42))
    truth = R.theta_of({k: v.double() for k, v in mod.state_dict().items()}, "", x.double())
    yard = mod.theta(x).detach()
    dev = SpatialTransformer(8)
    dev.load_state_dict(mod.state_dict())
    dev = dev.cuda().set_loc_impl("ftx")
    inside_bar("SpatialTransformer(8).theta ftx", "theta", dev.theta(x.cuda()).detach().cpu(), yard, truth)


TOL = 1e-3          # tests/test_stn_gpu.py: per-point logits within 1e-3 of the float64 restatement
GRAD_REL_L2 = 5e-2  # tests/test_stn_gpu.py: worst relative L2 of a parameter gradient against the float64 oracle, with its floor


def _small_model(seed, **kw):
    from fusiontransformer_amd.models.image_models_stn import Net2DSeg
    torch.manual_seed(seed)
    model = Net2DSeg(num_classes=20, dual_head=False, backbone_2d_kwargs=dict(vit_depth=2, late_feat_block_number=1, stn_feat_channels=8, **kw))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():     # off the identity initialisation, so that the localisation nets take part in the gradient
        for st in (model.stn_down, model.up["1"].up_stn):
            st.fc_loc[2].weight.copy_(torch.randn(st.fc_loc[2].weight.shape, generator=g) * 0.02)
    return model


def test_net2dseg_with_the_fused_localisation_nets_matches_the_float64_restatement():
    """test_net2dseg_train_mode_matches_the_float64_restatement's setup and gates with stn_loc_impl="ftx"."""
    import torch.nn.functional as F
    from oracle import ft_oracle as O
    model = _small_model(21, stn_loc_impl="ftx")
    assert model.stn_down.loc_impl == "ftx" and model.up["1"].up_stn.loc_impl == "ftx"
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    B, H, W, n = 2, 48, 80, 300
    g = torch.Generator().manual_seed(22)
    img = torch.randn((B, 3, H, W), generator=g)
    idx_all = torch.stack([torch.randint(0, H, (B * n,), generator=g), torch.randint(0, W, (B * n,), generator=g)], 1)
    frame = torch.repeat_interleave(torch.arange(B), n).int()
    label = torch.randint(0, 20, (B * n,), generator=g)
    cw = torch.rand(20, generator=g) + 0.5

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
    print("Net2DSeg (ftx localisation) logits: max abs error %.3e (gate %.1e)" % (err, TOL))
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
    print("Net2DSeg (ftx localisation) gradients: worst relative L2", report[:3])
    assert report[0][0] < GRAD_REL_L2, report[:5]
    for name, p in model.named_parameters():
        if name.startswith(("stn_down.", "up.1.up_stn.")):
            assert p.grad is not None and p.grad.abs().max().item() > 0, name


@pytest.mark.parametrize("size,width", [((48, 80), 8), ((370, 1226), None)])
def test_train_step_repeats_bit_for_bit_without_the_library_switch(size, width):
    """build_model(image_stn_cfg()) with stn_loc_impl="ftx" through TrainStep twice from one state: the loss and every parameter are
    bit-identical with torch.backends.cudnn.deterministic left alone.  Once on the toy picture, once at full width on a
    (2, 3, 370, 1226) batch -- the shape whose first-use search the library path could not afford in a test."""
    from fusiontransformer_amd.config import image_stn_cfg
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    cfg = image_stn_cfg()
    cfg.MODEL.vit_depth, cfg.MODEL.late_feat_block_number, cfg.MODEL.stn_loc_impl = 2, 1, "ftx"
    if width is not None:
        cfg.MODEL.stn_feat_channels = width
    torch.manual_seed(31)
    first, _ = build_model(cfg)
    assert first.image_backbone.stn_down.loc_impl == "ftx"
    state = {k: v.clone() for k, v in first.state_dict().items()}
    B, (H, W), n = 2, size, 300
    g = torch.Generator().manual_seed(32)
    idx = torch.stack([torch.randint(0, H, (B * n,), generator=g), torch.randint(0, W, (B * n,), generator=g)], 1)
    batch = {"img": torch.randn((B, 3, H, W), generator=g).cuda(), "img_indices": [idx[i * n:(i + 1) * n].numpy() for i in range(B)],
             "seg_label": torch.randint(0, 20, (B * n,), generator=g).cuda()}
    was = torch.backends.cudnn.deterministic
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
    assert torch.backends.cudnn.deterministic == was
    moved = [k for k, v in results[0][1].items() if v.dtype.is_floating_point and not torch.equal(v.cpu(), state[k])]
    trainable = [n_ for n_, p in first.named_parameters() if p.requires_grad]
    assert set(trainable) <= set(moved), sorted(set(trainable) - set(moved))[:5]
    assert torch.equal(results[0][0], results[1][0])
    for k, v in results[0][1].items():
        assert torch.equal(v, results[1][1][k]), k
