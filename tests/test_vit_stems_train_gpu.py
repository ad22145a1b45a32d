"""The training forms of the ViT patch embedding and tap stems on the GPU (include/ftx.h: ftx_vit_patch_embed_bwd_*,
ftx_vit_tap_stem_train_fwd_*, ftx_vit_tap_stem_bwd_*; functional.vit_patch_embed / vit_tap_stem; cfg.MODEL.image_native_stems).

1. Bit identity.  Every product of a new entry equals the plain entry (ftx_dense_wgrad_*, ftx_dense_gemm_*, ftx_rows_gemm_*, ftx_colsum) run
   on operands materialised with the numpy restatement of tests/test_vit_stems_train_host.py, followed by the stated store: a wrong
   address is a failed comparison, not a tolerance question.  Every output and workspace lies between guard bands (tests/guard.py).
2. Accuracy against float64 at the bars of tests/dense_edges.py (the dense families' own: factor / wgrad_factor times 2^-24 sum |a b|).
3. Whole models: one training step (Adam included) of the smallest ImageSegBilinear and ImageSeg with the switch on, against the float64
   oracle and against the switch off at the gates of tests/test_fullsize_train_gpu.py / tests/test_single_modality_train_gpu.py; bit
   identity of two runs, of image_native_train on and off, and of the switch off with the eager twin.

Shapes are the smallest at which an address can go wrong: t0 in {0, 1, 2}; patch 8 with one channel (c p p = 64, one granule) and patch
16 with three; a 2 x 2 grid with one frame; a 7 x 7 grid with three frames (147 rows: crosses a 128-row tile, frames of odd length); 588
rows of a 64 x 64 weight gradient (two splits, the second shorter); co in {4, 96}, dim in {64, 768}."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import dense_edges as E
from tests import guard as GD
from tests.helpers import product_inputs
from tests.test_fullsize_train_gpu import TOL_GRAD, TOL_LOGIT, TOL_LOSS
from tests.test_native_image_gpu import same
from tests.test_native_image_train_gpu import _cfg, _models, _steps
from tests.test_native_train_gpu import _assert_same_state, _graph_nodes
from tests.test_single_modality_train_gpu import TOL_BN
from tests.test_vit_stems_train_host import fold_np, strip_np, strip_store_np, unfold_np

pytestmark = pytest.mark.gpu
U = E.U
DEV = "cuda"
FAMILIES = E.FAMILIES
# (b, c, patch, grid, dim, t0, weight-gradient splits)
PATCH_CASES = [(1, 1, 8, 2, 64, 1, 1), (3, 3, 16, 7, 768, 2, 1), (3, 1, 8, 7, 64, 2, 1), (3, 1, 8, 14, 64, 1, 2)]
# (b, g, t0, dim, co, weight-gradient splits)
TAP_CASES = [(1, 4, 0, 64, 4, 1), (3, 49, 1, 768, 96, 1), (3, 49, 2, 64, 96, 1), (3, 196, 2, 64, 4, 2), (1, 4, 2, 768, 96, 1)]


@pytest.fixture(scope="module")
def env():
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return spf, _lib.load()


class Out:
    """An output between guard bands, the sentinel (a NaN) everywhere, 16-byte aligned and no more (tests/test_dense_edges_gpu.py)."""

    def __init__(self, shape):
        self.whole, self.view = GD.banded(shape, band=GD.dense_band(shape), device=DEV)
        self.address = GD.address(self.whole, self.view)

    def checked(self, what):
        assert GD.bands_intact(self.whole, self.view), (what, "a guard band was written")
        assert GD.written(self.view), (what, "an element was not written, or is not finite")
        return self.view


def operand(t):
    """A float operand between NaN bands: a read outside it poisons what it is multiplied into."""
    return GD.banded(t.shape, data=t, band=GD.dense_band(t.shape), device=DEV)[1]


def call(env, name, *args):
    spf, L = env
    spf.check(getattr(L, name)(*args, spf.stream()), name)
    torch.cuda.synchronize()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _id(case):
    return "-".join(map(str, case))


class Gate(object):
    def __init__(self):
        self.figures = []

    def __call__(self, what, out, ref, bound):
        r = E.worst(out, ref, bound)
        self.figures.append(f"{what} {r:.3g}")
        assert E.passes(out, ref, bound), (what, r)

    def record(self, head):
        print(f"\nSTEMS {head}: " + "  ".join(self.figures))


# ---------------------------------------------------------------- 1 + 2. the patch embedding's backward
def run_patch_bwd(env, family, case, with_dimg=True):
    spf, L = env
    b, c, p, grid, dim, t0, splits = case
    side, g, k = grid * p, grid * grid, c * p * p
    m = b * g
    assert spf.dense_tile(family, 1, m, dim, k)[2] == splits
    seed = 1000 * b + 10 * grid + dim + t0
    img, w = E.randn((b, c, side, side), seed, DEV), E.randn((dim, k), seed + 1, DEV, 0.02)
    dtok = E.randn((b, t0 + g, dim), seed + 2, DEV, 0.1)
    img_b, w_b, dtok_b = operand(img), operand(w), operand(dtok)
    ws_bytes = int(getattr(L, f"ftx_vit_patch_embed_bwd_{family}_workspace_bytes")(b, c, side, side, p, dim))
    ws_whole, ws = GD.banded_bytes(ws_bytes, device=DEV)
    dw, dbias, dcls, dpos = Out((dim, k)), Out((dim,)), Out((dim,)), Out((t0 + g, dim))
    ddist = Out((dim,)) if t0 == 2 else None
    dimg = Out((b, c, side, side)) if with_dimg else None
    call(env, "ftx_vit_patch_embed_bwd_" + family, dtok_b.data_ptr(), img_b.data_ptr(), w_b.data_ptr(), b, c, side, side, p, dim, t0, dw.address,
         dbias.address, dcls.address, ddist.address if ddist else 0, dpos.address, dimg.address if dimg else 0, GD.address(ws_whole, ws), ws_bytes)
    what = ("patch bwd", family) + case
    assert GD.bands_intact(ws_whole, ws), (what, "the workspace was used beyond the size its query returns")
    # the materialised operands: dY the strip rows, A the unfold
    dy = dev(strip_np(dtok.cpu().numpy(), t0))
    a = dev(unfold_np(img.cpu().numpy(), p))
    assert GD.same_bits(dw.checked(what), spf._dense_wgrad(dy, a, family)), (what, "dW differs from the plain entry on strip rows and unfold")
    frames = dtok[0].clone()
    for f in range(1, b):
        frames += dtok[f]                                   # fp32, frames ascending
    assert GD.same_bits(dpos.checked(what), frames), (what, "dpos is not the ordered sum over the frames")
    assert GD.same_bits(dbias.checked(what), spf.colsum(frames[t0:].contiguous())), (what, "dbias is not ftx_colsum of dpos' patch rows")
    assert GD.same_bits(dcls.checked(what), frames[0]) and (t0 == 1 or GD.same_bits(ddist.checked(what), frames[1])), what
    out = dict(dw=dw.view, dbias=dbias.view, dy=dy, a=a, dtok=dtok, w=w, splits=splits)
    if with_dimg:
        dx, _ = spf._dense_gemm(dy, w, 1, spf.EPI_NONE, mode=family)          # dY W, W stored (dim, c p p) = [K][N]
        folded = dev(fold_np(dx.cpu().numpy(), b, c, side, side, p))
        # `checked`: every pixel was written; equal to the fold, a bijection (host test): every pixel exactly once
        assert GD.same_bits(dimg.checked(what), folded), (what, "dimg differs from the fold of the plain data gradient")
        out.update(dimg=dimg.view, dx=dx)
    return out


@pytest.mark.parametrize("case", PATCH_CASES, ids=_id)
@pytest.mark.parametrize("family", FAMILIES)
def test_patch_embed_bwd_is_the_plain_entries_on_materialised_operands(env, family, case):
    b, c, p, grid, dim, t0, splits = case
    r = run_patch_bwd(env, family, case)
    gate = Gate()
    try:
        gt = r["dy"].t().contiguous()
        s, sa = E.gemm_ref(family, gt, r["a"])
        gate("dW", r["dw"], s, E.wgrad_factor(family, b * grid * grid, splits) * U * sa)
        s, sa = E.gemm_ref(family, r["dy"], r["w"])
        folded = lambda t: dev(fold_np(t.cpu().numpy(), b, c, grid * p, grid * p, p))      # noqa: E731
        gate("dimg", r["dimg"], folded(s), folded(E.factor(family, dim) * U * sa))
        # dbias: b - 1 fp32 additions per element of dpos, then float64 column sums rounded once: (b + 1) roundings of the magnitudes
        d64 = r["dtok"].double()[:, t0:]
        gate("dbias", r["dbias"], d64.sum((0, 1)), (b + 1) * U * d64.abs().sum((0, 1)))
    finally:
        gate.record("patch bwd %s %s" % (family, _id(case)))


@pytest.mark.parametrize("family", FAMILIES)
def test_patch_embed_bwd_without_the_image_gradient_writes_none(env, family):
    r = run_patch_bwd(env, family, PATCH_CASES[2], with_dimg=False)
    full = run_patch_bwd(env, family, PATCH_CASES[2])
    assert GD.same_bits(r["dw"], full["dw"]) and GD.same_bits(r["dbias"], full["dbias"])


# ---------------------------------------------------------------- 1 + 2. the tap stem
def tap_data(case):
    b, g, t0, dim, co, splits = case
    seed = 100 * b + g + 7 * t0 + dim + co
    tokens = E.randn((b, t0 + g, dim), seed, DEV)
    w, bias = E.randn((co, dim), seed + 1, DEV, 0.05), E.randn((co,), seed + 2, DEV, 0.5)
    return tokens, w, bias


def run_tap_fwd(env, family, case):
    spf, L = env
    b, g, t0, dim, co, splits = case
    tokens, w, bias = tap_data(case)
    rows = Out((b * g, co))
    banded = [operand(t) for t in (tokens, w, bias)]      # kept alive over the call
    call(env, "ftx_vit_tap_stem_train_fwd_" + family, *[t.data_ptr() for t in banded], b, g, t0, dim, co, rows.address)
    what = ("tap fwd", family) + case
    a = dev(strip_np(tokens.cpu().numpy(), t0))
    y, _ = spf._dense_gemm(a, w, 0, spf.EPI_BIAS, bias=bias, mode=family)
    assert GD.same_bits(rows.checked(what), torch.where(y < 0, torch.zeros_like(y), y)), (what, "rows differ from the plain entry and a ReLU")
    return tokens, w, bias, a, rows.view


@pytest.mark.parametrize("case", TAP_CASES, ids=_id)
@pytest.mark.parametrize("family", FAMILIES)
def test_tap_stem_train_fwd_is_the_plain_gemm_on_the_strip(env, family, case):
    b, g, t0, dim, co, splits = case
    tokens, w, bias, a, rows = run_tap_fwd(env, family, case)
    gate = Gate()
    try:
        s, sa = E.gemm_ref(family, a, w.t())
        pre, bound = E.bias_ref(s, sa, bias, E.factor(family, dim))
        # ReLU is 1-Lipschitz (tests/dense_edges.py tap_ref)
        gate("rows", rows, pre.clamp_min(0), bound)
        assert (rows == 0).any() and (rows > 0).any(), "the data exercises both sides of the ReLU"
    finally:
        gate.record("tap fwd %s %s" % (family, _id(case)))


@pytest.mark.parametrize("case", TAP_CASES, ids=_id)
@pytest.mark.parametrize("family", FAMILIES)
def test_tap_stem_bwd_is_the_plain_entries_on_the_masked_gradient(env, family, case):
    spf, L = env
    b, g, t0, dim, co, splits = case
    m = b * g
    assert spf.dense_tile(family, 1, m, co, dim)[2] == splits
    tokens, w, bias, a, rows = run_tap_fwd(env, family, case)
    rows = rows.clone()
    # the mask's three cases beside y > 0: exact zeros (the ReLU's own), a negative and a NaN in the saved output
    assert (rows == 0).any()
    rows[0, 0], rows[m - 1, co - 1], rows[m // 2, 1] = float("nan"), -1.0, -0.0
    drows = E.randn((m, co), m + co, DEV, 0.1)
    ws_bytes = int(getattr(L, f"ftx_vit_tap_stem_bwd_{family}_workspace_bytes")(b, g, dim, co))
    ws_whole, ws = GD.banded_bytes(ws_bytes, device=DEV)
    dw, dbias, dtok = Out((co, dim)), Out((co,)), Out((b, t0 + g, dim))
    banded = [operand(t) for t in (drows, rows, tokens, w)]      # kept alive over the call
    call(env, "ftx_vit_tap_stem_bwd_" + family, *[t.data_ptr() for t in banded], b, g, t0, dim, co, dw.address, dbias.address, dtok.address,
         GD.address(ws_whole, ws), ws_bytes)
    what = ("tap bwd", family) + case
    assert GD.bands_intact(ws_whole, ws), (what, "the workspace was used beyond the size its query returns")
    gm = torch.where(rows > 0, drows, torch.zeros_like(drows))                 # a select: 0 where rows is 0, negative or NaN
    assert gm[0, 0] == 0 and gm[m - 1, co - 1] == 0 and torch.isfinite(gm).all()
    assert GD.same_bits(dw.checked(what), spf._dense_wgrad(gm, a, family)), (what, "dW differs from the plain entry on the masked gradient")
    assert GD.same_bits(dbias.checked(what), spf.colsum(gm)), (what, "dbias is not ftx_colsum of the masked gradient")
    prod = torch.empty((m, dim), device=DEV)
    call(env, "ftx_rows_gemm_" + family, gm.data_ptr(), m, w.data_ptr(), 0, 0, co, dim, prod.data_ptr())
    got = dtok.checked(what)
    assert GD.same_bits(got, dev(strip_store_np(prod.cpu().numpy(), b, t0, g))), (what, "dtokens differ from the rows GEMM and the strip store")
    assert t0 == 0 or bool((got[:, :t0].view(torch.int32) == 0).all()), (what, "the leading rows are not exactly zero")
    gate = Gate()
    try:
        s, sa = E.gemm_ref(family, gm.t().contiguous(), a)
        gate("dW", dw.view, s, E.wgrad_factor(family, m, splits) * U * sa)
        s, sa = E.gemm_ref(family, gm, w)
        gate("dtokens", got[:, t0:].reshape(m, dim), s, E.factor(family, co) * U * sa)
    finally:
        gate.record("tap bwd %s %s" % (family, _id(case)))


# ---------------------------------------------------------------- the autograd nodes
@pytest.mark.parametrize("family", FAMILIES)
def test_nodes_return_the_entries_results_for_every_gradient_subset(env, family):
    spf, L = env
    b, c, p, grid, dim, t0, _ = PATCH_CASES[2]
    g, side = grid * grid, grid * p
    img = E.randn((b, c, side, side), 1, DEV)
    w, bias = E.randn((dim, c, p, p), 2, DEV, 0.02), E.randn((dim,), 3, DEV, 0.1)
    cls, dist, pos = E.randn((1, 1, dim), 4, DEV, 0.02), E.randn((1, 1, dim), 5, DEV, 0.02), E.randn((1, t0 + g, dim), 6, DEV, 0.02)
    gout = E.randn((b, t0 + g, dim), 7, DEV, 0.1)

    def run(need):
        leaves = [t.clone().requires_grad_(i in need) for i, t in enumerate((img, w, bias, cls, dist, pos))]
        out = spf.vit_patch_embed(*leaves, mode=family)
        grads = torch.autograd.grad(out, [leaves[i] for i in need], gout)
        return out.detach(), dict(zip(need, grads))
    out, full = run((0, 1, 2, 3, 4, 5))
    a = dev(unfold_np(img.cpu().numpy(), p))
    y, _ = spf._dense_gemm(a, w.view(dim, -1), 0, spf.EPI_BIAS, bias=bias, mode=family)
    assert GD.same_bits(out[:, t0:], y.view(b, g, dim) + pos[0, t0:].unsqueeze(0))
    assert GD.same_bits(out[:, 0], (cls + pos[:, 0]).view(1, dim).expand(b, dim)) and GD.same_bits(out[:, 1], (dist + pos[:, 1]).view(1, dim).expand(b, dim))
    assert [tuple(full[i].shape) for i in range(6)] == [tuple(t.shape) for t in (img, w, bias, cls, dist, pos)]
    for need in ((1,), (0,), (2, 5), (3, 4), (1, 2, 3, 4, 5)):
        o, got = run(need)
        assert GD.same_bits(o, out) and all(GD.same_bits(got[i], full[i]) for i in need), need
    tokens = out.clone()
    sw, sb = E.randn((96, dim, 1, 1), 8, DEV, 0.05), E.randn((96,), 9, DEV, 0.5)
    grow = E.randn((b * g, 96), 10, DEV, 0.1)

    def tap(need):
        leaves = [t.clone().requires_grad_(i in need) for i, t in enumerate((tokens, sw, sb))]
        rows = spf.vit_tap_stem(*leaves, t0=t0, mode=family)
        return rows.detach(), dict(zip(need, torch.autograd.grad(rows, [leaves[i] for i in need], grow)))
    rows, full = tap((0, 1, 2))
    assert [tuple(full[i].shape) for i in range(3)] == [tuple(t.shape) for t in (tokens, sw, sb)]
    assert bool((full[0][:, :t0] == 0).all())
    for need in ((0,), (1,), (2,), (1, 2)):
        o, got = tap(need)
        assert GD.same_bits(o, rows) and all(GD.same_bits(got[i], full[i]) for i in need), need
    with pytest.raises(ValueError):
        spf.vit_tap_stem(tokens, sw[:, :32], sb, t0=t0, mode=family)
    with pytest.raises(ValueError):
        spf.vit_patch_embed(img[:, :, :-4], w, bias, cls, dist, pos, mode=family)


# ---------------------------------------------------------------- 3. whole models

STEM_NODES = ("_VitPatchEmbed", "_VitTapStem")


def _stem_nodes(t):
    names = _graph_nodes(t)
    return {p: sum(n.startswith(p + "Backward") for n in names) for p in STEM_NODES}


@pytest.fixture(scope="module")
def batch():
    from fusiontransformer_amd.data.synth import make_batch
    return make_batch([0, 1], max_points=2500)


def _within_the_gates(what, on, off, loss_on, loss_off, logit_on, logit_off):
    """Loss, logits, every gradient and the BatchNorm buffers of one step with the switch on against the switch off, at the gates and
    with the floor of tests/test_single_modality_train_gpu.py (_judge), the switch-off model standing where the oracle stands there."""
    err = (logit_on.double() - logit_off.double()).abs().max().item()
    g_off = dict(off.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in g_off.values() if p.grad is not None)
    rows = []
    for name, p in on.named_parameters():
        q = g_off[name]
        assert (p.grad is None) == (q.grad is None), (what, name)
        if q.grad is not None:
            floor = 1e-4 * gmax * q.numel() ** 0.5
            rows.append(((p.grad.double() - q.grad.double()).norm().item() / max(q.grad.double().norm().item(), floor), name))
    rows.sort(reverse=True)
    b_off = dict(off.named_buffers())
    bn = max([(v.double() - b_off[k].double()).abs().max().item() for k, v in on.named_buffers() if v.dtype.is_floating_point] or [0.0])
    print("%s on vs off: logit %.3e (gate %.0e) loss %.3e (gate %.0e) grad %.3e %s (gate %.0e) bn %.3e (gate %.0e)"
          % (what, err, TOL_LOGIT, abs(loss_on - loss_off), TOL_LOSS, rows[0][0], rows[0][1], TOL_GRAD, bn, TOL_BN))
    assert err <= TOL_LOGIT and abs(loss_on - loss_off) < TOL_LOSS and rows[0][0] < TOL_GRAD and bn < TOL_BN, (what, err, rows[:5], bn)
    for k, v in on.named_buffers():
        assert v.dtype.is_floating_point or int(v.item()) == int(b_off[k].item()), (what, k)


def test_imagesegbilinear_step_switch_on_twice_with_the_native_trunk_and_against_switch_off(batch):
    """Four models from one seed, eager trunks: [on, on, on + image_native_train, off], one TrainStep (Adam included) each.  The first
    three agree bit for bit in everything they leave; on against off at the training-step gates."""
    from fusiontransformer_amd.trainer import TrainStep
    cfg, models = _models("image", 4)
    for m in models:
        m.image_backbone.backbone.use_graphs = False
    for m in models[:3]:
        m.image_backbone.set_native_stems(True)
    models[2].image_backbone.set_native_train(True)
    steps = [TrainStep(cfg, m) for m in models]
    preds = []
    for step in steps:
        torch.manual_seed(100)
        preds.append(step(product_inputs(batch)))
    torch.cuda.synchronize()
    for j in (1, 2):
        for k in preds[0]:
            assert same(preds[0][k], preds[j][k]), (j, k)
        for k in steps[0].last:
            assert same(steps[0].last[k], steps[j].last[k]), (j, k)
        assert _assert_same_state(models[0], models[j], ("model", j)) > 20
    for m in models[:3]:
        assert m.image_backbone.native_stems_reason() is None
    assert models[2].image_backbone.native_train_reason() is None and models[0].image_backbone.native_train_reason() == "the switch is off"
    assert models[3].image_backbone.native_stems_reason() == "the switch is off"
    for j in (0, 2):
        assert _stem_nodes(preds[j]["img_seg_logit"]) == {"_VitPatchEmbed": 1, "_VitTapStem": 1}
    assert _stem_nodes(preds[3]["img_seg_logit"]) == {"_VitPatchEmbed": 0, "_VitTapStem": 0}
    _within_the_gates("ImageSegBilinear", models[0], models[3], steps[0].last["loss_2d"].item(), steps[3].last["loss_2d"].item(),
                      preds[0]["img_seg_logit"].detach(), preds[3]["img_seg_logit"].detach())


def test_imagesegbilinear_step_with_the_switch_on_meets_the_train_step_gates():
    """tests/test_native_image_train_gpu.py's oracle test with the stems switch on: the float64 oracle, the gates of _judge."""
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    from oracle import ft_oracle as O
    from tests.test_fullsize_train_gpu import _snapshot
    from tests.test_single_modality_train_gpu import _judge
    cfg = _cfg("image", image_native_stems=True)
    torch.manual_seed(43)
    model = build_model(cfg)[0].cuda().train()
    step = TrainStep(cfg, model)
    oracle = O.Net2DBillinear(20, False, dict(cfg.MODEL)).double().train()
    cw = torch.tensor(cfg.TRAIN.CLASS_WEIGHTS).double()
    b = make_batch([0], max_points=2500)
    prefix = "image_backbone."
    pre = _snapshot(model)
    preds = step(product_inputs(b))
    torch.cuda.synchronize()
    assert model.image_backbone.native_stems_reason() is None
    oracle.load_state_dict({k[len(prefix):]: (v.double() if v.dtype.is_floating_point else v) for k, v in pre.items()})
    ref = oracle(torch.from_numpy(b["img"]).double(), b["img_indices"])
    ref_loss = F.cross_entropy(ref["img_seg_logit"], torch.from_numpy(b["seg_label"]).long(), weight=cw)
    ref_loss.backward()
    _judge("ImageSegBilinear, native stems", 0, 0, b, model, step, "loss_2d", preds["img_seg_logit"], ref["img_seg_logit"], ref_loss.item(),
           oracle, prefix, [])


def test_switch_off_and_a_library_trunk_are_the_eager_twin_bit_for_bit(batch):
    """With the switch off nothing changes, and with it on over vit_linear_impl="library" nothing engages: both equal the eager twin
    that never heard of the switch, and the reason names the cause."""
    cfg, (off, twin) = _models("image", 2)
    for m in (off, twin):
        m.image_backbone.backbone.use_graphs = False
    off.image_backbone.set_native_stems(False)
    preds = _steps(cfg, [off, twin], [batch])
    assert off.image_backbone.native_stems_reason() == "the switch is off"
    assert _stem_nodes(preds[0]["img_seg_logit"]) == {"_VitPatchEmbed": 0, "_VitTapStem": 0}
    cfg, (lib, twin) = _models("image", 2, vit_linear_impl="library")
    for m in (lib, twin):
        m.image_backbone.backbone.use_graphs = False
    lib.image_backbone.set_native_stems(True)
    preds = _steps(cfg, [lib, twin], [batch])
    why = lib.image_backbone.native_stems_reason()
    assert why is not None and "vit_linear_impl is 'library'" in why, why
    assert _stem_nodes(preds[0]["img_seg_logit"]) == {"_VitPatchEmbed": 0, "_VitTapStem": 0}


def test_imageseg_step_switch_on_twice_and_against_switch_off():
    """Net2DSeg, narrow and two blocks deep (tests/test_native_image_train_gpu.py): the trunk's input carries the gradient of stn_down's
    theta, so the embedding's backward writes the image gradient through the fold."""
    from tests.test_stn_loc_gpu import _small_model
    B, H, W, n = 2, 48, 80, 300
    g = torch.Generator().manual_seed(22)
    img = torch.randn((B, 3, H, W), generator=g).cuda()
    idx = torch.stack([torch.randint(0, H, (B * n,), generator=g), torch.randint(0, W, (B * n,), generator=g)], 1)
    per_frame = [idx[i * n:(i + 1) * n].numpy() for i in range(B)]
    label = torch.randint(0, 20, (B * n,), generator=g).cuda()
    runs = []
    for stems, native in ((True, False), (True, False), (True, True), (False, False)):
        m = _small_model(21, vit_linear_impl="ftx_split", image_native_stems=stems, image_native_train=native, stn_loc_impl="ftx").cuda().train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        out = m(img, per_frame)
        loss = F.cross_entropy(out["img_seg_logit"], label)
        loss.backward()
        opt.step()
        runs.append((m, out, loss.item()))
    (on, out_on, loss_on), (again, out_again, _), (nat, out_nat, _), (off, out_off, loss_off) = runs
    assert on.native_stems_reason() is None and nat.native_stems_reason() is None and off.native_stems_reason() == "the switch is off"
    assert nat.native_train_reason() is None
    assert _stem_nodes(out_on["img_seg_logit"])["_VitPatchEmbed"] == 1 and _stem_nodes(out_off["img_seg_logit"])["_VitPatchEmbed"] == 0
    for twin, out in ((again, out_again), (nat, out_nat)):
        assert same(out_on["img_seg_logit"], out["img_seg_logit"])
        assert _assert_same_state(on, twin, "ImageSeg") > 30
    for name, p in on.named_parameters():
        if name.startswith("stn_down."):
            assert p.grad is not None and float(p.grad.abs().max()) > 0, name
    _within_the_gates("ImageSeg", on, off, loss_on, loss_off, out_on["img_seg_logit"].detach(), out_off["img_seg_logit"].detach())
