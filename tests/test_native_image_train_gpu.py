"""The native training executor of the ViT image branch on the GPU (include/ftx.h: ftx_vit_train_fwd / ftx_vit_train_bwd;
fusiontransformer_amd/native_image_train.py): a segment against the package's chain, the arena and every output between guard bands,
whole models with the switch on against their twins, eagerly and as HIP graphs, the spatial-transformer model, the switch behind an
eager pass, the fallbacks, a second backward, the float64 oracle's training-step gates and the INTEGRATION section 3 sketch through
ctypes.  Every comparison with the package's own path is bit for bit (`same`)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import guard as GD
from tests.helpers import product_inputs, small_cfg
from tests.test_native_image_gpu import same
from tests.test_native_train_gpu import _assert_same_state, _graph_nodes

pytestmark = pytest.mark.gpu

# (vit_linear_impl, set_bf16, attn_impl) and the (linear_mode, attn_mode) the executor is handed for them
MODES = {"split-fp32": ("ftx_split", False, "ftx", (0, 0)), "split-split": ("ftx_split", False, "ftx_split", (0, 2)),
         "bf16-bf16": ("ftx", True, "ftx_bf16", (1, 1))}
# (dim, heads, b, tokens): 76 rows are a partial 64-row tile behind a full one and 38 keys a key tile with a tail; the model's shape
SHAPES = {"256": (256, 4, 2, 38), "768": (768, 12, 1, 578)}
SEGMENTS = [(0, 0), (0, 2), (1, 2)]      # the start without an addend (p is None) alone, chained blocks behind it, a start further in
TRUNK_NODES = ("_VitLinear", "_VitMlp", "_Attention", "_AddLayerNorm", "_LayerNorm", "_Materialize")


@pytest.fixture(scope="module")
def L():
    from fusiontransformer_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return _lib.load()


def _set_mode(bb, mode):
    lin, bf16, attn, _ = MODES[mode]
    bb.set_linear_impl(lin)
    bb.set_bf16(bf16)
    bb.set_attention_impl(attn)


def _bare_trunk(dim, heads, mode, depth=3, seed=0):
    """A trunk of `depth` blocks with non-zero biases and LayerNorm weights off one, in training mode on the GPU."""
    from fusiontransformer_amd.models.transformers import Image2DTransformer
    torch.manual_seed(seed)
    bb = Image2DTransformer(img_size=96, embed_dim=dim, depth=depth, num_heads=heads)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for blk in bb.blocks:
            for name, p in blk.named_parameters():
                if name.endswith("bias"):
                    p.copy_(torch.randn(p.shape, generator=g) * 0.1)
                elif name.startswith("norm"):
                    p.add_(torch.randn(p.shape, generator=g) * 0.1)
    _set_mode(bb, mode)
    return bb.cuda().train()


def _block_params(bb, first, last):
    from fusiontransformer_amd import native_image as ni
    return [t for blk in bb.blocks[first:last + 1] for t in ni.block_tensors(blk)]


def _package_segment(bb, first, last, x, gout):
    """(x_out, grad_x, the gradients of the blocks' parameters in BLOCK_FIELDS order) of blocks [first, last] run by _TrunkSegment."""
    from fusiontransformer_amd.models.transformers import _TrunkSegment
    params = _block_params(bb, first, last)
    xin = x.clone().requires_grad_(True)
    out = _TrunkSegment(bb, first, last, embed=False)(xin)
    grads = torch.autograd.grad(out, [xin] + params, gout)
    return out.detach(), grads[0], list(grads[1:])


@pytest.fixture(scope="module")
def segment_cases():
    """Per (shape, mode): the trunk, its input, the output gradient and the package's results for SEGMENTS, computed once."""
    made = {}

    def get(shape, mode):
        if (shape, mode) not in made:
            dim, heads, b, tokens = SHAPES[shape]
            bb = _bare_trunk(dim, heads, mode)
            g = torch.Generator().manual_seed(7)
            x = torch.randn((b, tokens, dim), generator=g).cuda()
            gout = (torch.randn((b, tokens, dim), generator=g) * 0.1).cuda()
            made[(shape, mode)] = (bb, x, gout, {seg: _package_segment(bb, seg[0], seg[1], x, gout) for seg in SEGMENTS})
        return made[(shape, mode)]
    return get


# ---------------------------------------------------------------- 1. a segment against the package's chain
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_segment_equals_the_package_chain(segment_cases, shape, mode):
    from fusiontransformer_amd import native_image as ni
    from fusiontransformer_amd.native_image_train import NativeImageTrain
    bb, x, gout, want = segment_cases(shape, mode)
    ex = NativeImageTrain(bb)
    assert ex.ready()[2:] == MODES[mode][3]
    for first, last in SEGMENTS:
        ref_out, ref_gx, ref_grads = want[(first, last)]
        params = _block_params(bb, first, last)
        xin = x.clone().requires_grad_(True)
        out = ex.segment(xin, first, last)
        assert [n for n in _graph_nodes(out) if n.startswith("_")] == ["_VitSegmentBackward"]
        grads = torch.autograd.grad(out, [xin] + params, gout)
        what = (shape, mode, first, last)
        assert same(out.detach(), ref_out), (what, "x_out", (out - ref_out).abs().max().item())
        assert same(grads[0], ref_gx), (what, "grad_x", (grads[0] - ref_gx).abs().max().item())
        names = [(i, f) for i in range(first, last + 1) for f in ni.BLOCK_FIELDS]
        assert len(grads) - 1 == len(names) == 12 * (last - first + 1)
        for (i, f), mine, ref in zip(names, grads[1:], ref_grads):
            assert mine.shape == ref.shape and same(mine, ref), (what, "block", i, f, (mine - ref).abs().max().item())
            assert float(ref.abs().max()) > 0, (what, i, f)
    assert ex.runs == len(SEGMENTS)


# ---------------------------------------------------------------- 2. + 9. the C entries called directly
def _c_tables(bb, tokens):
    from fusiontransformer_amd import native_image as ni
    from fusiontransformer_amd import native_image_train as nit
    keep = []
    return nit.model_record(bb, tokens), ni.block_table(bb, ni.keeper(keep)), keep


def _c_segment(L, bb, x, gout, first, last, modes, alloc, arena_of):
    """INTEGRATION section 3, "training the trunk from C", call for call through ctypes: the tables, ftx_vit_train_arena_bytes,
    ftx_vit_train_fwd, ftx_vit_train_bwd into one buffer per gradient, ftx_vit_train_release.  alloc(name, shape) -> an output tensor,
    arena_of(nbytes) -> the arena's address.  Returns (x_out, grad_in, {(block, field): gradient}, the call of the backward, the arena's address)."""
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import native_image as ni
    b, tokens, dim = x.shape
    model, blocks, keep = _c_tables(bb, tokens)
    vp = ctypes.c_void_p
    need = L.ftx_vit_train_arena_bytes(ni._ptr(model), len(blocks), first, last, b)
    assert need > 0 and need % 256 == 0, L.ftx_last_error()
    arena = arena_of(need)
    x_out, grad_in = alloc("x_out", x.shape), alloc("grad_in", x.shape)
    grads_tab = np.zeros(len(blocks), dtype=ni.BLOCK)
    grads = {}
    for i in range(first, last + 1):
        for f, p in zip(ni.BLOCK_FIELDS, ni.block_tensors(bb.blocks[i])):
            grads[(i, f)] = alloc("grad %d %s" % (i, f), p.shape)
            grads_tab[i][f] = grads[(i, f)].data_ptr()
    st = _lib.stream()
    lm, am = modes
    _lib.check(L.ftx_vit_train_fwd(ni._ptr(model), ni._ptr(blocks), len(blocks), b, vp(x.data_ptr()), first, last, lm, am, vp(x_out.data_ptr()), vp(arena),
                                   need, st), "ftx_vit_train_fwd")

    def backward():
        return L.ftx_vit_train_bwd(ni._ptr(model), ni._ptr(blocks), ni._ptr(grads_tab), len(blocks), b, vp(x.data_ptr()), vp(gout.data_ptr()), first, last,
                                   lm, am, vp(grad_in.data_ptr()), vp(arena), need, st)
    _lib.check(backward(), "ftx_vit_train_bwd")
    torch.cuda.synchronize()
    return x_out, grad_in, grads, backward, arena


@pytest.mark.parametrize("mode", list(MODES))
def test_arena_poisoned_and_every_output_between_guard_bands(L, segment_cases, mode):
    """The arena holds NaN before the forward and is exactly ftx_vit_train_arena_bytes long; x_out, grad_in and every gradient buffer
    (one allocation each, so the LayerNorm's parameter gradients take the way through the arena) lie between sentinel bands."""
    bb, x, gout, want = segment_cases("256", mode)
    first, last = 0, 2
    ref_out, ref_gx, ref_grads = want[(first, last)]
    banded, arenas = {}, []

    def alloc(name, shape):
        banded[name] = GD.banded(shape)
        return banded[name][1]

    def arena_of(nbytes):
        whole, payload = GD.banded_bytes(nbytes)
        payload.view(torch.float32).fill_(float("nan"))
        arenas.append((whole, payload))
        return GD.address(whole, payload)

    x_out, grad_in, grads, _, arena = _c_segment(L, bb, x, gout, first, last, MODES[mode][3], alloc, arena_of)
    assert L.ftx_vit_train_release(ctypes.c_void_p(arena)) == 0
    assert GD.bands_intact(*arenas[0]), "a guard band of the arena was written"
    for name, (whole, view) in banded.items():
        assert GD.bands_intact(whole, view), "a guard band of %s was written" % name
        assert GD.written(view), "%s: an element was not written, or depends on memory nobody wrote" % name
    from fusiontransformer_amd import native_image as ni
    assert same(x_out, ref_out) and same(grad_in, ref_gx)
    names = [(i, f) for i in range(first, last + 1) for f in ni.BLOCK_FIELDS]
    for key, ref in zip(names, ref_grads):
        assert same(grads[key], ref), (mode, key)


def test_integration_training_sketch_through_ctypes(L, segment_cases):
    """Plain buffers, blocks [1, 2]; a second ftx_vit_train_bwd and one behind the release are refused on the host."""
    from fusiontransformer_amd import native_image as ni
    bb, x, gout, want = segment_cases("256", "split-split")
    first, last = 1, 2
    ref_out, ref_gx, ref_grads = want[(first, last)]
    held = []

    def arena_of(nbytes):
        held.append(torch.empty((nbytes,), dtype=torch.uint8, device="cuda"))
        return held[0].data_ptr()

    x_out, grad_in, grads, backward, arena = _c_segment(L, bb, x, gout, first, last, (0, 2), lambda name, shape: torch.empty(shape, device="cuda"), arena_of)
    assert same(x_out, ref_out) and same(grad_in, ref_gx)
    for key, ref in zip([(i, f) for i in range(first, last + 1) for f in ni.BLOCK_FIELDS], ref_grads):
        assert same(grads[key], ref), key
    before = {k: v.clone() for k, v in grads.items()}
    assert backward() == -1 and "has run already" in L.ftx_last_error().decode()
    assert L.ftx_vit_train_release(ctypes.c_void_p(arena)) == 0
    assert backward() == -1 and "no forward" in L.ftx_last_error().decode()
    torch.cuda.synchronize()
    assert all(same(grads[k], before[k]) for k in grads) and same(grad_in, ref_gx)


# ---------------------------------------------------------------- 3. whole models against their twins
@pytest.fixture(scope="module")
def batches():
    from fusiontransformer_amd.data.synth import make_batch
    return [make_batch([0, 1], max_points=2500), make_batch([2, 3], max_points=2000)]


def _cfg(kind, **model_kw):
    """small_cfg of tests/helpers.py: `middle` with depth 3 (taps 0 and 2), or ImageSegBilinear as the image branch of `late`, depth 2."""
    cfg = small_cfg("middle", depth=3) if kind == "middle" else small_cfg("late")
    if kind == "image":
        cfg.MODEL.USE_FUSION, cfg.MODEL.USE_LIDAR, cfg.MODEL.TYPE, cfg.MODEL.DUAL_HEAD = False, False, "ImageSegBilinear", False
        cfg.TRAIN.FusionTransformer.lambda_xm = 0.0
    cfg.MODEL.vit_linear_impl = "ftx_split"
    for k, v in model_kw.items():
        cfg.MODEL[k] = v
    return cfg


def _models(kind, n, seed=5, **model_kw):
    """n models from one seed on the GPU in training mode, with non-zero biases in the trunk."""
    from fusiontransformer_amd.models.build import build_model
    cfg = _cfg(kind, **model_kw)
    torch.manual_seed(seed)
    models = [build_model(cfg)[0] for _ in range(n)]
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in models[0].image_backbone.backbone.blocks.named_parameters():
            if name.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    for m in models[1:]:
        m.load_state_dict(models[0].state_dict())
    return cfg, [m.cuda().train() for m in models]


def _steps(cfg, models, plan, seed=100):
    """TrainStep steps over the batches of `plan` on every model; after each step everything the models[1:] leave equals models[0]'s
    bit for bit.  Returns the last predictions per model."""
    from fusiontransformer_amd.trainer import TrainStep
    steps = [TrainStep(cfg, m) for m in models]
    preds = None
    for s, batch in enumerate(plan):
        preds = []
        for m, step in zip(models, steps):
            torch.manual_seed(seed + s)      # the LiDAR branch's Dropout
            preds.append(step(product_inputs(batch)))
        torch.cuda.synchronize()
        for j in range(1, len(models)):
            what = ("model", j, "step", s)
            assert preds[0].keys() == preds[j].keys() and steps[0].last.keys() == steps[j].last.keys()
            for k in preds[0]:
                assert same(preds[0][k], preds[j][k]), (what, k, (preds[0][k] - preds[j][k]).abs().max().item())
            for k in steps[0].last:
                assert same(steps[0].last[k], steps[j].last[k]), (what, k)
            assert _assert_same_state(models[0], models[j], what) > 20
    return preds


def _trunk_nodes(names):
    return {p: sum(n.startswith(p + "Backward") for n in names) for p in TRUNK_NODES + ("_VitSegment",)}


@pytest.mark.parametrize("kind,segments", [("image", 1), ("middle", 2)])
def test_switch_on_equals_the_eager_and_the_graphed_twin(kind, segments, batches):
    """The graphed twin goes first in every step: its capture then comes before any eager pass of the step."""
    cfg, (graphed, model, eager) = _models(kind, 3)
    net = model.image_backbone
    net.set_native_train(True)
    eager.image_backbone.backbone.use_graphs = False
    assert graphed.image_backbone.backbone.use_graphs and graphed.image_backbone.backbone.graph_taps
    preds = _steps(cfg, [graphed, model, eager], batches)
    assert net.native_train_reason() is None and eager.image_backbone.native_train_reason() == "the switch is off"
    assert graphed.image_backbone.backbone.graph_state() == "on", "the graphed twin did not run as HIP graphs"
    ex = net.backbone.__dict__["_native_tr"]
    assert ex.runs == segments * len(batches) and ex.last_arena_bytes > 0
    mine, theirs = _trunk_nodes(_graph_nodes(preds[1]["img_seg_logit"])), _trunk_nodes(_graph_nodes(preds[2]["img_seg_logit"]))
    depth = len(net.backbone.blocks)
    assert mine["_VitSegment"] == segments and theirs["_VitSegment"] == 0
    assert all(mine[p] == 0 for p in ("_VitMlp", "_Attention", "_AddLayerNorm", "_LayerNorm", "_Materialize")), mine
    assert theirs["_VitMlp"] == theirs["_Attention"] == depth and theirs["_VitLinear"] - mine["_VitLinear"] == 2 * depth, (mine, theirs)


# ---------------------------------------------------------------- 4. the spatial-transformer model
def test_imageseg_delivers_the_gradient_of_its_input():
    """Net2DSeg, narrow and two blocks deep: the trunk's input carries the gradient of stn_down's theta.  stn_loc_impl="ftx": the
    localisation nets' convolutions on the library's own kernels, whose gradients repeat bit for bit; the weight gradients of torch's
    convolutions differ in the last bits between two runs of the SAME model with the switch off (measured on an MI355X: up to 1.4e-9
    on all four localisation convolutions, the trunk's input gradient being equal), so they cannot witness anything here."""
    from tests.test_stn_loc_gpu import _small_model
    B, H, W, n = 2, 48, 80, 300
    g = torch.Generator().manual_seed(22)
    img = torch.randn((B, 3, H, W), generator=g).cuda()
    idx = torch.stack([torch.randint(0, H, (B * n,), generator=g), torch.randint(0, W, (B * n,), generator=g)], 1)
    per_frame = [idx[i * n:(i + 1) * n].numpy() for i in range(B)]
    label = torch.randint(0, 20, (B * n,), generator=g).cuda()
    models = []
    for on in (True, False):
        m = _small_model(21, vit_linear_impl="ftx_split", image_native_train=on, stn_loc_impl="ftx").cuda().train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3)
        out = m(img, per_frame)
        F.cross_entropy(out["img_seg_logit"], label).backward()
        opt.step()
        models.append((m, out))
    (on, out_on), (off, out_off) = models
    assert on.native_train_reason() is None and off.native_train_reason() == "the switch is off"
    assert on.backbone.__dict__["_native_tr"].runs == 2      # graph_taps is not set: every block is a segment
    assert same(out_on["img_seg_logit"], out_off["img_seg_logit"])
    assert _assert_same_state(on, off, "ImageSeg") > 30
    for name, p in on.named_parameters():
        if name.startswith("stn_down."):
            assert p.grad is not None and float(p.grad.abs().max()) > 0, name


# ---------------------------------------------------------------- 5. behind an eager pass
def test_switch_engages_behind_an_eager_training_step(batches):
    cfg, (model, twin) = _models("image", 2)
    for m in (model, twin):
        m.image_backbone.backbone.use_graphs = False
    _steps(cfg, [model, twin], batches[:1])
    assert model.image_backbone.native_train_reason() == "the switch is off"
    model.image_backbone.set_native_train(True)
    preds = _steps(cfg, [model, twin], batches[1:], seed=200)
    assert model.image_backbone.native_train_reason() is None
    assert _trunk_nodes(_graph_nodes(preds[0]["img_seg_logit"]))["_VitSegment"] == 1


# ---------------------------------------------------------------- 6. fallbacks
FALLBACKS = {"eval mode": "eval mode", "no_grad": "gradients are disabled", "library linears": "vit_linear_impl='library'",
             "a frozen parameter": "frozen", "torch attention": "attn_impl ['torch']"}


@pytest.mark.parametrize("case", list(FALLBACKS))
def test_fallbacks_leave_the_existing_path_alone(case, batches):
    kw = dict(vit_linear_impl="library") if case == "library linears" else dict(attn_impl="torch") if case == "torch attention" else {}
    cfg, (model, twin) = _models("image", 2, **kw)
    model.image_backbone.set_native_train(True)
    for m in (model, twin):
        m.image_backbone.backbone.use_graphs = False      # the existing path here: the eager trunk
    if case == "a frozen parameter":
        for m in (model, twin):
            m.image_backbone.backbone.blocks[1].norm2.bias.requires_grad_(False)
    if case in ("eval mode", "no_grad"):
        if case == "eval mode":
            model.eval(), twin.eval()
        with torch.no_grad():
            outs = [m(product_inputs(batches[0])) for m in (model, twin)]
        assert all(same(outs[0][k], outs[1][k]) for k in outs[0])
    else:
        preds = _steps(cfg, [model, twin], batches[:1])
        assert _trunk_nodes(_graph_nodes(preds[0]["img_seg_logit"]))["_VitSegment"] == 0
    why = model.image_backbone.native_train_reason()
    assert why is not None and FALLBACKS[case] in why, why
    assert model.image_backbone.backbone.__dict__.get("_native_tr") is None or model.image_backbone.backbone.__dict__["_native_tr"].runs == 0


# ---------------------------------------------------------------- 7. a second backward
def test_a_second_backward_on_a_retained_graph_raises(segment_cases):
    from fusiontransformer_amd.native_image_train import NativeImageTrain
    bb, x, gout, want = segment_cases("256", "split-fp32")
    ex = NativeImageTrain(bb)
    params = _block_params(bb, 0, 2)
    xin = x.clone().requires_grad_(True)
    out = ex.segment(xin, 0, 2)
    first = torch.autograd.grad(out, [xin] + params, gout, retain_graph=True)
    kept = [t.clone() for t in first]
    with pytest.raises(RuntimeError, match="second backward needs a second forward"):
        torch.autograd.grad(out, [xin] + params, gout, retain_graph=True)
    torch.cuda.synchronize()
    assert all(same(a, b) for a, b in zip(first, kept))
    assert same(first[0], want[(0, 2)][1])


# ---------------------------------------------------------------- 8. the float64 oracle's training-step gates
def test_imagesegbilinear_step_with_the_switch_on_meets_the_train_step_gates():
    """The method and the gates of tests/test_single_modality_train_gpu.py (its _judge), one step, two blocks deep."""
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    from oracle import ft_oracle as O
    from tests.test_fullsize_train_gpu import _snapshot
    from tests.test_single_modality_train_gpu import _judge
    cfg = _cfg("image", image_native_train=True)
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
    assert model.image_backbone.native_train_reason() is None
    oracle.load_state_dict({k[len(prefix):]: (v.double() if v.dtype.is_floating_point else v) for k, v in pre.items()})
    ref = oracle(torch.from_numpy(b["img"]).double(), b["img_indices"])
    ref_loss = F.cross_entropy(ref["img_seg_logit"], torch.from_numpy(b["seg_label"]).long(), weight=cw)
    ref_loss.backward()
    _judge("ImageSegBilinear, native training executor", 0, 0, b, model, step, "loss_2d", preds["img_seg_logit"], ref["img_seg_logit"], ref_loss.item(),
           oracle, prefix, [])
