"""The fp32-accurate attention kernels on the bf16 MFMA (ftx_attn_fwd_split / ftx_attn_bwd_split, attn_impl="ftx_split": every operand
in three bf16 pieces, six piece products; contract in include/ftx.h) against float64, inside the bars of the fp32 kernels: attn_ref.Case
(...).bars, bit for bit what tests/test_attn_fp32_gpu.py holds ftx_attn_fwd_tiled / ftx_attn_bwd_tiled to.  No tolerance of the kernel
tests is a number in this file.  Then the structure the other two families are held to (slices, guard bands, run to run, the automatic
tiling, the autograd path), and the model: a trunk with attn_impl="ftx_split" and vit_linear_impl="ftx_split" at the default path's
gates, and the native image executor with ATTN_SPLIT.

The family builds its own set of tilings (ftx_attn_split_tiling_built), per direction.  Every test walks the six tilings of the fp32
family: where the split family builds one for a direction it runs it, where it does not the entry must refuse it and that direction
runs the automatic choice.  Measured on an MI355X: profiles/attn_split_accuracy.txt."""
import numpy as np
import pytest
import torch

from tests import attn_ref as R
from tests.helpers import oracle_inputs, product_inputs, small_cfg
from tests.test_attn_fp32_gpu import B, EXPLICIT, H, _banded, _bands_intact, assert_inside_bars, bitwise_equal, case

pytestmark = pytest.mark.gpu

AUTOMATIC = (0, 0)
TILINGS = [AUTOMATIC] + EXPLICIT


def lib():
    from fusiontransformer_amd import _lib
    return _lib.load()


def built(tiling, backward):
    return tiling == AUTOMATIC or bool(lib().ftx_attn_split_tiling_built(tiling[0], tiling[1], int(backward)))


def launch(qkv, go, scale, fwd=AUTOMATIC, bwd=None, banded=False):
    """The two C entries directly, as tests/test_attn_fp32_gpu.launch: float32 CPU tensors out, lse, grad_qkv."""
    from fusiontransformer_amd._lib import check, ptr, stream
    L = lib()
    bwd = fwd if bwd is None else bwd
    Bq, T, _, Hq, D = qkv.shape
    if banded:
        (_, x), (_, g) = _banded(qkv.shape, qkv), _banded(go.shape, go)
        (w_out, out), (w_lse, lse), (w_gq, gq) = _banded((Bq, T, Hq * D)), _banded((Bq, Hq, T)), _banded(qkv.shape)
    else:
        x, g = torch.from_numpy(qkv).cuda(), torch.from_numpy(go).cuda()
        out, lse, gq = torch.empty((Bq, T, Hq * D), device="cuda"), torch.empty((Bq, Hq, T), device="cuda"), torch.empty_like(x)
    ws_bytes = int(L.ftx_attn_bwd_workspace_bytes(Bq, T, Hq))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    check(L.ftx_attn_fwd_split(ptr(x), Bq, T, Hq, D, float(scale), ptr(out), ptr(lse), fwd[0], fwd[1], stream()), "fwd")
    check(L.ftx_attn_bwd_split(ptr(x), ptr(out), ptr(g), ptr(lse), Bq, T, Hq, D, float(scale), ptr(gq), ptr(ws), ws_bytes, bwd[0], bwd[1],
                               stream()), "bwd")
    torch.cuda.synchronize()
    res = (out.cpu(), lse.cpu(), gq.cpu())
    return (res, all(_bands_intact(w) for w in (w_out, w_lse, w_gq))) if banded else res


def directions(tiling):
    """(forward tiling, backward tiling) of a test at `tiling`: the tiling where the family builds it, the automatic choice where not."""
    return tuple(tiling if built(tiling, d) else AUTOMATIC for d in (False, True))


def label(what, tiling):
    f, b = directions(tiling)
    return f"split {what} tiling={tiling}" + ("" if (f, b) == (tiling, tiling) else f" (runs fwd {f} bwd {b})")


# ---------------------------------------------------------------- the built set
def test_built_set_meets_the_minimum_and_the_rest_is_refused():
    L = lib()
    sets = {d: [t for t in EXPLICIT if built(t, d)] for d in (False, True)}
    print("split attention, built tilings: forward", sets[False], "backward", sets[True])
    for d, s in sets.items():
        assert (4, 2) in s and any(qw == 2 for qw, _ in s) and any(qw == 1 for qw, _ in s), (d, s)
    assert not L.ftx_attn_split_tiling_built(0, 0, 0), "(0, 0) is the automatic choice, not a tiling"
    c = case("gauss", 33, 0.125, 1, H)
    for qw, split in [(3, 2), (4, 4), (8, 1), (1, 16), (0, 2), (-1, 2)]:
        assert not L.ftx_attn_split_tiling_built(qw, split, 0) and not L.ftx_attn_split_tiling_built(qw, split, 1)
    for t in [(3, 2), (4, 4)] + [t for t in EXPLICIT if not built(t, False)]:
        with pytest.raises(RuntimeError, match="ftx_attn_fwd_split.*not a built tiling"):
            launch(c.qkv, c.go, 0.125, t, AUTOMATIC)
    for t in [(3, 2), (4, 4)] + [t for t in EXPLICIT if not built(t, True)]:
        with pytest.raises(RuntimeError, match="ftx_attn_bwd_split.*not a built tiling"):
            launch(c.qkv, c.go, 0.125, AUTOMATIC, t)


# ---------------------------------------------------------------- accuracy: the fp32 bars
@pytest.mark.parametrize("tiling", TILINGS)
@pytest.mark.parametrize("kind,T,scale", R.ACCURACY + [("large", T, 0.125) for T in R.LARGE_T])
def test_split_matches_float64_inside_the_fp32_bars(kind, T, scale, tiling):
    """out, lse, dQ, dK, dV at B = 2, H = 3 on the cases of the fp32 kernels: flat and peaked softmax rows at every tile edge, a scale
    that is no power of two, a running maximum that rises in every tile, a dominant key in the ragged tile, scores around +-7000."""
    c = case(kind, T, scale)
    fwd, bwd = directions(tiling)
    assert_inside_bars(c, launch(c.qkv, c.go, scale, fwd, bwd), label(f"acc {kind} T={T} scale={scale}", tiling))


def test_split_autograd_path_is_the_same_launch():
    """functional.attention(..., operands="split") (what the model calls) gives bit for bit what the C entries give, and logs its kinds."""
    from fusiontransformer_amd import functional as spf
    c = case("peaked", 129)
    x = torch.from_numpy(c.qkv).cuda().requires_grad_(True)
    spf.LAUNCH_LOG = []
    try:
        out = spf.attention(x, 0.125, operands="split")
        out.backward(torch.from_numpy(c.go).cuda())
        torch.cuda.synchronize()
        log = list(spf.LAUNCH_LOG)
    finally:
        spf.LAUNCH_LOG = None
    assert [k for k, *_ in log] == ["attn_fwd_split", "attn_bwd_split"]
    direct = launch(c.qkv, c.go, 0.125)
    assert bitwise_equal((out.detach().cpu(), x.grad.cpu()), (direct[0], direct[2]))
    assert_inside_bars(c, (out.detach().cpu(), direct[1], x.grad.cpu()), "split functional.attention peaked T=129")
    # an explicit tiling travels to both entries
    t = (4, 2)
    y = torch.from_numpy(c.qkv).cuda().requires_grad_(True)
    spf.attention(y, 0.125, tiling=t, operands="split").backward(torch.from_numpy(c.go).cuda())
    assert bitwise_equal((y.grad.cpu(),), (launch(c.qkv, c.go, 0.125, t)[2],))
    # the mode engages: not the bits of the fp32 kernels
    assert not bitwise_equal((out.detach().cpu(),), (spf.attention(x.detach(), 0.125).cpu(),))


# ---------------------------------------------------------------- structure
@pytest.mark.parametrize("tiling", EXPLICIT)
@pytest.mark.parametrize("T", [33, 129])
def test_slices_are_independent_bitwise(T, tiling):
    """Slice (b, h) of a (2, T, 3 heads) launch equals the (1, T, 1 head) launch of that slice bit for bit."""
    c = case("peaked", T)
    fwd, bwd = (tiling if built(tiling, d) else (4, 2) for d in (False, True))      # explicit both ways: the automatic choice follows the shape
    out, lse, gq = launch(c.qkv, c.go, 0.125, fwd, bwd)
    for b in range(B):
        for h in range(H):
            one = launch(np.ascontiguousarray(c.qkv[b:b + 1, :, :, h:h + 1]), np.ascontiguousarray(c.go[b:b + 1, :, 64 * h:64 * h + 64]),
                         0.125, fwd, bwd)
            assert bitwise_equal(one, (out[b:b + 1, :, 64 * h:64 * h + 64], lse[b:b + 1, h:h + 1], gq[b:b + 1, :, :, h:h + 1])), (b, h)


@pytest.mark.parametrize("tiling", TILINGS)
@pytest.mark.parametrize("T", [1, 33, 70])
def test_guard_bands(T, tiling):
    """Operands between NaN bands, outputs between sentinel bands: nothing outside an operand is read or written, the result is bit for
    bit the unbanded one and inside the bars."""
    c = case("gauss", T, 0.125, 1, H)
    fwd, bwd = directions(tiling)
    got, intact = launch(c.qkv, c.go, 0.125, fwd, bwd, banded=True)
    assert intact, "a guard band of an output was written"
    assert_inside_bars(c, got, label(f"banded T={T}", tiling))
    assert bitwise_equal(got, launch(c.qkv, c.go, 0.125, fwd, bwd))


@pytest.mark.parametrize("tiling", [AUTOMATIC, (1, 8), (4, 2)])
def test_deterministic_run_to_run(tiling):
    qkv, go = R.make_inputs("gauss", 2, 578, 4)
    fwd, bwd = directions(tiling)
    assert bitwise_equal(launch(qkv, go, 0.125, fwd, bwd), launch(qkv, go, 0.125, fwd, bwd))


# The family's automatic choice (csrc/ftx_attn.hip, AttnSplitFamily::config), wave-tiles = ceil(T / 32) * H * B against the 1024 SIMDs.
# Forward: <= 256 one wave per group, <= 512 two, above four, as the other families, with the key groups the LDS holds (four; two with
# four waves).  Backward: (2,2) at every size, the built tiling without scratch that won or tied at every batch measured.  Shapes as
# tests/test_attn_fp32_gpu.AUTO: four on the thresholds, four with the same counts and enough tiles for another split to give other bits.
AUTO = [((16, 33, 8), (1, 4), (2, 2)),       # 256
        ((257, 1, 1), (2, 4), (2, 2)),       # 257
        ((16, 33, 16), (2, 4), (2, 2)),      # 512
        ((19, 1, 27), (4, 2), (2, 2)),       # 513
        ((4, 250, 8), (1, 4), (2, 2)),       # 256
        ((1, 8200, 1), (2, 4), (2, 2)),      # 257
        ((8, 250, 8), (2, 4), (2, 2)),       # 512
        ((9, 70, 19), (4, 2), (2, 2))]       # 513


@pytest.mark.parametrize("shape,fwd,bwd", AUTO)
def test_automatic_choice_is_the_documented_tiling(shape, fwd, bwd):
    b, T, h = shape
    assert -(-T // 32) * h * b in (256, 257, 512, 513)
    assert built(fwd, False) and built(bwd, True)
    qkv, go = R.make_inputs("gauss", b, T, h)
    auto = launch(qkv, go, 0.125)
    assert bitwise_equal(auto, launch(qkv, go, 0.125, fwd, bwd))
    if T >= 70:     # another split is another order of the same sums: other bits
        for other in EXPLICIT:
            if other[1] != fwd[1] and built(other, False):
                assert not bitwise_equal(auto[:2], launch(qkv, go, 0.125, other, bwd)[:2]), other
            if other[1] != bwd[1] and built(other, True):
                assert not bitwise_equal(auto[2:], launch(qkv, go, 0.125, fwd, other)[2:]), other


# ---------------------------------------------------------------- model level: the fp32 model with no fp32 MFMA in the trunk
def _model(seed, impl="ftx_split"):
    """tests/test_vit_linear_split_gpu._model with the attention switched as well; `impl` is the Linears' (that test's argument)."""
    from fusiontransformer_amd.models.build import build_model
    from oracle import ft_oracle as O
    cfg = small_cfg("middle")
    torch.manual_seed(seed)
    oracle = O.build_model(dict(cfg.MODEL))
    cfg.MODEL.vit_linear_impl = impl
    cfg.MODEL.attn_impl = "ftx_split"
    model, _, _ = build_model(cfg)
    model.load_state_dict(oracle.state_dict())
    vit = model.image_backbone.backbone
    assert all(blk.attn.attn_impl == "ftx_split" for blk in vit.blocks)
    return cfg, oracle, model.cuda()


def test_eval_logits_match_the_oracle_at_the_fp32_gate():
    """The default path's gate (tests/test_model_gpu.test_eval_logits_match_oracle: 1e-3 on both heads), and every attention launch of the
    trunk is the split kernel."""
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.data.synth import make_batch
    from tests.test_vit_linear_split_gpu import TOL
    batch = make_batch([0, 1], max_points=2500)
    cfg, oracle, model = _model(0)
    model.image_backbone.backbone.use_graphs = False      # eagerly: a captured graph logs its launches once, at capture
    model.image_backbone.backbone.eval_graphs = False
    oracle.eval(); model.eval()
    spf.LAUNCH_LOG = []
    try:
        with torch.no_grad():
            ref = oracle(oracle_inputs(batch))
            out = model(product_inputs(batch))
        torch.cuda.synchronize()
        kinds = [k for k, *_ in spf.LAUNCH_LOG]
    finally:
        spf.LAUNCH_LOG = None
    attn = [k for k in kinds if k.startswith("attn_")]
    assert attn and set(attn) == {"attn_fwd_split"} and len(attn) == len(model.image_backbone.backbone.blocks), attn
    errs = {k: (out[k].cpu() - ref[k]).abs().max().item() for k in ref}
    print("eval logits, attn_impl = vit_linear_impl = ftx_split, max abs error against the CPU oracle:", errs)
    for k, err in errs.items():
        assert err <= TOL, (k, errs)


def test_train_step_matches_the_oracle(monkeypatch):
    """tests/test_vit_linear_split_gpu.test_train_step_matches_the_oracle itself -- its shapes, its gates -- on a model whose attention is
    split as well."""
    from tests import test_vit_linear_split_gpu as V
    monkeypatch.setattr(V, "_model", _model)
    V.test_train_step_matches_the_oracle()


def test_native_image_executor_runs_the_split_attention_bit_for_bit():
    """ftx_vit_eval with attn_mode = ATTN_SPLIT against the package trunk (the switch off) with attn_impl = "ftx_split", as
    tests/test_native_image_gpu.test_executor_equals_the_package_trunk has it for the other modes: from the embedded tokens, every tap
    bit for bit the tap stem of the trunk's tokens.  The executor issues the launches the package trunk issues."""
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd import native_image as ni
    from tests.test_native_image_gpu import CO, GRID, SIDE, C, _image_net, _stem_of_tokens, rnd, same
    depth, b = 3, 2
    net = _image_net("middle", depth, "split")
    bb = net.backbone
    x = rnd(torch.Generator().manual_seed(5), b, C, SIDE, SIDE)
    model, blocks, taps, _ = ni.emit(net)
    arena = torch.empty(ni.arena_bytes(model, len(blocks), b), dtype=torch.uint8, device="cuda")
    outs = {}
    for impl in ("ftx", "ftx_split"):
        bb.set_attention_impl(impl)
        with torch.no_grad():
            tokens_in = bb._embed(x).contiguous()
            ref = bb.forward_blocks(x)
        lin, att = ni.modes(net)
        assert (lin, att) == (ni.LINEAR_SPLIT, ni.ATTN_SPLIT if impl == "ftx_split" else ni.ATTN_FP32)
        outs[impl] = [torch.full((b, GRID, GRID, CO), float("nan"), device="cuda") for _ in taps]
        ni.eval_call(model, blocks, taps, b, None, tokens_in, 0, depth - 1, lin, att, outs[impl], arena)
        for t, o in zip(taps, outs[impl]):
            key = str(int(t["block"]))
            want = _stem_of_tokens(spf, _lib.load(), net, key, ref[key], "split")
            assert same(o, want), (impl, key, (o - want).abs().max().item())
    assert not same(outs["ftx"][-1], outs["ftx_split"][-1]), "the mode engages: other bits than the fp32 attention"
    # a mode the entry does not know is refused, naming the argument
    with pytest.raises(RuntimeError, match="attn_mode"):
        ni.eval_call(model, blocks, taps, b, None, tokens_in, 0, depth - 1, lin, 3, outs["ftx"], arena)
