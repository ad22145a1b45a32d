"""bf16-operand attention (ftx_attn_fwd_bf16 / ftx_attn_bwd_bf16, attn_impl="ftx_bf16") against its precision contract.

"Rounded reference" = the fp64 formula of test_ops_gpu.test_attention_matches_timm_formula on qkv and grad_out rounded through
torch.bfloat16 (round-to-nearest-even, as the kernels round).  The kernels also round P (as the P.V operand) and dS (as the dK / dQ
operand) to bf16; the reference does not, which is what the bars below absorb.  Measured on an MI355X at (2, 578, 12), scale 1/8:
max |out - ref| 6.4e-4, relative L2 of dQ / dK / dV 1.7e-3 / 1.7e-3 / 1.7e-3; lse within 1.4e-7 relative of the rounded reference and
2.9e-4 from the unrounded fp64 lse (1.9e-4 at scale 0.1).  Large logits (scores ~ +-7000): out 1.3e-4, dQ / dK / dV 1.9e-3 / 1.9e-3 / 1.8e-4.

Those two constants (OUT_TOL, GRAD_TOL) cannot see one wrong key or one wrong tile (tests/test_attn_bf16_host.py shows a case they
accept).  test_bf16_matches_the_rounded_float64_inside_the_bars holds out, lse, dQ, dK and dV at every tile edge and under every
tiling to bars computed at run time from a yardstick: the contract stated unfused in float64 (tests/attn_ref.py: yardstick_bf16,
bar_bf16, CaseBf16, with the derivation).  No tolerance of those tests is a number in this file.  Measured on an MI355X:
profiles/attn_bf16_accuracy.txt."""
import functools

import numpy as np
import pytest
import torch

from tests import attn_ref as R
from tests.helpers import oracle_inputs, product_inputs, small_cfg

pytestmark = pytest.mark.gpu

TILINGS = [(0, 0), (4, 2), (2, 2), (2, 4), (1, 2), (1, 4), (1, 8)]
OUT_TOL = 1e-2      # max-abs of out against the rounded reference
GRAD_TOL = 1e-2     # relative L2 of dQ, dK, dV against the rounded reference


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


rounded = R.rounded      # bf16 round-to-nearest-even, as float64


def reference(qkv64, go64, scale):
    """fp64 timm formula: out, lse (B, H, T), grad_qkv."""
    B, T, _, H, D = qkv64.shape
    r = qkv64.clone().requires_grad_(True)
    q, k, v = r.permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * scale
    lse = torch.logsumexp(s, dim=-1)
    out = (s.softmax(dim=-1) @ v).transpose(1, 2).reshape(B, T, H * D)
    out.backward(go64)
    return out.detach(), lse.detach(), r.grad


def run_bf16(qkv, go, scale, tiling=(0, 0)):
    """The two C entries directly (the autograd function hides lse): out, lse, grad_qkv."""
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd._lib import check, ptr, stream
    L = _lib.load()
    B, T, _, H, D = qkv.shape
    x, g = dev(qkv), dev(go)
    out = torch.empty((B, T, H * D), device="cuda")
    lse = torch.empty((B, H, T), device="cuda")
    gqkv = torch.empty_like(x)
    ws_bytes = int(L.ftx_attn_bwd_workspace_bytes(B, T, H))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    check(L.ftx_attn_fwd_bf16(ptr(x), B, T, H, D, float(scale), ptr(out), ptr(lse), tiling[0], tiling[1], stream()), "fwd")
    check(L.ftx_attn_bwd_bf16(ptr(x), ptr(out), ptr(g), ptr(lse), B, T, H, D, float(scale), ptr(gqkv), ptr(ws), ws_bytes,
                              tiling[0], tiling[1], stream()), "bwd")
    torch.cuda.synchronize()
    return out.cpu().double(), lse.cpu().double(), gqkv.cpu().double()


def rel_l2(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def check_against_rounded(qkv, go, scale, tiling=(0, 0)):
    out, lse, gq = run_bf16(qkv, go, scale, tiling)
    ref_out, ref_lse, ref_g = reference(rounded(qkv), rounded(go), scale)
    assert torch.isfinite(out).all() and torch.isfinite(lse).all() and torch.isfinite(gq).all()
    err_out = float((out - ref_out).abs().max())
    errs = [rel_l2(gq[:, :, i], ref_g[:, :, i]) for i in range(3)]
    assert err_out <= OUT_TOL, (tiling, err_out)
    assert max(errs) <= GRAD_TOL, (tiling, errs)
    return out, lse, gq, (ref_out, ref_lse, ref_g), err_out, errs


def test_lse_pins_the_operand_rounding():
    """lse is the fp32-accurate log-sum-exp of scores of bf16 operands: Q and K rounded from their stored values, the scale applied to
    the fp32 score afterwards.  scale 0.1 (not a power of two): a scale folded into Q before rounding would move lse by ~1e-3."""
    rng = np.random.default_rng(20)
    B, T, H = 2, 578, 12
    qkv = rng.standard_normal((B, T, 3, H, 64)).astype(np.float32)
    go = rng.standard_normal((B, T, H * 64)).astype(np.float32)
    for scale in (0.1, 64 ** -0.5):
        _, lse, _ = run_bf16(qkv, go, scale)
        _, lse_r, _ = reference(rounded(qkv), rounded(go), scale)
        _, lse_u, _ = reference(torch.from_numpy(qkv).double(), torch.from_numpy(go).double(), scale)
        err_r = float(((lse - lse_r).abs() / lse_r.abs().clamp_min(1.0)).max())
        err_u = float(((lse - lse_u).abs() / lse_u.abs().clamp_min(1.0)).max())
        assert err_r <= 2e-5, (scale, err_r)
        assert err_u > 2 * 2e-5 and err_u > 100 * err_r, (scale, err_u, err_r)   # clearly not the lse of the unrounded operands


def test_output_and_gradients_match_the_rounded_reference():
    rng = np.random.default_rng(21)
    B, T, H = 2, 578, 12
    qkv = rng.standard_normal((B, T, 3, H, 64)).astype(np.float32)
    go = rng.standard_normal((B, T, H * 64)).astype(np.float32)
    out, _, _, _, err_out, errs = check_against_rounded(qkv, go, 64 ** -0.5)
    # the mode engages: the fp32 kernel's output is measurably different
    from fusiontransformer_amd import functional as spf
    out32 = spf.attention(dev(qkv), 64 ** -0.5).cpu().double()
    assert float((out - out32).abs().max()) > 1e-5


@pytest.mark.parametrize("tiling", TILINGS)
def test_every_tiling_on_ragged_shapes(tiling):
    """Every built tiling and the automatic choice, on 70 tokens (2 full tiles + 6 rows: some key groups of the wide splits get no
    tile) and on the ViT's 578 tokens (4 * 128 + 66)."""
    rng = np.random.default_rng(22)
    for B, T, H in [(1, 70, 2), (1, 578, 3)]:
        qkv = rng.standard_normal((B, T, 3, H, 64)).astype(np.float32)
        go = rng.standard_normal((B, T, H * 64)).astype(np.float32)
        check_against_rounded(qkv, go, 0.125, tiling)


def test_unbuilt_tiling_is_refused():
    from fusiontransformer_amd import functional as spf
    with pytest.raises(RuntimeError, match="not a built tiling"):
        spf.attention(dev(np.zeros((1, 70, 3, 2, 64), np.float32)), 0.125, tiling=(3, 2), bf16=True)


def test_large_logits_are_stable():
    """Scores around +-7000 (test_ops_gpu.test_attention_large_logits_are_stable): the online softmax must not overflow, and the
    gradients of a saturated softmax stay within the bars (delta uses the rounded dO, see attn_delta_bf16_kernel)."""
    rng = np.random.default_rng(11)
    qkv = rng.standard_normal((1, 100, 3, 2, 64)).astype(np.float32)
    qkv[:, :, :2] *= 30.0
    go = rng.standard_normal((1, 100, 128)).astype(np.float32)
    check_against_rounded(qkv, go, 0.125)


def test_deterministic_run_to_run():
    rng = np.random.default_rng(23)
    qkv = rng.standard_normal((2, 578, 3, 4, 64)).astype(np.float32)
    go = rng.standard_normal((2, 578, 256)).astype(np.float32)
    for tiling in ((0, 0), (1, 8)):
        a, b = run_bf16(qkv, go, 0.125, tiling), run_bf16(qkv, go, 0.125, tiling)
        for x, y in zip(a, b):
            assert torch.equal(x, y), tiling


def test_autograd_path_logs_bf16_launches():
    from fusiontransformer_amd import functional as spf
    rng = np.random.default_rng(24)
    qkv = rng.standard_normal((1, 70, 3, 2, 64)).astype(np.float32)
    go = rng.standard_normal((1, 70, 128)).astype(np.float32)
    spf.LAUNCH_LOG = []
    try:
        x = dev(qkv).requires_grad_(True)
        out = spf.attention(x, 0.125, bf16=True)
        out.backward(dev(go))
        torch.cuda.synchronize()
        log = list(spf.LAUNCH_LOG)
    finally:
        spf.LAUNCH_LOG = None
    assert [k for k, *_ in log] == ["attn_fwd_bf16", "attn_bwd_bf16"]
    for _, _, _, meta in log:
        assert set(meta) == {"b", "t", "h", "d", "products"}
    ref_out, ref_lse, ref_g = run_bf16(qkv, go, 0.125)
    assert torch.equal(out.detach().cpu().double(), ref_out) and torch.equal(x.grad.cpu().double(), ref_g)


# ---------------------------------------------------------------- against the rounded float64, inside the yardstick's bars
@functools.lru_cache(maxsize=None)
def _case_bf16(kind, T, scale, b, h):
    return R.CaseBf16(kind, b, T, h, scale)


def case_bf16(kind, T, scale=0.125, b=2, h=3):
    """Inputs, rounded float64 reference, yardstick and bars: computed once and shared by every tiling (and by
    tests/test_attn_fp32_gpu.py)."""
    return _case_bf16(kind, T, scale, b, h)


def assert_inside_bf16_bars(c, got, label):
    assert all(bool(torch.isfinite(x).all()) for x in got), label
    r, E = c.ratios(got)
    print(R.format_row(f"bf16 {label} max|lse|={c.max_lse:.0f}", c.E_bar, E, r))
    assert R.worst(r) <= 1.0, (label, r, E)


@pytest.mark.parametrize("tiling", TILINGS)
@pytest.mark.parametrize("kind,T,scale", R.ACCURACY + [("large", T, 0.125) for T in R.LARGE_T])
def test_bf16_matches_the_rounded_float64_inside_the_bars(kind, T, scale, tiling):
    """out, lse, dQ, dK, dV at B = 2, H = 3: flat and peaked softmax rows at every tile edge, a scale that is no power of two, a
    running maximum that rises in every tile, a dominant key in the ragged tile, and scores around +-7000 (|lse| up to ~5000)."""
    c = case_bf16(kind, T, scale)
    assert_inside_bf16_bars(c, run_bf16(c.qkv, c.go, scale, tiling), f"acc {kind} T={T} scale={scale} tiling={tiling}")


def test_bf16_autograd_path_is_the_same_launch():
    """functional.attention(..., bf16=True) (what the model calls) gives bit for bit what the C entries give, so the bars hold for it."""
    from fusiontransformer_amd import functional as spf
    c = case_bf16("peaked", 129)
    x = dev(c.qkv).requires_grad_(True)
    out = spf.attention(x, 0.125, bf16=True)
    out.backward(dev(c.go))
    direct = run_bf16(c.qkv, c.go, 0.125)
    bits = lambda t: t.float().contiguous().view(torch.int32)        # run_bf16 widened float32 results: narrowing is exact
    assert torch.equal(bits(out.detach().cpu()), bits(direct[0])) and torch.equal(bits(x.grad.cpu()), bits(direct[2]))
    assert_inside_bf16_bars(c, (out.detach().cpu(), direct[1], x.grad.cpu()), "functional.attention peaked T=129")


# ---------------------------------------------------------------- model level
def _model(seed, bf16_attention=True):
    from fusiontransformer_amd.models.build import build_model
    from oracle import ft_oracle as O
    cfg = small_cfg("middle")
    torch.manual_seed(seed)
    oracle = O.build_model(dict(cfg.MODEL))
    if bf16_attention:
        cfg.MODEL.attn_impl = "ftx_bf16"
    model, _, _ = build_model(cfg)
    model.load_state_dict(oracle.state_dict())
    model.image_backbone.backbone.set_bf16(True)
    return cfg, oracle, model.cuda()


def test_bf16_trunk_stays_close_to_the_fp32_oracle():
    """set_bf16(True) + attn_impl="ftx_bf16": every GEMM and the attention on bf16 operands.  Bars of the bf16 mode
    (test_model_gpu.test_bf16_forward_mode_stays_close_to_the_fp32_oracle): image logits 3e-2, LiDAR logits 2e-2."""
    from fusiontransformer_amd.data.synth import make_batch
    cfg, oracle, model = _model(1)
    vit = model.image_backbone.backbone
    assert all(blk.attn.attn_impl == "ftx_bf16" for blk in vit.blocks)
    batch = make_batch([0, 1], max_points=2500)
    oracle.eval(); model.eval()
    with torch.no_grad():
        ref = oracle(oracle_inputs(batch))
        out = model(product_inputs(batch))     # the forward-only eval graph
    err = {k: (out[k].cpu() - ref[k]).abs().max().item() for k in ref}
    assert err["img_seg_logit"] <= 3e-2 and err["lidar_seg_logit"] <= 2e-2, err


def test_bf16_trunk_launches_only_bf16_attention():
    """Eagerly (a captured graph logs its launches once, at capture): every attention launch is the bf16 kernel."""
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.data.synth import make_batch
    cfg, oracle, model = _model(2)
    model.image_backbone.backbone.use_graphs = False
    model.eval()
    pin = product_inputs(make_batch([0], max_points=1500))
    spf.LAUNCH_LOG = []
    try:
        with torch.no_grad():
            model(pin)
        torch.cuda.synchronize()
        kinds = [k for k, *_ in spf.LAUNCH_LOG]
    finally:
        spf.LAUNCH_LOG = None
    attn = [k for k in kinds if k.startswith("attn_")]
    assert attn and set(attn) == {"attn_fwd_bf16"}, attn
    assert len(attn) == len(model.image_backbone.backbone.blocks)


def test_graphed_two_stream_step_is_bit_identical_to_eager_twin():
    """bench.py's selfcheck for this mode: a training step with the graphed trunk on two streams against an eager-trunk, one-stream
    twin with the same parameters: logits and every gradient bit for bit (capturing step and a replay)."""
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.trainer import fusion_losses
    pin = product_inputs(make_batch([2, 3], max_points=3000))

    def run(graphs, steps):
        cfg, oracle, model = _model(5)
        model.train()
        vit = model.image_backbone.backbone
        vit.use_graphs = graphs
        model.overlap_branches = graphs
        res = []
        for _ in range(steps):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(0)
            out = model(pin)
            l2, l3 = fusion_losses(out, pin["seg_label"], None, 0.1, True)
            (l2 + l3).backward()
            torch.cuda.synchronize()
            res.append(({k: v.detach().clone() for k, v in out.items()}, {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}))
        if graphs:
            assert vit.__dict__.get("_graph_cache") and all(v is not None for v in vit._graph_cache.values()), "the trunk was not captured"
            assert all(key[6][i][0] == "ftx_bf16" for key in vit._graph_cache for i in range(len(vit.blocks)))
        return res

    graphed = run(True, 2)
    eager = run(False, 1)[0]
    for outs, grads in graphed:
        for k in eager[0]:
            assert torch.equal(outs[k], eager[0][k]), k
        assert grads.keys() == eager[1].keys()
        for n in grads:
            assert torch.equal(grads[n], eager[1][n]), n
