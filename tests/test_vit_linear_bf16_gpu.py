"""bf16-operand ViT Linears (ftx_dense_gemm_bf16 / ftx_dense_wgrad_bf16, vit_linear_impl="ftx") against their precision contract.

Each element is gated against a float64 reference computed on the bf16-ROUNDED operands (torch.bfloat16, round-to-nearest-even, as the
kernels round), with the bound  chain * 2^-24 * sum_k |a_k b_k|  (chain = the kernel's accumulation chain: the reduction length plus the
bias add, plus the split count for a split weight gradient) -- the per-element method of tests/test_spconv_regimes_gpu.py.  The GELU
epilogues add a few fp32 ulps for erf / exp.  Each gate is shown to reject the library bf16 path's output (bf16-rounded results) and a
reference with one reduction term dropped."""
import pytest
import torch

from tests.helpers import oracle_inputs, product_inputs, small_cfg

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
LINEARS = {"qkv": (768, 2304), "proj": (768, 768), "fc1": (768, 3072), "fc2": (3072, 768)}   # nn.Linear(K, N)
ROWS = [1, 33, 578, 2312, 2313, 4624]


def _spf():
    from fusiontransformer_amd import functional as spf
    return spf


def _r64(t):
    return t.to(torch.bfloat16).double()


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / 2.0 ** 0.5))


def _dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / 2.0 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2.0 * torch.pi) ** 0.5


def _data(m, k, n, seed, positive=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if positive:
        x = torch.rand(m, k, device="cuda", generator=g)
        w = torch.rand(n, k, device="cuda", generator=g) * 0.05
    else:
        x = torch.randn(m, k, device="cuda", generator=g)
        w = torch.randn(n, k, device="cuda", generator=g) * 0.02
    b = torch.randn(n, device="cuda", generator=g) * 0.1
    return x, w, b


def gemm_ref(a, b_kn):
    """float64 sum on rounded operands and sum |a b| for out = a @ b_kn (b_kn (k, n))."""
    a64, b64 = _r64(a), _r64(b_kn)
    return a64 @ b64, a64.abs() @ b64.abs()


def passes(out, ref, bound):
    return bool(((out.double() - ref).abs() <= bound).all())


def worst(out, ref, bound):
    return float(((out.double() - ref).abs() / bound.clamp_min(1e-300)).max())


def _check(out, ref, bound, what):
    assert torch.isfinite(out).all(), what
    assert passes(out, ref, bound), (what, worst(out, ref, bound))


# ---------------------------------------------------------------- kernels: every form, every shape, every tile / split at those shapes
@pytest.mark.parametrize("m", ROWS)
@pytest.mark.parametrize("name", list(LINEARS))
def test_every_form_meets_the_bound(name, m):
    spf = _spf()
    k, n = LINEARS[name]
    x, w, b = _data(m, k, n, seed=m * 7 + k + n)
    s, sa = gemm_ref(x, w.t())
    chain = k + 2
    # forward: NONE, BIAS, and BIAS_GELU where the Linear is fc1
    out, _ = spf._dense_gemm(x, w, 0, spf.EPI_NONE)
    _check(out, s, chain * U * sa, (name, m, "fwd NONE"))
    out, _ = spf._dense_gemm(x, w, 0, spf.EPI_BIAS, bias=b)
    pre_ref, pre_bound = s + b.double(), chain * U * (sa + b.double().abs())
    _check(out, pre_ref, pre_bound, (name, m, "fwd BIAS"))
    if name == "fc1":
        h, pre = spf._dense_gemm(x, w, 0, spf.EPI_BIAS_GELU, bias=b, with_pre=True)
        assert torch.equal(pre, out), "the pre-activation is the BIAS epilogue's output"
        # gelu of the fp32 pre-activation: its error through gelu' plus a few ulps of erf in fp32
        p64 = pre.double()
        _check(h, _gelu64(pre_ref), _dgelu64(pre_ref).abs() * pre_bound + 8 * U * (p64.abs() + _gelu64(p64).abs()) + 1e-30, (name, m, "fwd BIAS_GELU"))
    # data gradient dX (m, k) = dY (m, n) . W (n, k): reduction over n
    dy = torch.randn(m, n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(m + 1)) * 0.1
    dx_ref, dx_abs = gemm_ref(dy, w)
    dx, _ = spf._dense_gemm(dy, w, 1, spf.EPI_NONE)
    _check(dx, dx_ref, (n + 2) * U * dx_abs, (name, m, "dX NONE"))
    if name == "fc2":   # DGELU: fc2's dX times gelu'(fc1's pre-activation) = fc1's output gradient
        pre = torch.randn(m, k, device="cuda", generator=torch.Generator(device="cuda").manual_seed(m + 2)) * 2
        dp, _ = spf._dense_gemm(dy, w, 1, spf.EPI_DGELU, pre_in=pre)
        d64 = _dgelu64(pre.double())
        _check(dp, dx_ref * d64, (n + 2) * U * dx_abs * d64.abs() + 8 * U * dx_ref.abs() * (1 + pre.double().abs()) + 1e-30, (name, m, "dX DGELU"))
    # weight gradient dW (n, k) = dY^T X over the m rows, split as the tile query says
    splits = spf.dense_bf16_tile(1, m, n, k)[2]
    dw = spf._dense_wgrad(dy, x)
    dw_ref, dw_abs = gemm_ref(dy.t(), x)
    _check(dw, dw_ref, (-(-m // splits) + 64 + splits) * U * dw_abs, (name, m, "dW", splits))


def test_shapes_reach_every_tile_and_split():
    spf = _spf()
    tiles, splits = set(), set()
    for m in ROWS:
        for k, n in LINEARS.values():
            tiles.add(spf.dense_bf16_tile(0, m, n, k)[:2])
            tiles.add(spf.dense_bf16_tile(0, m, k, n)[:2])
            splits.add(spf.dense_bf16_tile(1, m, n, k)[2])
    assert tiles == {(64, 64), (64, 128), (128, 128)} and splits == {1, 2, 3, 8}


def test_m_zero_and_tails():
    spf = _spf()
    x, w, b = _data(0, 768, 768, 3)
    out, _ = spf._dense_gemm(x, w, 0, spf.EPI_BIAS, bias=b)
    assert out.shape == (0, 768)
    dw = spf._dense_wgrad(torch.zeros(0, 768, device="cuda"), x)
    assert torch.equal(dw, torch.zeros_like(dw))
    # output columns that are a multiple of 4 but not of the 64-column tile
    x, w, b = _data(130, 128, 68, 4)
    s, sa = gemm_ref(x, w.t())
    out, _ = spf._dense_gemm(x, w, 0, spf.EPI_BIAS, bias=b)
    _check(out, s + b.double(), 130 * U * (sa + b.double().abs()), "n tail")
    dw = spf._dense_wgrad(x[:, :68].contiguous(), x)
    r, ra = gemm_ref(x[:, :68].t(), x)
    _check(dw, r, 200 * U * ra, "wgrad n tail")


# ---------------------------------------------------------------- the gates can tell
def test_gate_rejects_library_bf16_output_and_a_dropped_term():
    spf = _spf()
    m, (k, n) = 2312, LINEARS["proj"]
    x, w, b = _data(m, k, n, seed=11, positive=True)
    s, sa = gemm_ref(x, w.t())
    bound = (k + 2) * U * sa
    out, _ = spf._dense_gemm(x, w, 0, spf.EPI_NONE)
    assert passes(out, s, bound)
    lib = (x.to(torch.bfloat16) @ w.to(torch.bfloat16).t()).float()      # the library bf16 path: a bf16 result, widened
    assert lib.dtype == torch.float32
    assert not passes(lib, s, bound), "bf16-rounded results must fail the fp32-output contract"
    mutant = s - _r64(x)[:, 100:101] * _r64(w)[:, 100].unsqueeze(0)      # reduction term k = 100 dropped
    assert not passes(out, mutant, bound)
    # the same for the weight gradient (reduction over the rows) and the data gradient
    dy = torch.rand(m, n, device="cuda") * 0.1
    dw = spf._dense_wgrad(dy, x)
    r, ra = gemm_ref(dy.t(), x)
    wb = (-(-m // 8) + 64 + 8) * U * ra
    assert passes(dw, r, wb)
    assert not passes((dy.t().to(torch.bfloat16) @ x.to(torch.bfloat16)).float(), r, wb)
    assert not passes(dw, r - _r64(dy)[1000].unsqueeze(1) * _r64(x)[1000].unsqueeze(0), wb)
    dx, _ = spf._dense_gemm(dy, w, 1, spf.EPI_NONE)
    r, ra = gemm_ref(dy, w)
    assert passes(dx, r, (n + 2) * U * ra)
    assert not passes((dy.to(torch.bfloat16) @ w.to(torch.bfloat16)).float(), r, (n + 2) * U * ra)


# ---------------------------------------------------------------- determinism
def test_repeated_launches_are_bit_identical():
    spf = _spf()
    m, (k, n) = 2313, LINEARS["fc1"]
    x, w, b = _data(m, k, n, 5)
    dy = torch.randn(m, n, device="cuda")
    first = (spf._dense_gemm(x, w, 0, spf.EPI_BIAS_GELU, bias=b, with_pre=True), spf._dense_gemm(dy, w, 1, spf.EPI_NONE)[0], spf._dense_wgrad(dy, x))
    for _ in range(3):
        again = (spf._dense_gemm(x, w, 0, spf.EPI_BIAS_GELU, bias=b, with_pre=True), spf._dense_gemm(dy, w, 1, spf.EPI_NONE)[0], spf._dense_wgrad(dy, x))
        assert torch.equal(first[0][0], again[0][0]) and torch.equal(first[0][1], again[0][1])
        assert torch.equal(first[1], again[1]) and torch.equal(first[2], again[2])


_REPLAY_CHILD = r"""
import sys, torch
sys.path.insert(0, sys.argv[1])
from fusiontransformer_amd import functional as spf
g = torch.Generator(device="cuda").manual_seed(6)
m, k, n = 2312, 768, 768      # proj at batch 4: an 8-way split weight gradient, its workspace from the graph's pool
x = torch.randn(m, k, device="cuda", generator=g)
w = torch.randn(n, k, device="cuda", generator=g) * 0.02
b = torch.randn(n, device="cuda", generator=g)
dy = torch.randn(m, n, device="cuda", generator=g)

def run():
    y, _ = spf._dense_gemm(x, w, 0, spf.EPI_BIAS, bias=b)
    return y, spf._dense_gemm(dy, w, 1, spf.EPI_NONE)[0], spf._dense_wgrad(dy, x)

eager = run()
side = torch.cuda.Stream()
side.wait_stream(torch.cuda.current_stream())
with torch.cuda.stream(side):
    run()
torch.cuda.current_stream().wait_stream(side)
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    static = run()
for _ in range(2):
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, e) for a, e in zip(static, eager)), "replay differs from the eager launch"
print("replay ok")
"""


def test_graph_replay_is_bit_identical_to_eager():
    """Captured in a fresh process, so nothing left behind by earlier tests (autograd graphs, streams, events) can be released by the
    garbage collector while the capture is open: the runtime aborts on that instead of raising."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", _REPLAY_CHILD, root], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "replay ok" in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])


# ---------------------------------------------------------------- autograd layer and fallback
def test_vit_linear_and_mlp_run_the_kernels():
    spf = _spf()
    m, k, hid = 578, 768, 3072
    x, w1, b1 = _data(m, k, hid, 7)
    _, w2, b2 = _data(1, hid, k, 8)
    xg = x.view(1, m, k).clone().requires_grad_(True)
    p = [t.clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    spf.LAUNCH_LOG = []
    try:
        y = spf.vit_mlp(xg, *p)
        go = torch.randn_like(y)
        y.backward(go)
        torch.cuda.synchronize()
        kinds = [kd for kd, *_ in spf.LAUNCH_LOG]
    finally:
        spf.LAUNCH_LOG = None
    assert kinds == ["vit_gemm_bf16"] * 2 + ["vit_gemm_bf16", "vit_wgrad_bf16", "vit_gemm_bf16", "vit_wgrad_bf16"], kinds
    # the node is exactly the kernels composed
    h, pre = spf._dense_gemm(x, w1, 0, spf.EPI_BIAS_GELU, bias=b1, with_pre=True)
    yr, _ = spf._dense_gemm(h, w2, 0, spf.EPI_BIAS, bias=b2)
    go2 = go.view(m, k)
    dpre, _ = spf._dense_gemm(go2, w2, 1, spf.EPI_DGELU, pre_in=pre)
    assert torch.equal(y.detach().view(m, k), yr)
    assert torch.equal(xg.grad.view(m, k), spf._dense_gemm(dpre, w1, 1, spf.EPI_NONE)[0])
    assert torch.equal(p[0].grad, spf._dense_wgrad(dpre, x)) and torch.equal(p[2].grad, spf._dense_wgrad(go2, h))
    assert torch.equal(p[1].grad, spf.colsum(dpre)) and torch.equal(p[3].grad, spf.colsum(go2))
    # vit_linear: forward with and without the bias
    xl = x.clone().requires_grad_(True)
    wl = w1.clone().requires_grad_(True)
    yl = spf.vit_linear(xl, wl, None)
    assert torch.equal(yl.detach(), spf._dense_gemm(x, w1, 0, spf.EPI_NONE)[0])
    yl.backward(pre)
    assert torch.equal(xl.grad, spf._dense_gemm(pre, w1, 1, spf.EPI_NONE)[0]) and torch.equal(wl.grad, spf._dense_wgrad(pre, x))


def test_refused_shapes_fall_back_to_the_library_bf16_path():
    from fusiontransformer_amd.models.transformers import _LinearFn
    spf = _spf()
    x, w, b = _data(40, 100, 68, 9)     # 100 input features: not a multiple of 64
    assert not spf.vit_linear_supported(x, w)
    outs = []
    for fn in (lambda xx, ww, bb: spf.vit_linear(xx, ww, bb), lambda xx, ww, bb: _LinearFn.apply(xx, ww, bb, True)):
        xx, ww, bb = (t.clone().requires_grad_(True) for t in (x, w, b))
        spf.LAUNCH_LOG = []
        try:
            y = fn(xx, ww, bb)
            y.backward(torch.ones_like(y))
            torch.cuda.synchronize()
            assert not [kd for kd, *_ in spf.LAUNCH_LOG if kd.startswith("vit_")]
        finally:
            spf.LAUNCH_LOG = None
        outs.append((y.detach(), xx.grad, ww.grad, bb.grad))
    for a, e in zip(*outs):
        assert torch.equal(a, e)
    _, w2, b2 = _data(1, 68, 100, 10)
    y = spf.vit_mlp(x.clone(), w, b, w2, b2)
    ref = _LinearFn.apply(torch.nn.functional.gelu(_LinearFn.apply(x, w, b, True)), w2, b2, True)
    assert torch.equal(y, ref)


# ---------------------------------------------------------------- model level
def _model(seed, impl="ftx"):
    from fusiontransformer_amd.models.build import build_model
    from oracle import ft_oracle as O
    cfg = small_cfg("middle")
    torch.manual_seed(seed)
    oracle = O.build_model(dict(cfg.MODEL))
    cfg.MODEL.vit_linear_impl = impl
    model, _, _ = build_model(cfg)
    model.load_state_dict(oracle.state_dict())
    model.image_backbone.backbone.set_bf16(True)
    return cfg, oracle, model.cuda()


def test_ftx_linears_stay_close_to_the_fp32_oracle():
    """set_bf16(True) + vit_linear_impl="ftx": the bars of test_model_gpu.test_bf16_forward_mode_stays_close_to_the_fp32_oracle
    (image logits 3e-2, LiDAR logits 2e-2), through the forward-only eval graph."""
    from fusiontransformer_amd.data.synth import make_batch
    cfg, oracle, model = _model(1)
    vit = model.image_backbone.backbone
    assert all(lin.ftx_linear_impl == "ftx" for blk in vit.blocks for lin in (blk.attn.qkv, blk.mlp.fc1))
    batch = make_batch([0, 1], max_points=2500)
    oracle.eval(); model.eval()
    with torch.no_grad():
        ref = oracle(oracle_inputs(batch))
        out = model(product_inputs(batch))
    err = {k: (out[k].cpu() - ref[k]).abs().max().item() for k in ref}
    assert err["img_seg_logit"] <= 3e-2 and err["lidar_seg_logit"] <= 2e-2, err


def test_ftx_trunk_launches_the_dense_kernels():
    """Eagerly: every block runs 3 forward GEMMs for qkv, proj and the fused MLP's two Linears, and no library bf16 GEMM."""
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.data.synth import make_batch
    cfg, oracle, model = _model(2)
    vit = model.image_backbone.backbone
    vit.use_graphs = False
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
    live = vit.last_block + 1 if vit.last_block is not None else len(vit.blocks)
    assert kinds.count("vit_gemm_bf16") == 4 * live, kinds


def test_graphed_two_stream_step_is_bit_identical_to_eager_twin():
    """bench.py's selfcheck for this mode: a training step with the graphed trunk on two streams against an eager-trunk, one-stream
    twin with the same parameters: logits and every gradient bit for bit (capturing step and a replay).  The graphed model is built
    and captured first (a capture after an eager backward is refused by the runtime, DESIGN)."""
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
            assert all([impl for impl, _ in key[6][i][1]] == ["ftx"] * 4 for key in vit._graph_cache for i in range(len(vit.blocks)))
        return res

    graphed = run(True, 2)
    eager = run(False, 1)[0]
    for outs, grads in graphed:
        for k in eager[0]:
            assert torch.equal(outs[k], eager[0][k]), k
        assert grads.keys() == eager[1].keys()
        for n in grads:
            assert torch.equal(grads[n], eager[1][n]), n
