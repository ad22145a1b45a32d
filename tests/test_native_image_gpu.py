"""The native eval path of the ViT image branch on the GPU: the patch-embedding and tap-stem forms of the dense GEMM families against
the plain entries on a materialised A, bit for bit; ftx_rows_add_bias against torch; the executor (ftx_vit_eval) against the package's
trunk bit for bit, split over calls and replayed from a HIP graph; the switch (Net2DBillinear.set_native_eval) end to end on the three
fusion models and ImageSegBilinear against the CPU oracle; and the INTEGRATION section 3 sketch through ctypes."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import split_ref as R
from tests.helpers import oracle_inputs, product_inputs, small_cfg

pytestmark = pytest.mark.gpu
TOL = 1e-3   # the project's eval gate (tests/test_model_gpu.py::test_eval_logits_match_oracle)
P, GRID, SIDE, C = 16, 24, 384, 3
G = GRID * GRID
CO = 96
EPS = float(np.float32(1e-5))


@pytest.fixture(scope="module")
def env():
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import functional as spf
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return spf, _lib.load()


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b):
    """torch.equal, and the same bit patterns (torch.equal alone takes -0.0 for 0.0)."""
    return a.shape == b.shape and torch.equal(a, b) and torch.equal(bits(a), bits(b))


def rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).cuda()


# ---------------------------------------------------------------- patch embedding
def unfold(img):
    b, c, side, _ = img.shape
    gs = side // P
    return img.reshape(b, c, gs, P, gs, P).permute(0, 2, 4, 1, 3, 5).reshape(b * gs * gs, c * P * P).contiguous()


@pytest.fixture(scope="module")
def images():
    g = torch.Generator().manual_seed(1)
    return {(b, side): rnd(g, b, C, side, side) for b, side in ((1, 384), (3, 384), (3, 80), (9, 400))}


# (b, image side, dim, t0, tile rows the launch must pick, whether the last row tile is partial).  384: the model's 24 x 24 grid, 576 rows
# per frame, the 64 x 64 tile at one and three frames.  80: 25 patches per frame, 75 rows, a partial tile behind a full one.  400 with
# nine frames: 5625 rows, the 128 x 128 tile (44 x 6 tiles >= 256) with a partial last tile.
PATCH_CASES = [(1, 384, 256, 2, 64, False), (1, 384, 768, 2, 64, False), (3, 384, 256, 2, 64, False), (3, 384, 768, 2, 64, False),
               (3, 384, 768, 1, 64, False), (3, 80, 768, 2, 64, True), (9, 400, 768, 2, 128, True)]


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("b,side,dim,t0,tile,tail", PATCH_CASES)
def test_patch_embed_equals_unfold_gemm_pos(env, images, mode, b, side, dim, t0, tile, tail):
    spf, L = env
    g = torch.Generator().manual_seed(10 * b + dim + t0 + side)
    img = images[(b, side)]
    gp = (side // P) ** 2
    w, bias = rnd(g, dim, C * P * P, scale=0.02), rnd(g, dim, scale=0.1)
    cls, dist, pos = rnd(g, dim, scale=0.02), (rnd(g, dim, scale=0.02) if t0 == 2 else None), rnd(g, t0 + gp, dim, scale=0.02)
    tm, _, _ = spf.dense_tile(mode, 0, b * gp, dim, C * P * P)
    assert tm == tile and ((b * gp) % tm != 0) == tail and b * gp > tm

    def run():
        out = torch.full((b, t0 + gp, dim), float("nan"), device="cuda")
        spf.check(getattr(L, "ftx_vit_patch_embed_" + mode)(img.data_ptr(), w.data_ptr(), bias.data_ptr(), cls.data_ptr(), spf.ptr(dist), pos.data_ptr(), b,
                                                             C, side, side, P, dim, t0, out.data_ptr(), spf.stream()), "ftx_vit_patch_embed_" + mode)
        return out
    out = run()
    a = unfold(img)
    y, _ = spf._dense_gemm(a, w, 0, spf.EPI_BIAS, bias=bias, mode=mode)
    head = [cls.view(1, 1, dim).expand(b, 1, dim)] + ([dist.view(1, 1, dim).expand(b, 1, dim)] if t0 == 2 else [])
    ref = torch.cat(head + [y.view(b, gp, dim)], dim=1) + pos.unsqueeze(0)
    assert same(out, ref), (out - ref).abs().max().item()
    assert same(run(), out), "repeated launches differ"
    if mode == "split":
        add = (bias.unsqueeze(0) + pos[t0:]).repeat(b, 1)
        e, t = R.g2_figures(out[:, t0:].reshape(b * gp, dim), a, w.t(), add)
        print(f"patch embed split b={b} side={side} dim={dim}: G2 E = {e:.3g}, T = {t:.3g}")
        assert R.g2_passes(out[:, t0:].reshape(b * gp, dim), a, w.t(), add)


# ---------------------------------------------------------------- tap stem
# (b, tokens per frame behind the t0 leading ones, dim): the model's 576 at one and three frames, and 25 (75 rows: a partial tile)
@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("b,gp,dim", [(1, G, 256), (1, G, 768), (3, G, 256), (3, G, 768), (3, 25, 768)])
def test_tap_stem_equals_gemm_relu_batchnorm(env, mode, b, gp, dim):
    spf, L = env
    g = torch.Generator().manual_seed(100 * b + dim + gp)
    t0 = 2
    tokens = rnd(g, b, t0 + gp, dim)
    w, bias = rnd(g, CO, dim, scale=0.05), rnd(g, CO, scale=0.5)
    lo, hi = 5, 9
    bias[lo], bias[hi] = -1e4, 1e4
    gamma, beta = (torch.rand(CO, generator=g) + 0.5).cuda(), rnd(g, CO, scale=0.2)
    rm, rv = rnd(g, CO, scale=0.3), (torch.rand(CO, generator=g) + 0.5).cuda()
    rm[lo], beta[lo] = 1.0, -0.3          # BatchNorm(0) of that column is negative: a ReLU behind the BatchNorm would show
    out = torch.full((b * gp, CO), float("nan"), device="cuda")
    spf.check(getattr(L, "ftx_vit_tap_stem_" + mode)(tokens.data_ptr(), w.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                                                      rv.data_ptr(), EPS, b, gp, t0, dim, CO, out.data_ptr(), spf.stream()), "ftx_vit_tap_stem_" + mode)
    a = tokens[:, t0:].contiguous().view(b * gp, dim)
    y, _ = spf._dense_gemm(a, w, 0, spf.EPI_BIAS, bias=bias, mode=mode)
    with torch.no_grad():
        ref = spf.batch_norm(torch.relu(y), gamma, beta, rm, rv, False, 0.1, EPS)
        of_zero = spf.batch_norm(torch.zeros(1, CO, device="cuda"), gamma, beta, rm, rv, False, 0.1, EPS)
    assert same(out, ref), (out - ref).abs().max().item()
    assert of_zero[0, lo].item() < 0 and bool((out[:, lo] == of_zero[0, lo]).all()), "bias -1e4: ReLU gives 0, BatchNorm(0) comes out"
    want_hi = (1e4 - rm[hi].item()) / np.sqrt(rv[hi].item() + EPS) * gamma[hi].item() + beta[hi].item()
    assert bool(((out[:, hi] - want_hi).abs() < 1e-2 * abs(want_hi)).all()), "bias +1e4 passes the ReLU and is normalised"


# ---------------------------------------------------------------- materialise
def test_rows_add_bias_equals_torch(env):
    spf, L = env
    g = torch.Generator().manual_seed(3)
    for n, c in ((1, 4), (578, 768), (1731, 256)):
        r, p, pb = rnd(g, n, c), rnd(g, n, c), rnd(g, c)
        r[0, :4] = torch.tensor([-0.0, -0.0, 0.0, 1.0])
        p[0, :4] = torch.tensor([-0.0, 0.0, -0.0, -1.0])
        pb[:4] = torch.tensor([-0.0, 0.0, -0.0, 0.0])
        out = torch.full((n, c), float("nan"), device="cuda")
        spf.check(L.ftx_rows_add_bias(r.data_ptr(), p.data_ptr(), pb.data_ptr(), n, c, out.data_ptr(), spf.stream()), "ftx_rows_add_bias")
        assert same(out, r + (p + pb))
        assert bits(out)[0, 0].item() == bits(torch.tensor([-0.0]))[0].item() and bits(out)[0, 1].item() == 0
        out.fill_(float("nan"))
        spf.check(L.ftx_rows_add_bias(r.data_ptr(), None, None, n, c, out.data_ptr(), spf.stream()), "ftx_rows_add_bias")
        assert same(out, r), "NULL p: a copy, -0.0 included"


# ---------------------------------------------------------------- the executor
def _randomise_batchnorm(model, seed):
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            c = m.running_mean.shape[0]
            m.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(c, generator=g) + 0.5)
            m.weight.data.copy_(torch.rand(c, generator=g) + 0.5)
            m.bias.data.copy_(torch.randn(c, generator=g) * 0.2)


def _image_net(kind, depth, flavour, seed=0):
    """The image branch of a small fusion model on the GPU in eval mode; flavour "split": fp32 model on the split kernels, "bf16": bf16
    linears on the library's own bf16 kernels plus bf16 attention."""
    from fusiontransformer_amd.models.build import build_model
    cfg = small_cfg(kind, depth=depth)
    if flavour == "split":
        cfg.MODEL.vit_linear_impl = "ftx_split"
    else:
        cfg.MODEL.vit_linear_impl, cfg.MODEL.vit_bf16, cfg.MODEL.attn_impl = "ftx", True, "ftx_bf16"
    torch.manual_seed(seed)
    model = build_model(cfg)[0]
    _randomise_batchnorm(model, seed + 100)
    net = model.image_backbone.cuda().eval()
    with torch.no_grad():      # biases are zero-initialised: give every bias and LayerNorm a value that a dropped or misplaced one would show
        g = torch.Generator().manual_seed(seed + 7)
        for name, prm in net.named_parameters():
            if name.endswith(".bias") and "backbone" in name:
                prm.copy_(torch.randn(prm.shape, generator=g) * 0.05)
            if "norm" in name and name.endswith(".weight"):
                prm.copy_(1 + torch.randn(prm.shape, generator=g) * 0.1)
    net.backbone.eval_graphs = False      # the package's trunk eagerly: the same kernels as its graph, without the capture
    return net


def _stem_of_tokens(spf, L, net, key, tokens, mode):
    """The tap stem entry on stripped tokens (b, G, dim): what the executor's tap output must equal when its tokens equal these."""
    from fusiontransformer_amd import native_image as ni
    b, _, dim = tokens.shape
    w, bias, gamma, beta, rm, rv = ni.tap_tensors(net.up[key])
    out = torch.empty((b, GRID, GRID, w.shape[0]), device="cuda")
    tokens = tokens.contiguous()
    spf.check(getattr(L, "ftx_vit_tap_stem_" + mode)(tokens.data_ptr(), w.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), rm.data_ptr(),
                                                      rv.data_ptr(), float(net.up[key].stem[2].eps), b, G, 0, dim, w.shape[0], out.data_ptr(), spf.stream()),
              "ftx_vit_tap_stem_" + mode)
    return out


@pytest.mark.parametrize("flavour", ["split", "bf16"])
@pytest.mark.parametrize("kind,depth", [("middle", 3), ("late", 2)])
def test_executor_equals_the_package_trunk(env, kind, depth, flavour):
    spf, L = env
    from fusiontransformer_amd import native_image as ni
    net = _image_net(kind, depth, flavour)
    bb = net.backbone
    b = 2
    x = rnd(torch.Generator().manual_seed(5), b, C, SIDE, SIDE)
    with torch.no_grad():
        tokens_in = bb._embed(x).contiguous()
        ref = bb.forward_blocks(x)
    model, blocks, taps, _ = ni.emit(net)
    lin, att = ni.modes(net)
    assert (lin, att) == ((ni.LINEAR_SPLIT, ni.ATTN_FP32) if flavour == "split" else (ni.LINEAR_BF16, ni.ATTN_BF16))
    assert [int(t["block"]) for t in taps] == ([0, 2] if kind == "middle" else [1])
    arena = torch.empty(ni.arena_bytes(model, len(blocks), b), dtype=torch.uint8, device="cuda")

    def outs():
        return [torch.full((b, GRID, GRID, CO), float("nan"), device="cuda") for _ in taps]
    whole = outs()
    ni.eval_call(model, blocks, taps, b, None, tokens_in, 0, depth - 1, lin, att, whole, arena)
    mode = "split" if flavour == "split" else "bf16"
    for t, o in zip(taps, whole):
        key = str(int(t["block"]))
        want = _stem_of_tokens(spf, L, net, key, ref[key], mode)
        assert same(o, want), (kind, flavour, key, (o - want).abs().max().item())
    # block by block on one arena: the residual state is carried by the arena
    parts = outs()
    for i in range(depth):
        n = sum(1 for t in taps if int(t["block"]) <= i)
        ni.eval_call(model, blocks, taps, b, None, tokens_in if i == 0 else None, i, i, lin, att, parts[:n], arena)
    for o, p in zip(whole, parts):
        assert same(o, p), "one call and one call per block differ"
    # continuations the arena holds no state for: a block that is not the next one, another batch size, a released arena
    with pytest.raises(RuntimeError, match="residual state is in front of block"):
        ni.eval_call(model, blocks, taps, b, None, None, 1, depth - 1, lin, att, parts, arena)
    ni.eval_call(model, blocks, taps, b, None, tokens_in, 0, 0, lin, att, parts[:sum(1 for t in taps if int(t["block"]) == 0)], arena)
    with pytest.raises(RuntimeError, match="holds no residual state for b = 1"):
        ni.eval_call(model, blocks, taps, 1, None, None, 1, depth - 1, lin, att, parts, arena)
    ni.eval_call(model, blocks, taps, b, None, tokens_in, 0, 0, lin, att, parts[:sum(1 for t in taps if int(t["block"]) == 0)], arena)
    assert L.ftx_vit_eval_release(arena.data_ptr()) == 0
    with pytest.raises(RuntimeError, match="holds no residual state for b = 2"):
        ni.eval_call(model, blocks, taps, b, None, None, 1, depth - 1, lin, att, parts, arena)
    # a misaligned tap output is refused with the tables, before anything runs: the outputs written above stay as they are
    before = [p.clone() for p in parts]
    skew = torch.empty(parts[-1].numel() + 1, device="cuda")[1:].view_as(parts[-1])
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ni.eval_call(model, blocks, taps, b, None, tokens_in, 0, depth - 1, lin, att, parts[:-1] + [skew], arena)
    torch.cuda.synchronize()
    for p, q in zip(parts, before):
        assert same(p, q)


def test_executor_from_the_image_and_as_a_hip_graph(env):
    """From the image through the patch embedding (the package has no counterpart with these bits: checked against the entries it
    chains), then the same call captured once on a side stream and replayed twice."""
    spf, L = env
    from fusiontransformer_amd import native_image as ni
    net = _image_net("middle", 3, "split", seed=2)
    bb = net.backbone
    b = 1
    x = rnd(torch.Generator().manual_seed(6), b, C, SIDE, SIDE)
    model, blocks, taps, _ = ni.emit(net)
    lin, att = ni.modes(net)
    need = ni.arena_bytes(model, len(blocks), b)
    arena = torch.empty(need, dtype=torch.uint8, device="cuda")
    eager = [torch.empty((b, GRID, GRID, CO), device="cuda") for _ in taps]
    ni.eval_call(model, blocks, taps, b, x, None, 0, 2, lin, att, eager, arena)
    tokens = torch.empty((b, 2 + G, 768), device="cuda")
    pe = bb.patch_embed.proj
    spf.check(L.ftx_vit_patch_embed_split(x.data_ptr(), pe.weight.data_ptr(), pe.bias.data_ptr(), bb.cls_token.data_ptr(), bb.dist_token.data_ptr(),
                                          bb.pos_embed.data_ptr(), b, C, SIDE, SIDE, P, 768, 2, tokens.data_ptr(), spf.stream()), "ftx_vit_patch_embed_split")
    from_tokens = [torch.empty_like(o) for o in eager]
    ni.eval_call(model, blocks, taps, b, None, tokens, 0, 2, lin, att, from_tokens, arena)
    for o, p in zip(eager, from_tokens):
        assert same(o, p)
    with torch.no_grad():
        pkg = bb._embed(x)
    print("patch embedding, split kernels against the package's library GEMM: max |diff| = %.3g" % (tokens - pkg).abs().max().item())
    assert (tokens - pkg).abs().max().item() < 1e-4
    with pytest.raises(RuntimeError, match="-3"):
        ni.eval_call(model, blocks, taps, b, x, None, 0, 2, lin, att, eager, arena[:need - 256])
    # capture
    graphed = [torch.full_like(o, float("nan")) for o in eager]
    garena = torch.empty(need, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ni.eval_call(model, blocks, taps, b, x, None, 0, 2, lin, att, graphed, garena)      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ni.eval_call(model, blocks, taps, b, x, None, 0, 2, lin, att, graphed, garena)
    for _ in range(2):
        for o in graphed:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for o, p in zip(eager, graphed):
            assert same(o, p), "the replayed graph differs from the eager call"


# ---------------------------------------------------------------- the switch, end to end
KINDS = ["middle", "early", "late", "image"]
PARITY = {}


@pytest.fixture(scope="module")
def oracle_runs():
    """Per fusion kind: (cfg, the oracle's state dict, its eval-mode outputs on the shared batch), computed once."""
    from fusiontransformer_amd.data.synth import make_batch
    from oracle import ft_oracle as O
    batch = make_batch([0, 1], max_points=2500)
    runs = {}

    def get(kind):
        if kind not in runs:
            cfg = small_cfg(kind)
            cfg.MODEL.vit_linear_impl = "ftx_split"
            torch.manual_seed(0)
            oracle = O.build_model(dict(cfg.MODEL)).eval()
            with torch.no_grad():
                ref = oracle(oracle_inputs(batch))
            runs[kind] = (cfg, oracle.state_dict(), ref)
        return runs[kind]
    return batch, get


def _product(kind, oracle_runs, **model_kw):
    """The product model of `kind` ("image": ImageSegBilinear with the image branch of the late-fusion oracle) with the oracle's weights."""
    from fusiontransformer_amd.models.build import build_model
    batch, get = oracle_runs
    cfg, sd, ref = get("late" if kind == "image" else kind)
    cfg = copy.deepcopy(cfg)      # CfgNode.clone() shares the nested nodes
    for k, v in model_kw.items():
        cfg.MODEL[k] = v
    if kind == "image":
        cfg.MODEL.USE_FUSION, cfg.MODEL.USE_LIDAR, cfg.MODEL.TYPE = False, False, "ImageSegBilinear"
        model = build_model(cfg)[0]
        model.load_state_dict({k: v for k, v in sd.items() if k.startswith("image_backbone.")})
        ref = {"img_seg_logit": ref["img_seg_logit"]}      # the one output this model returns
    else:
        model = build_model(cfg)[0]
        model.load_state_dict(sd)
    return model.cuda().eval(), ref, batch


def _worst(out, ref):
    return max((out[k].cpu() - ref[k]).abs().max().item() for k in ref)


@pytest.mark.parametrize("kind", KINDS)
def test_switch_on_matches_the_oracle_and_keeps_the_forward_contract(env, kind, oracle_runs, monkeypatch):
    spf, _ = env
    from fusiontransformer_amd import native_image as ni
    from fusiontransformer_amd.models import image_models_billinear as ib
    from fusiontransformer_amd.models import transformers as tr
    model, ref, batch = _product(kind, oracle_runs)
    net = model.image_backbone
    pin = product_inputs(batch)
    with torch.no_grad():
        off = model(pin)
    assert net.native_eval_reason() == "the switch is off"
    torch.cuda.synchronize()
    # the sites of the image branch's library GEMMs and the executor's calls, counted
    calls = {"patch": 0, "stem": 0, "eval": 0}
    events = []
    pe_forward, stem_forward, eval_call = tr.PatchEmbed.forward, ib.BilinearModule.forward_tokens, ni.eval_call
    monkeypatch.setattr(tr.PatchEmbed, "forward", lambda self, x: (calls.__setitem__("patch", calls["patch"] + 1), pe_forward(self, x))[1])
    monkeypatch.setattr(ib.BilinearModule, "forward_tokens", lambda self, t, g: (calls.__setitem__("stem", calls["stem"] + 1), stem_forward(self, t, g))[1])

    def counted(*a, **k):
        calls["eval"] += 1
        events.append("eval")
        return eval_call(*a, **k)
    monkeypatch.setattr(ni, "eval_call", counted)
    net.set_native_eval(True)
    spf.LAUNCH_LOG = []
    try:
        with torch.no_grad():
            on = model(pin)
        torch.cuda.synchronize()
        kinds = [k for k, *_ in spf.LAUNCH_LOG]
    finally:
        spf.LAUNCH_LOG = None
    assert net.native_eval_reason() is None
    has_mid = net.middle_feat_block_number is not None and int(net.middle_feat_block_number) != int(net.late_feat_block_number)
    assert calls == {"patch": 0, "stem": 0, "eval": 2 if has_mid else 1}, "no library GEMM of the image branch ran"
    assert kinds.count("vit_eval") == calls["eval"] and not [k for k in kinds if k.startswith("vit_gemm") or k.startswith("attn_")]
    assert on.keys() == off.keys()
    e_on, e_off = _worst(on, ref), _worst(off, ref)
    for k in ref:
        err = (on[k].cpu() - ref[k]).abs().max().item()
        print(f"native image eval vs oracle {kind} {k}: max |diff| = {err:.3g}")
        assert err <= TOL, (kind, k, err)
    PARITY[kind] = {"switch_on": e_on, "switch_off": e_off}
    # the forward contract of the image branch itself: preds keys, on_middle once and before the late segment, on_step after every call
    events.clear()
    with torch.no_grad():
        p_on = net(img=pin["img"], img_indices=pin["img_indices"], on_middle=lambda f: events.append("middle"), on_step=lambda: events.append("step"))
        net.set_native_eval(False)
        p_off = net(img=pin["img"], img_indices=pin["img_indices"])
    assert p_on.keys() == p_off.keys()
    if net.middle_feat_block_number is not None:
        assert events.count("middle") == 1
        if has_mid:
            assert events == ["step", "eval", "middle", "step", "eval", "step"], events
    else:
        assert events == ["step", "eval", "step"], events
    for k in on:
        if k.startswith("img_"):
            assert same(p_on[k], on[k]), k
    record = os.environ.get("FTX_NATIVE_IMAGE_PARITY_OUT")      # set by whoever refreshes profiles/native_image_parity.json
    if len(PARITY) == len(KINDS) and record:
        with open(record, "w") as f:
            json.dump({"what": "worst |logit - CPU oracle| over the outputs of each small model, eval mode, vit_linear_impl=ftx_split; "
                               "image_native_eval on and off", "tolerance": TOL, "models": PARITY}, f, indent=1, sort_keys=True)
            f.write("\n")


@pytest.mark.parametrize("how", ["library", "training"])
def test_switch_leaves_other_configurations_alone(how, oracle_runs):
    kw = dict(vit_linear_impl="library") if how == "library" else {}
    model, _, batch = _product("middle", oracle_runs, **kw)
    net = model.image_backbone
    pin = product_inputs(batch)

    def run(on):
        net.set_native_eval(on)
        state = {k: v.clone() for k, v in model.state_dict().items()}
        torch.manual_seed(11)
        torch.cuda.manual_seed(11)
        if how == "training":
            model.train()
            out = model(pin)
        else:
            with torch.no_grad():
                out = model(pin)
        torch.cuda.synchronize()
        model.load_state_dict(state)
        return {k: v.detach().clone() for k, v in out.items()}
    off, on = run(False), run(True)
    assert net._native is None, "the executor must not be built, let alone run"
    assert ("library" if how == "library" else "training mode") in net.native_eval_reason()
    assert on.keys() == off.keys()
    for k in off:
        assert same(on[k], off[k]), (how, k)


# ---------------------------------------------------------------- the INTEGRATION sketch
def test_integration_sketch_through_ctypes(env, oracle_runs):
    """INTEGRATION section 3, "the image branch from C", call for call through ctypes: ftx_sample_down_fwd -> ftx_vit_eval ->
    ftx_lift_gather_fwd -> ftx_rows_gemm, against the package with the switch on."""
    spf, _ = env
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd import native_image as ni
    from fusiontransformer_amd.models.image_models_billinear import pack_img_indices
    model, _, batch = _product("middle", oracle_runs)
    net = model.image_backbone.set_native_eval(True)
    pin = product_inputs(batch)
    with torch.no_grad():
        want = net(img=pin["img"], img_indices=pin["img_indices"])
    assert net.native_eval_reason() is None
    lib = ctypes.CDLL(_lib.LIB_PATH)
    vp, i32, i64, f32, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    lib.ftx_sample_down_workspace_bytes.restype = sz
    lib.ftx_vit_eval_arena_bytes.restype = sz
    lib.ftx_vit_eval_arena_bytes.argtypes = [vp, i32, i32]
    lib.ftx_sample_down_fwd.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, f32, f32, i32, vp, vp, vp, sz, vp]
    lib.ftx_vit_eval.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, i32, i32, i32, i32, vp, vp, sz, vp]
    lib.ftx_lift_gather_fwd.argtypes = [vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp, vp]
    lib.ftx_rows_gemm.argtypes = [vp, i64, vp, i32, vp, i32, i32, vp, vp]
    dev = dict(device="cuda", dtype=torch.float32)
    st = spf.stream()
    img = pin["img"].contiguous()
    b, _, h, w = img.shape
    idx, frame = pack_img_indices(pin["img_indices"], img.device)
    n = idx.shape[0]
    model_rec, blocks, taps, _ = ni.emit(net)       # once per model: the three tables
    conv, bn = net.sample_down.stem[0], net.sample_down.stem[2]
    x = torch.empty((b, 3, SIDE, SIDE), **dev)
    saved = torch.empty(33, device="cuda", dtype=torch.float64)
    ws_bytes = lib.ftx_sample_down_workspace_bytes()
    ws = torch.empty(ws_bytes, device="cuda", dtype=torch.uint8)
    assert lib.ftx_sample_down_fwd(img.data_ptr(), b, h, w, SIDE, SIDE, conv.weight.data_ptr(), conv.bias.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(),
                                   bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.momentum, bn.eps, 0, x.data_ptr(), saved.data_ptr(),
                                   ws.data_ptr(), ws_bytes, st) == 0
    need = lib.ftx_vit_eval_arena_bytes(ni._ptr(model_rec), len(blocks), b)
    arena = torch.empty(need, device="cuda", dtype=torch.uint8)
    grids = [torch.empty((b, GRID, GRID, CO), **dev) for _ in taps]
    tap_out = (vp * len(taps))(*[g.data_ptr() for g in grids])
    mid, late = int(taps[0]["block"]), int(taps[1]["block"])
    feats = [torch.empty((n, CO), **dev) for _ in taps]
    assert lib.ftx_vit_eval(ni._ptr(model_rec), ni._ptr(blocks), len(blocks), ni._ptr(taps), 1, b, x.data_ptr(), None, 0, mid, 0, 0, tap_out, arena.data_ptr(),
                            need, st) == 0
    assert lib.ftx_lift_gather_fwd(grids[0].data_ptr(), idx.data_ptr(), frame.data_ptr(), n, b, GRID, GRID, CO, 370, 1226, feats[0].data_ptr(), st) == 0
    # ... the middle features go to the LiDAR stream here (ftx_spvcnn_eval segment 2 takes them through the fusion transform) ...
    assert lib.ftx_vit_eval(ni._ptr(model_rec), ni._ptr(blocks), len(blocks), ni._ptr(taps), 2, b, None, None, mid + 1, late, 0, 0, tap_out,
                            arena.data_ptr(), need, st) == 0
    assert lib.ftx_lift_gather_fwd(grids[1].data_ptr(), idx.data_ptr(), frame.data_ptr(), n, b, GRID, GRID, CO, 370, 1226, feats[1].data_ptr(), st) == 0
    logits = []
    for head in (net.linear, net.linear2):
        out = torch.empty((n, head.out_features), **dev)
        assert lib.ftx_rows_gemm(feats[1].data_ptr(), n, head.weight.data_ptr(), 1, head.bias.data_ptr(), CO, head.out_features, out.data_ptr(), st) == 0
        logits.append(out)
    torch.cuda.synchronize()
    assert same(feats[0], want["img_middle_feats"]) and same(feats[1], want["img_feats"])
    assert same(logits[0], want["img_seg_logit"]) and same(logits[1], want["img_seg_logit2"])
