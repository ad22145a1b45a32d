"""Float64 restatement of one fused layer of the spatial transformers' localisation net,
    relu(max_pool2d(conv2d(x, w, bias), 2, 2)),
its routing map, the float32 yardstick the GPU tests take their bars from, and the inputs of tests/test_stn_loc_*.py.

Routing.  sel (b, co, ph, pw) int8 holds the position 0..3 (row-major in the 2 x 2 window, the first on a tie -- torch's own choice,
read off max_pool2d's indices) of the window's maximum, -1 where that maximum is <= 0 (dead ReLU, zero gradient).  `routed` restates
the layer as "take the conv value at the routed position": with a layer's own sel it is the layer exactly, and with a GIVEN sel it is
linear in x, w and bias -- which is how the backward kernels are judged: every implementation (float64 truth, float32 yardstick,
kernel) gets the truth's routing, so the comparison is about arithmetic and nothing is left out of it.

Ambiguity.  The forward's sel can only differ from the truth's where two values each within the forward bar of their truth could swap
order or sign: the float64 top-two gap is < 2 x bar, or |maximum| < 1 x bar."""
import functools

import torch
import torch.nn.functional as F

BAR_FACTOR = 4          # as tests/test_stn_gpu.py
AMBIGUOUS_CAP = 0.005   # share of windows that may be ambiguous, asserted on the CPU before a kernel is judged

# (b, c, ih, iw, k, co), layout
SMALL = [((1, 1, 8, 8, 7, 8), "nchw"), ((2, 3, 9, 12, 7, 8), "nchw"), ((2, 96, 23, 37, 7, 8), "nchw"), ((2, 96, 23, 37, 7, 8), "nhwc"),
         ((2, 8, 21, 30, 5, 90), "nchw"), ((1, 3, 48, 80, 7, 8), "nchw"), ((3, 8, 40, 70, 5, 90), "nchw")]
FULL = [(1, 96, 384, 384, 7, 8), (1, 8, 189, 189, 5, 90), (1, 3, 370, 1226, 7, 8)]


def pooled_size(ih, iw, k):
    return (ih - k + 1) // 2, (iw - k + 1) // 2


def layer(x, w, bias):
    """(relu(pool(conv)), sel int8) in x's dtype."""
    conv = F.conv2d(x, w.to(x.dtype), None if bias is None else bias.to(x.dtype))
    pooled, idx = F.max_pool2d(conv, 2, stride=2, return_indices=True)
    ow = conv.shape[-1]
    ph, pw = pooled.shape[-2:]
    dy = idx // ow - 2 * torch.arange(ph).view(1, 1, ph, 1)
    dx = idx % ow - 2 * torch.arange(pw).view(1, 1, 1, pw)
    sel = torch.where(pooled > 0, dy * 2 + dx, torch.full_like(idx, -1)).to(torch.int8)
    return F.relu(pooled), sel


def windows(conv):
    """(b, co, ph, pw, 4): the 2 x 2 windows the pool sees, row-major; the odd trailing row / column is dropped."""
    b, co, oh, ow = conv.shape
    ph, pw = oh // 2, ow // 2
    return conv[:, :, :2 * ph, :2 * pw].reshape(b, co, ph, 2, pw, 2).permute(0, 1, 2, 4, 3, 5).reshape(b, co, ph, pw, 4)


def routed(x, w, bias, sel):
    """The layer with the routing given: the conv value at position sel of every window, 0 where sel is -1.  Differentiable."""
    win = windows(F.conv2d(x, w.to(x.dtype), None if bias is None else bias.to(x.dtype)))
    return win.gather(-1, sel.clamp(min=0).long().unsqueeze(-1)).squeeze(-1) * (sel >= 0).to(x.dtype)


def ambiguous(x64, w64, bias64, bar):
    """Mask (b, co, ph, pw) of the windows whose routing a result within `bar` of the float64 truth may legitimately change."""
    top = windows(F.conv2d(x64, w64, bias64)).sort(-1, descending=True).values
    return ((top[..., 0] - top[..., 1]) < 2 * bar) | (top[..., 0].abs() < bar)


def rel_l2(got, want):
    """Relative L2 error of a whole tensor; 0 where both are exactly equal."""
    d, n = (got.double() - want.double()).norm().item(), want.double().norm().item()
    return 0.0 if d == 0.0 else (d / n if n > 0 else float("inf"))


def inputs(shape, seed=3):
    """Seeded randn x and torch-default-scaled Conv2d parameters (uniform in +- 1 / sqrt(fan in)) of a (b, c, ih, iw, k, co) case."""
    b, c, ih, iw, k, co = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, c, ih, iw), generator=g)
    bound = 1.0 / (c * k * k) ** 0.5
    w = (torch.rand((co, c, k, k), generator=g) * 2 - 1) * bound
    bias = (torch.rand((co,), generator=g) * 2 - 1) * bound
    return x, w, bias


@functools.lru_cache(maxsize=None)
def case(shape):
    """Everything the forward comparison of one case needs, computed once on the CPU and never modified: inputs, the float64 truth
    (pooled output, its mean, sel), the float32 yardstick's outputs, the two forward bars and the ambiguous mask with its share."""
    x, w, bias = inputs(shape)
    truth, sel = layer(x.double(), w.double(), bias.double())
    yard, yard_sel = layer(x, w, bias)
    bar = BAR_FACTOR * (yard.double() - truth).abs().max().item()
    tmean, ymean = truth.mean((2, 3)), yard.mean((2, 3))
    amb = ambiguous(x.double(), w.double(), bias.double(), bar)
    return dict(x=x, w=w, bias=bias, truth=truth, sel=sel, yard=yard, yard_sel=yard_sel, bar=bar, truth_mean=tmean, yard_mean=ymean,
                ambiguous=amb, ambiguous_share=amb.double().mean().item())


def backward_truth(shape, g, mean):
    """Gradients (dX, dW, db) of sum(g * routed(...)) -- or of sum(g * its spatial mean) -- under the TRUTH's routing, as float64 autograd
    (the truth) and as float32 autograd on the CPU with the same routing (the yardstick)."""
    cs = case(shape)
    res = []
    for dt in (torch.float64, torch.float32):
        x, w, bias = (t.to(dt).clone().requires_grad_(True) for t in (cs["x"], cs["w"], cs["bias"]))
        y = routed(x, w, bias, cs["sel"])
        if mean:
            y = y.mean((2, 3))
        (y * g.to(dt)).sum().backward()
        res.append((x.grad, w.grad, bias.grad))
    return res[0], res[1]


def theta_of(params, prefix, x):
    """stn_ref.theta_of's chain restated with `layer`: the host tests assert the two agree exactly."""
    p = lambda k: params[prefix + k].to(x.dtype)
    xs, _ = layer(x, p("localization.0.weight"), p("localization.0.bias"))
    xs, _ = layer(xs, p("localization.3.weight"), p("localization.3.bias"))
    xs = xs.mean((2, 3))
    xs = F.relu(F.linear(xs, p("fc_loc.0.weight"), p("fc_loc.0.bias")))
    return F.linear(xs, p("fc_loc.2.weight"), p("fc_loc.2.bias")).view(-1, 2, 3)
