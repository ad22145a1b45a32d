"""The contract of every torch.autograd.Function node of fusiontransformer_amd/functional.py, over the table of tests/autograd_cases.py.

The value tests always call with good, contiguous operands that all require a gradient.  These hold the layer between torch and the
kernels to what it promises besides values.  Every comparison is of bits (tests/guard.py same_bits); a tolerance appears twice:
the float-atomic forms are held to the scatter bound of tests/pointvoxel_ref.py ((L + 8) 2^-24 R against float64, the bar of
test_sorted_and_atomic_forms_on_skewed_segments), and the eval-mode BatchNorm parameter gradients to the yardstick rule of
tests/test_stn_gpu.py (BAR_FACTOR x the error of torch's own float32 evaluation on the CPU, against float64).

  A  gradient subsets: whichever inputs ask, each gradient asked for is there and has the bits of the all-on run, and so has the output;
  B  layouts: an input or an incoming gradient in permuted, NaN-interleaved, 16-byte-offset or stride-0 storage gives the same bits
     or a ValueError -- never other numbers, never NaN;
  C  lifetime: a backward after the stream's scratch buffer was reused, overwritten and re-grown; a second backward; an input or a
     saved output changed in place (autograd's version counter must object: what the backward reads went through
     save_for_backward); the forward outside grad mode;
  D  every differentiable input that asks gets a gradient, every other float input that asks is refused by name;
  E  a bad operand raises ValueError before anything is launched: the calls run against tests/nolaunch.py, under which a launch is
     an AssertionError, so a missing check fails at the stub and nothing short ever reaches a kernel.

With FTX_TEST_REPORT_DIR set, the BatchNorm figures are written to <dir>/autograd_contract.txt."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests.autograd_cases import CASES, VARIATIONS
from tests.guard import same_bits
from tests.nolaunch import NoLaunch

pytestmark = pytest.mark.gpu
BAR_FACTOR = 4                      # as tests/test_stn_gpu.py
# autograd's objections to an in-place change of something a node saved: the version counter of a saved tensor, and its two guards
# for a saved view of an input (layer_norm, vit_linear, vit_mlp keep x reshaped) or of an output (add_layer_norm returns two views)
INPLACE = "modified by an inplace operation|has been modified inplace"
REPORT = []

by_case = pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
saving = [c for c in CASES if c.saves_output]
by_saving_case = pytest.mark.parametrize("case", saving, ids=[c.id for c in saving])


@pytest.fixture(scope="module")
def spf():
    from fusiontransformer_amd import functional
    yield functional
    d = os.environ.get("FTX_TEST_REPORT_DIR")
    if d and REPORT:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "autograd_contract.txt"), "w") as f:
            f.write("case | quantity | kernel error | yardstick error (torch float32 on the CPU) | bar = %d x yardstick\n" % BAR_FACTOR)
            f.write("\n".join(REPORT) + "\n")


# ---------------------------------------------------------------------------------------------------------------- running a case
def grad_outs(outs, seed=7):
    return tuple(torch.randn(t.shape, generator=torch.Generator().manual_seed(seed + i), dtype=torch.float32).cuda() for i, t in enumerate(outs))


def forward(spf, case, o, need=None):
    """The entry on fresh leaves over o's storage: (operands as passed, outputs, names of the inputs that asked)."""
    names = case.names("diff", o)
    need = names if need is None else need
    lv = dict(o)
    for k in names:
        lv[k] = o[k].detach().requires_grad_(k in need)
    return lv, case.call(spf, lv), [k for k in names if k in need]


def backward(lv, outs, asked, gos=None, retain=False):
    gos = grad_outs(outs) if gos is None else gos
    return dict(zip(asked, torch.autograd.grad(outs, [lv[k] for k in asked], gos, retain_graph=retain, allow_unused=True)))


def run(spf, case, o, need=None, gos=None):
    lv, outs, asked = forward(spf, case, o, need)
    return [t.detach() for t in outs], backward(lv, outs, asked, gos)


def assert_same(case, got, ref, what):
    """Outputs and the gradients asked for: present, finite, and (but for a float-atomic quantity) the reference's bits."""
    (outs, grads), (routs, rgrads) = got, ref
    assert len(outs) == len(routs)
    for i, (a, b) in enumerate(zip(outs, routs)):
        assert torch.isfinite(a).all(), "%s %s: output %d is not finite" % (case.id, what, i)
        assert "out" in case.nondet or same_bits(a, b), "%s %s: output %d differs" % (case.id, what, i)
    for k, g in grads.items():
        assert g is not None, "%s %s: no gradient for %s" % (case.id, what, k)
        assert torch.isfinite(g).all(), "%s %s: the gradient of %s is not finite" % (case.id, what, k)
        assert "grad" in case.nondet or same_bits(g, rgrads[k]), "%s %s: the gradient of %s differs" % (case.id, what, k)


def reference(spf, case, o):
    ref = run(spf, case, o)
    assert_same(case, ref, ref, "all on")
    return ref


# ---------------------------------------------------------------------------------------------------------------- A
def at_the_scatter_bar(spf, case, o):
    """A form with a sorted and a float-atomic twin, against float64 at the bound both are held to."""
    from tests import pointvoxel_ref as PV
    outs, grads = run(spf, case, o)
    for quantity, (ref, R, L) in case.truth(o, grad_outs(outs)[0]).items():
        got = (outs[0] if quantity == "out" else grads[case.names("diff", o)[0]]).cpu().numpy().reshape(ref.shape)
        assert np.isfinite(got).all()
        r = PV.ratio(got, ref, PV.bound(R, L))
        print("%s %s: error / bound = %.3g" % (case.id, quantity, r))
        assert r <= 1.0, "%s %s: error is %.3g x the bound" % (case.id, quantity, r)


@by_case
def test_gradient_subsets(spf, case):
    o = case.build()
    if case.check is not None:
        case.check(o)
    names = case.names("diff", o)
    ref = reference(spf, case, o)
    assert set(ref[1]) == set(names)
    for r in range(1, len(names)):
        for subset in itertools.combinations(names, r):
            assert_same(case, run(spf, case, o, subset), ref, "with only %s asking" % (subset,))
    if case.truth is not None:
        at_the_scatter_bar(spf, case, o)
    if case.entry == "add_layer_norm" and case.id.endswith("-s]"):
        # only the sum is used: its gradient passes through to both addends as it is, and the LayerNorm's parameters get exact zeros
        go, g = grad_outs(ref[0])[0], ref[1]
        assert torch.equal(g["x"], go) and torch.equal(g["y"], go)
        assert not g["weight"].any() and not g["bias"].any()


# ---------------------------------------------------------------------------------------------------------------- B
LAYOUTS = ("permuted", "nan_rows", "offset16")


def relayout(t, how):
    """t's values in other storage (None where that is no other storage): `permuted` dimensions reversed in memory; `nan_rows` every
    other row of a buffer twice as long whose skipped rows hold NaN; `offset16` contiguous, 4 floats into a NaN-filled buffer (16-byte
    aligned and no more: the dense entries' header contract forbids less); `expanded` stride 0 (needs a constant t)."""
    nan = float("nan")
    if t.dim() == 0 or t.numel() < 2:
        return None
    if how == "permuted":
        perm = list(reversed(range(t.dim())))
        v = t.permute(perm).contiguous().permute(perm)
    elif how == "nan_rows":
        ax = next(i for i, s in enumerate(t.shape) if s > 1)
        shape = list(t.shape)
        shape[ax] *= 2
        sl = tuple(slice(None, None, 2) if i == ax else slice(None) for i in range(t.dim()))
        v = torch.full(shape, nan, dtype=t.dtype, device=t.device)[sl]
        v.copy_(t)
    elif how == "offset16":
        v = torch.full((t.numel() + 8,), nan, dtype=t.dtype, device=t.device)[4:4 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 32 == 16
        return v
    elif how == "expanded":
        v = t.flatten()[0].expand(t.shape)
    assert torch.equal(v, t)
    return None if v.is_contiguous() else v


@by_case
def test_input_layouts(spf, case):
    o = case.build()
    ref = reference(spf, case, o)
    tried = 0
    for name in case.ops:
        t = o.get(name)
        if t is None or not t.is_floating_point():
            continue
        for how in LAYOUTS:
            v = relayout(t, how)
            if v is None:
                continue
            tried += 1
            try:
                got = run(spf, case, dict(o, **{name: v}))
            except ValueError:
                continue
            assert_same(case, got, ref, "with %s %s" % (name, how))
    assert tried


GRAD_LAYOUTS = ("expanded", "permuted", "nan_rows")


@by_case
def test_gradient_layouts(spf, case):
    o = case.build()
    shapes = [t.shape for t in run(spf, case, o)[0]]
    for how in GRAD_LAYOUTS:
        if how == "expanded":      # what out.sum().backward() feeds
            dense = tuple(torch.full(s, 0.37 + i, dtype=torch.float32, device="cuda") for i, s in enumerate(shapes))
        else:
            dense = grad_outs([torch.empty(s) for s in shapes])
        views = [relayout(g, how) for g in dense]
        if all(v is None for v in views):
            continue
        ref = run(spf, case, o, gos=dense)
        try:
            got = run(spf, case, o, gos=tuple(g if v is None else v for g, v in zip(dense, views)))
        except ValueError:
            continue
        assert_same(case, got, ref, "with a %s gradient" % how)


# ---------------------------------------------------------------------------------------------------------------- C
@by_case
def test_backward_after_the_scratch_buffer_was_reused(spf, case, monkeypatch):
    """forward, a larger forward of the same node on other values, then the first backward: nothing a backward needs may live in the
    stream's scratch buffer.  The buffer is this test's own; after the second forward it is overwritten with 0xFF (NaN as float32 and
    float64) and replaced by a larger one, which is what a later, larger call does to it."""
    monkeypatch.setattr(spf, "_SCRATCH", {})
    o, big = case.build(), case.build(2)
    ref = reference(spf, case, o)
    lv, outs, asked = forward(spf, case, o)
    forward(spf, case, big)
    for key, buf in list(spf._SCRATCH.items()):
        buf.fill_(0xFF)
        spf._SCRATCH[key] = torch.full((2 * buf.numel(),), 0xFF, dtype=torch.uint8, device=buf.device)
    assert_same(case, ([t.detach() for t in outs], backward(lv, outs, asked)), ref, "after a second forward")


@by_case
def test_backward_twice(spf, case):
    o = case.build()
    lv, outs, asked = forward(spf, case, o)
    gos = grad_outs(outs)
    first = backward(lv, outs, asked, gos, retain=True)
    assert_same(case, ([], first), ([], first), "first backward")
    torch.autograd.backward(outs, gos, retain_graph=True)
    second = {k: lv[k].grad.clone() for k in asked}
    assert_same(case, ([], second), ([], first), "second backward")
    torch.autograd.backward(outs, gos)
    if "grad" not in case.nondet:
        for k in asked:
            assert same_bits(lv[k].grad, second[k] + second[k]), "%s: .grad of %s is not twice the gradient" % (case.id, k)


@by_case
def test_input_changed_in_place_before_backward(spf, case):
    o = case.build()
    ref = reference(spf, case, o)
    for name in case.names("diff", o):
        mine = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in o.items()}
        lv, outs, asked = forward(spf, case, mine)
        with torch.no_grad():
            lv[name].add_(1.0)
        if case.ops[name].reads:
            with pytest.raises(RuntimeError, match=INPLACE):
                backward(lv, outs, asked)
            continue
        try:        # not read by the backward: saved all the same (autograd objects), or the gradients do not move
            grads = backward(lv, outs, asked)
        except RuntimeError as e:
            assert re.search(INPLACE, str(e)), e
            continue
        assert_same(case, ([], grads), ([], ref[1]), "with %s changed after the forward" % name)


@by_saving_case
def test_saved_output_changed_in_place_before_backward(spf, case):
    lv, outs, asked = forward(spf, case, case.build())
    with torch.no_grad():
        outs[0].add_(1.0)
    with pytest.raises(RuntimeError, match=INPLACE):
        backward(lv, outs, asked)


@by_case
def test_forward_outside_grad_mode(spf, case):
    o = case.build()
    ref = reference(spf, case, o)
    lv = dict(o)
    for k in case.names("diff", o) + case.names("refused", o):
        lv[k] = o[k].detach().requires_grad_(True)
    with torch.no_grad():
        outs = case.call(spf, lv)
    assert not any(t.requires_grad for t in outs)
    assert_same(case, (list(outs), {}), ref, "under no_grad")


# ---------------------------------------------------------------------------------------------------------------- D
@by_case
def test_every_input_that_asks_is_answered(spf, case):
    o = case.build()
    for name in case.names("diff", o):
        _, grads = run(spf, case, o, [name])
        g = grads[name]
        assert g is not None, "%s: %s requires grad and gets None" % (case.id, name)
        assert g.shape == o[name].shape and g.dtype == torch.float32 and torch.isfinite(g).all()
    for name in case.names("refused", o):
        lv = dict(o, **{name: o[name].detach().requires_grad_(True)})
        with pytest.raises((RuntimeError, ValueError), match=name):
            case.call(spf, lv)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("residual", [False, True])
def test_batch_norm_eval_parameter_gradients(spf, residual, relu):
    """d gamma and d beta of the eval-mode BatchNorm against float64 F.batch_norm(training=False) autograd on the CPU; the yardstick is
    the same expression in float32 on the CPU.  The ReLU is a kink: the inputs keep every pre-activation 1e-5 clear of 0 in float64
    (asserted), two orders above a float32 rounding of these values, so all three evaluations take the same mask."""
    import torch.nn.functional as F
    case = next(c for c in CASES if c.id == "batch_norm[eval-res%d-relu%d]" % (residual, relu))
    o = case.build()
    outs, grads = run(spf, case, o)
    go = grad_outs(outs)[0].cpu()
    res = {}
    for dt in (torch.float64, torch.float32):
        p = {k: o[k].detach().cpu().to(dt) for k in ("x", "residual", "gamma", "beta", "running_mean", "running_var") if o[k] is not None}
        p["gamma"].requires_grad_(True)
        p["beta"].requires_grad_(True)
        y = F.batch_norm(p["x"], p["running_mean"], p["running_var"], p["gamma"], p["beta"], False, 0.0, 1e-5)
        if residual:
            y = y + p["residual"]
        if relu:
            if dt == torch.float64:
                assert y.abs().min().item() > 1e-5, "a pre-activation sits on the ReLU's kink"
            y = F.relu(y)
        y.backward(go.to(dt))
        res[dt] = (p["gamma"].grad, p["beta"].grad)
    for i, q in enumerate(("gamma", "beta")):
        truth, yard = res[torch.float64][i], res[torch.float32][i]
        ek, ey = (grads[q].cpu().double() - truth).abs().max().item(), (yard.double() - truth).abs().max().item()
        line = "%s | grad_%s | %.3e | %.3e | %.3e" % (case.id, q, ek, ey, BAR_FACTOR * ey)
        REPORT.append(line)
        print(line)
        assert ek <= BAR_FACTOR * ey, line


# ---------------------------------------------------------------------------------------------------------------- E
def vary(t, how, axis):
    """A bad twin of a good operand (None where the shape leaves no room for it)."""
    if how == "float64":
        return t.double()
    if how == "cpu":
        return t.cpu()
    if how in ("short", "long"):
        shape = list(t.shape)
        shape[axis] += -4 if how == "short" else 1
        return torch.zeros(shape, dtype=t.dtype, device=t.device) if shape[axis] >= 1 else None
    if how == "extra_dim":
        return t.unsqueeze(0)
    if how == "strided":
        if t.dim() == 0 or t.numel() < 2:
            return None
        ax = next(i for i, s in enumerate(t.shape) if s > 1)
        shape = list(t.shape)
        shape[ax] *= 2
        v = torch.zeros(shape, dtype=t.dtype, device=t.device)[tuple(slice(None, None, 2) if i == ax else slice(None) for i in range(t.dim()))]
        assert v.shape == t.shape and not v.is_contiguous()
        return v
    raise KeyError(how)


@by_case
def test_bad_operands_never_launch(spf, case, monkeypatch):
    from fusiontransformer_amd import _lib
    o = case.build()                     # maps and segments come from the real library, before the stub goes in
    lv = forward_operands(case, o)
    monkeypatch.setattr(_lib, "load", lambda: NoLaunch())
    # good operands (an absent optional one included) do reach the stubbed launch: the stub stands where the kernels are
    with pytest.raises(AssertionError, match="launched"):
        case.call(spf, lv)
    if not case.fullest:
        return
    wrong = []
    for name, op in case.ops.items():
        for how in VARIATIONS:
            v = vary(o[name], how, op.axis) if how in op.bad else None
            if v is None:
                continue
            if op.role == "diff" and v.is_floating_point():
                v.requires_grad_(True)
            try:
                case.call(spf, dict(lv, **{name: v}))
            except ValueError:
                continue
            except AssertionError as e:
                wrong.append("%s %s: not refused, it reached the launch (%s)" % (name, how, e))
            except Exception as e:
                wrong.append("%s %s: %s instead of ValueError: %s" % (name, how, type(e).__name__, e))
            else:
                wrong.append("%s %s: no error" % (name, how))
    assert not wrong, "%s:\n  " % case.id + "\n  ".join(wrong)


def forward_operands(case, o):
    """Good operands as a training step passes them: every differentiable input requires grad."""
    lv = dict(o)
    for k in case.names("diff", o):
        lv[k] = o[k].detach().requires_grad_(True)
    return lv
