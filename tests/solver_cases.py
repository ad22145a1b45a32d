"""Inputs and drivers shared by tests/test_solver_host.py and tests/test_solver_gpu.py: the awkward tensor set, the optimizer
configurations under test, a driver that steps any torch-style optimizer over them and records parameters and state after every
step, and the error of such a run against tests/optim_ref.py in units of 2^-24 times each tensor's largest magnitude."""
import numpy as np
import torch

from tests import optim_ref as R

# one element, a 16 K chunk boundary, one past it, lengths that are no multiple of 4, several chunks; tensor 4 gets no gradient in
# steps 1-2.  Tensor 7 and its gradient start one element into their storage (4-byte alignment: the scalar path); tensor 8's
# gradient is not contiguous.
SHAPES = [(1,), (16384,), (16385,), (333, 7), (3, 64, 96), (70001,), (5,), (4099,), (40, 50)]
SKIPS, SKIP_STEPS, OFFSET, STRIDED = 4, (1, 2), 7, 8
STEPS = 6
LR, WD = 3e-3, 5e-4

# name -> (rule, keyword arguments, clipped)
CONFIGS = {
    "sgd momentum": ("SGD", dict(momentum=0.9), False),
    "sgd nesterov": ("SGD", dict(momentum=0.9, nesterov=True), False),
    "sgd dampening": ("SGD", dict(momentum=0.9, dampening=0.1), False),
    "sgd plain": ("SGD", dict(momentum=0.0), False),
    "adamw": ("AdamW", dict(), False),
    "adam clipped": ("Adam", dict(), True),
    "sgd momentum clipped": ("SGD", dict(momentum=0.9), True),
    "adamw clipped": ("AdamW", dict(), True),
}
STATE_KEYS = {"SGD": ("momentum_buffer",), "Adam": ("exp_avg", "exp_avg_sq"), "AdamW": ("exp_avg", "exp_avg_sq")}


def inputs(seed=21, shapes=SHAPES, steps=STEPS):
    rng = np.random.default_rng(seed)
    base = [rng.standard_normal(sh).astype(np.float32) for sh in shapes]
    grads = []
    for step in range(steps):
        grads.append([None if (i == SKIPS and step in SKIP_STEPS) else rng.standard_normal(sh).astype(np.float32) for i, sh in enumerate(shapes)])
    return base, grads


def max_norm_for(grads, coef=0.3):
    """A max_norm under which the first step's coefficient is about `coef` (an input of the test, fixed by the seed)."""
    return float(np.float32(coef * R.grad_norm(grads[0])))


def place(a, device, dtype, offset=False, strided=False):
    """A tensor holding `a`: plain, or starting one element into its storage, or (2-D) stored transposed."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype, copy=True)      # never the caller's memory
    if offset:
        whole = torch.empty(t.numel() + 1, device=device, dtype=dtype)
        whole[1:].copy_(t.reshape(-1))
        t = whole[1:].view(t.shape)
    if strided:
        t = t.t().contiguous().t()
    return t


def make_params(base, device, dtype=torch.float32, awkward=True):
    return [torch.nn.Parameter(place(b, device, dtype, offset=awkward and i == OFFSET)) for i, b in enumerate(base)]


def set_grads(params, grads, device, dtype=torch.float32, awkward=True):
    for i, (p, g) in enumerate(zip(params, grads)):
        p.grad = None if g is None else place(g, device, dtype, offset=awkward and i == OFFSET, strided=awkward and i == STRIDED)


def snapshot(opt, params, keys):
    out = {"param": [p.detach().cpu().numpy().copy() for p in params]}
    for k in keys:
        out[k] = [opt.state[p][k].detach().cpu().numpy().copy() if k in opt.state[p] else None for p in params]
    return out


def drive(opt, params, grads, keys, device, dtype=torch.float32, clip=None, awkward=True, scheduler=None):
    """Steps `opt` over grads; clip: a max_norm applied with clip_grad_norm_ before every step (the torch sequence).  Returns the
    snapshot after every step."""
    shots = []
    for g in grads:
        set_grads(params, g, device, dtype, awkward)
        if clip is not None:
            torch.nn.utils.clip_grad_norm_([p for p in params if p.grad is not None], clip, foreach=False)
        opt.step()
        if scheduler is not None:
            scheduler.step()
        shots.append(snapshot(opt, params, keys))
    return shots


def reference(rule, kwargs, base, grads, max_norm=None, lrs=None):
    ref = getattr(R, rule)(base, LR, weight_decay=WD, max_norm=max_norm, **kwargs)
    shots = []
    for s, g in enumerate(grads):
        ref.step(g, None if lrs is None else lrs[s])
        shot = {"param": [p.copy() for p in ref.p]}
        for k, v in ref.state().items():
            shot[k] = [None if x is None else x.copy() for x in v]
        shots.append(shot)
    return shots


def worst(shots, ref_shots):
    """{quantity: worst error over steps and tensors, in units of 2^-24 max|reference tensor|}.  A state tensor that is absent on
    one side must be absent on the other."""
    out = {}
    for shot, ref in zip(shots, ref_shots):
        assert set(ref) <= set(shot), (sorted(shot), sorted(ref))
        for k in shot:
            for a, b in zip(shot[k], ref.get(k, [None] * len(shot[k]))):
                assert (a is None) == (b is None), k
                if b is not None:
                    out[k] = max(out.get(k, 0.0), R.worst_units(a, b))
    return out


def yardstick(name, base, grads):
    """torch's own float32 optimizer on the CPU (foreach=False), clipped variants preceded by clip_grad_norm_, against the float64
    restatement: the error a correctly rounded float32 chain of this length makes."""
    rule, kwargs, clipped = CONFIGS[name]
    max_norm = max_norm_for(grads) if clipped else None
    params = make_params(base, "cpu", awkward=False)
    opt = getattr(torch.optim, rule)(params, lr=LR, weight_decay=WD, foreach=False, **kwargs)
    shots = drive(opt, params, grads, STATE_KEYS[rule], "cpu", clip=max_norm, awkward=False)
    return worst(shots, reference(rule, kwargs, base, grads, max_norm))
