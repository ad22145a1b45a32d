"""The solver's step at the benched model's real parameter set (middle fusion: ~330 tensors, 108 M floats): HIP-event time per step of

  * optim.Adam.step()                                   -- one launch, as bench.py runs it
  * optim.Adam(max_grad_norm=1).step()                  -- sum of squares + finalize + the scaled update
  * torch.nn.utils.clip_grad_norm_ + optim.Adam.step()  -- what the fused clip replaces
  * optim.SGD / optim.AdamW against torch.optim's foreach and fused forms

alternated in one process: every round times every variant once, the table gives the median over the rounds and their spread.
usage (GPU box): python tools/bench_optim.py [--iters 20] [--rounds 7] [--out profiles/optim_step.txt]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fusiontransformer_amd import optim  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--kind", default="middle", choices=["middle", "early", "late"])
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_optim.py needs a GPU: nothing here can be timed on the CPU")


def parameter_shapes(kind):
    from fusiontransformer_amd.config import fusion_cfg
    from fusiontransformer_amd.models.build import build_model
    torch.manual_seed(0)
    model = build_model(fusion_cfg(kind))[0]
    return [tuple(p.shape) for p in model.parameters() if p.requires_grad]


shapes = parameter_shapes(args.kind)
gen = torch.Generator(device="cuda").manual_seed(1)
params = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=gen) * 0.02) for s in shapes]
grads = [torch.randn(s, device="cuda", generator=gen) * 1e-3 for s in shapes]
n_el = sum(p.numel() for p in params)
HYPER = dict(lr=1e-6, weight_decay=5e-4)


def with_clip(opt):
    def step():
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
    return step


adam = optim.Adam(params, **HYPER)
VARIANTS = [
    ("optim.Adam", adam.step, 7),
    ("optim.Adam(max_grad_norm=1)", optim.Adam(params, max_grad_norm=1.0, **HYPER).step, 8),
    ("clip_grad_norm_ + optim.Adam", with_clip(adam), None),
    ("optim.SGD momentum 0.9", optim.SGD(params, momentum=0.9, **HYPER).step, 5),
    ("torch SGD foreach", torch.optim.SGD(params, momentum=0.9, foreach=True, **HYPER).step, None),
    ("torch SGD fused", torch.optim.SGD(params, momentum=0.9, fused=True, **HYPER).step, None),
    ("optim.SGD(max_grad_norm=1)", optim.SGD(params, momentum=0.9, max_grad_norm=1.0, **HYPER).step, 6),
    ("optim.AdamW", optim.AdamW(params, **HYPER).step, 7),
    ("torch AdamW foreach", torch.optim.AdamW(params, foreach=True, **HYPER).step, None),
    ("torch AdamW fused", torch.optim.AdamW(params, fused=True, **HYPER).step, None),
    ("optim.AdamW(max_grad_norm=1)", optim.AdamW(params, max_grad_norm=1.0, **HYPER).step, 8),
]


def timed(fn):
    for p, g in zip(params, grads):
        p.grad = g
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters


for _, fn, _ in VARIANTS:          # every variant creates its state and its tables, and loads its code objects, before anything is timed
    timed(fn)
times = {name: [] for name, _, _ in VARIANTS}
for _ in range(args.rounds):
    for name, fn, _ in VARIANTS:
        times[name].append(timed(fn))

lines = ["%s fusion: %d parameter tensors, %.1f M floats; %d rounds of %d steps, variants alternated in one process"
         % (args.kind, len(params), n_el / 1e6, args.rounds, args.iters),
         "HIP-event time per step (host issue included); streams = 4-byte streams per element the own kernels must move",
         "%-32s %10s %10s %10s %8s %10s" % ("variant", "median ms", "min ms", "max ms", "streams", "GB/s")]
for name, _, streams in VARIANTS:
    t = sorted(times[name])
    med = t[len(t) // 2]
    rate = "%10.0f" % (streams * 4.0 * n_el / med / 1e6) if streams else "%10s" % "-"
    lines.append("%-32s %10.3f %10.3f %10.3f %8s %s" % (name, med, t[0], t[-1], streams or "-", rate))
text = "\n".join(lines)
print(text)
if args.out:
    with open(args.out, "w") as f:
        f.write(text + "\n")
