"""Step time of the single-modality baselines (LidarSeg, ImageSegBilinear, ImageSeg) and time of the single-head loss kernel.

usage: python tools/bench_single.py [--steps 60] [--warmup 15] [--out profiles/single_modality_steps.json]
       python tools/bench_single.py --image-stn [--steps 60] [--out profiles/image_stn_steps.json]   # only: ImageSeg beside ImageSegBilinear
       python tools/bench_single.py --native-index-ab [--steps 20]     # LidarSeg steps, native index build off / on, alternating windows
       python tools/bench_single.py --native-train-ab [--steps 20] [--ab-model LidarSeg|middle]   # the same for the training executor
       python tools/bench_single.py --native-train-ab --dropout [--steps 20]   # LidarSeg with the training executor: torch's Dropout and five
                                                                               # segments against the library's Dropout and three; then the kernel
       python tools/bench_single.py --native-image-train-ab [--steps 20]   # the ViT trunk in training: HIP graphs / eager / the native training executor
       python tools/bench_single.py --native-stems-ab [--steps 20]         # the patch embedding and tap stems in training: image_native_stems off / on
       python tools/bench_single.py --native-train-steps on|off --steps N     # N untimed batch-1 steps, to count launches under a kernel trace
       python tools/bench_single.py --lidar-split [--steps 20] [--out profiles/spconv_split_steps.json]   # LidarSeg steps, default against lidar_split

* Steps: TrainStep on synthetic KITTI-shaped frames (data/synth.make_batch), two alternating resident batches as bench.py
  uses, batch 4 and batch 1, HIP events around the timed loop after the warm-up, profiler off.  LidarSeg runs with the index
  prefetch of the next batch (TrainStep(batch, next_batch)).
* Kernel: ftx_seg_loss at n = 81 237, c = 20 with and without gradient, beside the only way the fused two-head kernel can
  produce the same loss (ftx_fusion_loss_mix fed the same tensor as both heads, lambda_xm = 0).  The three are alternated in
  one process over repeated windows; each window is 50 calls captured into one HIP graph (GPU time, back to back) and 50 eager
  calls through the C ABI (includes the host's issue rate).  Median and min..max over the windows are written.

There is no fallback: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_KERNEL, C_KERNEL, CALLS, WINDOWS = 81237, 20, 50, 9


def _inputs(batch, cycle, device):
    from fusiontransformer_amd.data.synth import make_batch
    from fusiontransformer_amd.models.image_models_billinear import pack_img_indices
    from fusiontransformer_amd.sparse import SparseTensor
    b = make_batch([1000 * cycle + i for i in range(batch)])
    return int(b["coords"].shape[0]), {
        "img": torch.from_numpy(b["img"]).to(device),
        "img_indices": pack_img_indices(b["img_indices"], device),
        "lidar": SparseTensor(torch.from_numpy(b["feats"]).to(device), torch.from_numpy(b["coords"]).int().to(device)),
        "seg_label": torch.from_numpy(b["seg_label"]).to(device),
    }


def step_time(kind, batch, steps, warmup, stn_loc=None):
    from fusiontransformer_amd import config
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    cfg = {"LidarSeg": config.lidar_cfg, "ImageSegBilinear": config.image_cfg, "ImageSeg": config.image_stn_cfg}[kind]()
    if stn_loc is not None:
        cfg.MODEL.stn_loc_impl = stn_loc
    torch.manual_seed(0)
    model, metric = build_model(cfg)
    model = model.cuda().train()
    step = TrainStep(cfg, model, metrics=metric)
    assert step.fused_loss and type(step.optimizer).__module__.endswith("optim")
    points, res = zip(*[_inputs(batch, cycle, "cuda") for cycle in (0, 1)])
    seq = [res[i % 2] for i in range(warmup + steps + 1)]     # the index structures are consumed by each forward and rebuilt
    for i in range(warmup):
        step(seq[i], next_batch=seq[i + 1])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(warmup, warmup + steps):
        step(seq[i], next_batch=seq[i + 1])
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    loss = next(iter(step.last.values())).item()
    assert loss == loss, "the loss is NaN"
    r = {"model": kind, "batch": batch, "points_per_batch": list(points), "steps": steps, "warmup": warmup, "ms_per_step": ms,
         "frames_per_s": batch * 1e3 / ms, "last_loss": loss}
    if stn_loc is not None:
        r["stn_loc_impl"] = stn_loc
    return r


def _graph_nodes(t):
    """Number of autograd nodes under tensor t."""
    seen, todo = set(), [t.grad_fn]
    while todo:
        f = todo.pop()
        if f is not None and f not in seen:
            seen.add(f)
            todo += [g for g, _ in f.next_functions]
    return len(seen)


def _named_nodes(t, prefixes):
    """{prefix: how many autograd nodes under tensor t have a name that starts with it}."""
    seen, todo = set(), [t.grad_fn]
    while todo:
        f = todo.pop()
        if f is not None and f not in seen:
            seen.add(f)
            todo += [g for g, _ in f.next_functions]
    return {p: sum(f.name().startswith(p + "Backward") for f in seen) for p in prefixes}


def _switch_ab(switch, batch, steps, warmup, windows=5, model_kind="LidarSeg", both=()):
    """Step time with one switch of the SPVCNN (`set_<switch>`) off and on (the switches of `both` on in either arm): two models from one
    seed in one process, windows of `steps` steps alternating between them; median (min..max) ms per step, and per arm `host_issue_ms` (wall clock of the loop before the
    synchronise, per step: an UPPER bound on the issue time, since it includes the blocking host reads of an index build that the
    prefetch did not finish), the autograd nodes under the LiDAR logits and the peak of torch's allocator above what was resident."""
    import time
    from fusiontransformer_amd import config
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    cfg = config.lidar_cfg() if model_kind == "LidarSeg" else config.fusion_cfg(model_kind)
    _, res = zip(*[_inputs(batch, cycle, "cuda") for cycle in (0, 1)])
    arms, nets = {}, {}
    for mode in ("off", "on"):
        torch.manual_seed(0)
        model = build_model(cfg)[0].cuda().train()
        nets[mode] = model.backbone if model_kind == "LidarSeg" else model.lidar_backbone
        for other in both:
            getattr(nets[mode], "set_" + other)(True)
        getattr(nets[mode], "set_" + switch)(mode == "on")
        arms[mode] = TrainStep(cfg, model)
    info = {m: {} for m in arms}

    def window(mode, n):
        step = arms[mode]
        seq = [res[i % 2] for i in range(n + 1)]
        for x in seq:
            x["lidar"].prepared = None
        torch.cuda.synchronize()
        resident = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(n):
            preds = step(seq[i], next_batch=seq[i + 1])
        e1.record()
        host = (time.perf_counter() - t0) * 1e3 / n
        torch.cuda.synchronize()
        info[mode].setdefault("host_issue_ms", []).append(host)
        info[mode]["autograd_nodes"] = _graph_nodes(preds["lidar_seg_logit"])
        info[mode]["peak_above_resident_bytes"] = int(torch.cuda.max_memory_allocated() - resident)
        return e0.elapsed_time(e1) / n

    for mode in arms:
        window(mode, warmup)
        info[mode]["host_issue_ms"] = []
    ms = {m: [] for m in arms}
    for w in range(windows):
        for mode in (("off", "on") if w % 2 == 0 else ("on", "off")):
            ms[mode].append(window(mode, steps))
    spread = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
    out = {"model": model_kind, "switch": switch, "batch": batch, "steps_per_window": steps, "windows": windows,
           "ms_per_step": {m: spread(v) for m, v in ms.items()}}
    for m in arms:
        out[m] = dict(info[m], host_issue_ms=spread(info[m]["host_issue_ms"]))
    tr = getattr(nets["on"], "_native_tr", None)
    if (switch == "native_train" or "native_train" in both) and tr:
        out["on"]["arena_bytes"] = int(tr.last_arena_bytes)
        out["on"]["segments"] = int(tr.tp.n_segments)
    if both:
        out["on_in_both_arms"] = list(both)
    out["every_on_window_beats_every_off_window"] = bool(max(ms["on"]) < min(ms["off"]))
    out["every_off_window_beats_every_on_window"] = bool(max(ms["off"]) < min(ms["on"]))
    return out


def native_index_ab(batch, steps, warmup, windows=5):
    """LidarSeg step time with the native index build (SPVCNN.set_native_index) off and on: two models from one seed in one process,
    windows of `steps` steps alternating between them; median (min..max) ms per step."""
    from fusiontransformer_amd import config
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    cfg = config.lidar_cfg()
    _, res = zip(*[_inputs(batch, cycle, "cuda") for cycle in (0, 1)])
    arms = {}
    for mode in ("off", "on"):
        torch.manual_seed(0)
        model = build_model(cfg)[0].cuda().train()
        model.backbone.set_native_index(mode == "on")
        arms[mode] = TrainStep(cfg, model)

    def window(step, n):
        seq = [res[i % 2] for i in range(n + 1)]
        for x in seq:
            x["lidar"].prepared = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(n):
            step(seq[i], next_batch=seq[i + 1])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    for step in arms.values():
        window(step, warmup)
    ms = {m: [] for m in arms}
    for w in range(windows):
        for mode in (("off", "on") if w % 2 == 0 else ("on", "off")):
            ms[mode].append(window(arms[mode], steps))
    return {"model": "LidarSeg", "batch": batch, "steps_per_window": steps, "windows": windows,
            "ms_per_step": {m: {"median": statistics.median(v), "min": min(v), "max": max(v)} for m, v in ms.items()}}


def native_train_ab(batch, steps, warmup, windows=5, model_kind="LidarSeg"):
    """Step time with the native training executor (SPVCNN.set_native_train) off and on."""
    return _switch_ab("native_train", batch, steps, warmup, windows, model_kind)


def native_dropout_ab(batch, steps, warmup, windows=5):
    """LidarSeg step time with the training executor on in both arms: torch's Dropout between five segments (off) against the library's
    Dropout as an op of three segments (SPVCNN.set_native_dropout, on).  A claim of faster or slower holds only where the windows do
    not overlap (the two `every_..._window_beats_...` flags); otherwise no difference is shown."""
    return _switch_ab("native_dropout", batch, steps, warmup, windows, "LidarSeg", both=("native_train",))


def dropout_kernel_times(calls=CALLS, windows=WINDOWS):
    """HIP-event time of ftx_dropout (functional.dropout outside autograd, out of place) beside torch.nn.functional.dropout on the same
    tensors: the two Dropout sites of a KITTI-shaped batch of 4 (rows of the stride-16 level x 256 and of the stride-4 level x 128
    channels), p = 0.3, windows of `calls` eager calls alternating between the two; us per call, median (min..max)."""
    import numpy as np
    import torch.nn.functional as F
    from fusiontransformer_amd import functional as spf
    from fusiontransformer_amd.data.synth import make_batch
    coords = make_batch([1000 * 0 + i for i in range(4)])["coords"]
    rows = lambda stride: len(np.unique(np.concatenate([coords[:, :3] // stride, coords[:, 3:]], 1), axis=0))
    out = {"what": "dropout kernel", "p": 0.3, "calls_per_window": calls, "windows": windows, "unit": "us per call", "sites": []}
    for site, (stride, ch) in enumerate(((16, 256), (4, 128))):
        x = torch.randn(rows(stride), ch, device="cuda")
        variants = {"ftx_dropout": lambda c: spf.dropout(x, 0.3, 1, c), "torch_dropout": lambda c: F.dropout(x, 0.3, True)}
        us = {k: [] for k in variants}
        with torch.no_grad():
            for w in range(windows + 1):          # the first window warms up
                for name, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for c in range(calls):
                        fn(c)
                    e1.record()
                    torch.cuda.synchronize()
                    if w:
                        us[name].append(e0.elapsed_time(e1) * 1e3 / calls)
        r = {"site": site, "shape": list(x.shape), "bytes_moved": 8 * x.numel()}
        for name, v in us.items():
            r[name] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        out["sites"].append(r)
    return out


def native_image_train_ab(batch, steps, warmup, windows=5, model_kind="ImageSegBilinear"):
    """Step time of the three ways the ViT trunk trains, vit_linear_impl="ftx_split", with the method of _switch_ab: three models from
    one seed in one process -- `graphs` (the switch off, the trunk as HIP graphs: the default path), `eager` (the switch off,
    vit_graphs=False) and `native` (Image2DTransformer.set_native_train) -- windows of `steps` steps alternating between them; median
    (min..max) ms per step, and per arm the loop's wall clock per step before the synchronise (the host-issue bound), the autograd nodes
    under the image logits and the peak of torch's allocator above what was resident; for `native` the bytes of its arenas in one step."""
    import time
    from fusiontransformer_amd import config
    from fusiontransformer_amd import native_image_train as nit
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    _, res = zip(*[_inputs(batch, cycle, "cuda") for cycle in (0, 1)])
    arms, nets = {}, {}
    for mode in ("graphs", "eager", "native"):      # the captures of `graphs` come first (its warm-up window runs first, too)
        cfg = config.image_cfg() if model_kind == "ImageSegBilinear" else config.fusion_cfg(model_kind)
        cfg.MODEL.vit_linear_impl = "ftx_split"
        cfg.MODEL.vit_graphs = mode != "eager"
        cfg.MODEL.image_native_train = mode == "native"
        torch.manual_seed(0)
        model = build_model(cfg)[0].cuda().train()
        nets[mode] = model.image_backbone
        arms[mode] = TrainStep(cfg, model)
    info = {m: {} for m in arms}

    def window(mode, n):
        step = arms[mode]
        seq = [res[i % 2] for i in range(n + 1)]
        for x in seq:
            x["lidar"].prepared = None
        torch.cuda.synchronize()
        resident = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(n):
            preds = step(seq[i], next_batch=seq[i + 1])
        e1.record()
        host = (time.perf_counter() - t0) * 1e3 / n
        torch.cuda.synchronize()
        info[mode].setdefault("host_issue_ms", []).append(host)
        info[mode]["autograd_nodes"] = _graph_nodes(preds["img_seg_logit"])
        info[mode]["peak_above_resident_bytes"] = int(torch.cuda.max_memory_allocated() - resident)
        return e0.elapsed_time(e1) / n

    for mode in arms:
        window(mode, warmup)
        info[mode]["host_issue_ms"] = []
    ms = {m: [] for m in arms}
    order = list(arms)
    for w in range(windows):
        for mode in order[w % 3:] + order[:w % 3]:
            ms[mode].append(window(mode, steps))
    spread = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
    out = {"model": model_kind, "vit_linear_impl": "ftx_split", "batch": batch, "steps_per_window": steps, "windows": windows,
           "ms_per_step": {m: spread(v) for m, v in ms.items()}, "ms_per_step_windows": ms}
    for m in arms:
        out[m] = dict(info[m], host_issue_ms=spread(info[m]["host_issue_ms"]))
    trunk = nets["native"].backbone
    out["native"]["reason"] = trunk.native_train_reason()
    out["graphs"]["graph_state"] = nets["graphs"].backbone.graph_state()
    ex = trunk.__dict__.get("_native_tr")
    if ex is not None and trunk.native_train_reason() is None:
        ends, first, total = trunk._segment_ends(), 0, 0
        tokens = trunk.num_tokens + trunk.patch_embed.num_patches
        for e in ends:
            total += nit.arena_bytes(ex.model(tokens), len(ex.live()), first, e, batch)
            first = e + 1
        out["native"]["arena_bytes_per_step"] = int(total)
        out["native"]["segments"] = len(ends)
    for other in ("graphs", "eager"):
        out["every_native_window_beats_every_%s_window" % other] = bool(max(ms["native"]) < min(ms[other]))
        out["every_%s_window_beats_every_native_window" % other] = bool(max(ms[other]) < min(ms["native"]))
    return out


def native_stems_ab(batch, steps, warmup, windows=5, model_kind="ImageSegBilinear"):
    """Step time of the image branch with the patch embedding and the tap stems on the library's training forms
    (cfg.MODEL.image_native_stems) against the switch off, vit_linear_impl="ftx_split", the trunk as HIP graphs in both arms (the default
    path), with the method and the rule of native_image_train_ab: two models from one seed in one process, windows of `steps` steps
    alternating between them; median (min..max) ms per step, per arm the host-issue time, the stem nodes under the image logits and the peak
    of torch's allocator above what was resident (the unfold copy and the strip copies go away)."""
    import time
    from fusiontransformer_amd import config
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    _, res = zip(*[_inputs(batch, cycle, "cuda") for cycle in (0, 1)])
    arms, nets = {}, {}
    for mode in ("off", "on"):
        cfg = config.image_cfg() if model_kind == "ImageSegBilinear" else config.fusion_cfg(model_kind)
        cfg.MODEL.vit_linear_impl = "ftx_split"
        cfg.MODEL.image_native_stems = mode == "on"
        torch.manual_seed(0)
        model = build_model(cfg)[0].cuda().train()
        nets[mode] = model.image_backbone
        arms[mode] = TrainStep(cfg, model)
    info = {m: {} for m in arms}

    def window(mode, n):
        step = arms[mode]
        seq = [res[i % 2] for i in range(n + 1)]
        for x in seq:
            x["lidar"].prepared = None
        torch.cuda.synchronize()
        resident = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for i in range(n):
            preds = step(seq[i], next_batch=seq[i + 1])
        e1.record()
        host = (time.perf_counter() - t0) * 1e3 / n
        torch.cuda.synchronize()
        info[mode].setdefault("host_issue_ms", []).append(host)
        info[mode]["stem_nodes"] = _named_nodes(preds["img_seg_logit"], ("_VitPatchEmbed", "_VitTapStem"))
        info[mode]["peak_above_resident_bytes"] = int(torch.cuda.max_memory_allocated() - resident)
        return e0.elapsed_time(e1) / n

    for mode in arms:
        window(mode, warmup)
        info[mode]["host_issue_ms"] = []
    ms = {m: [] for m in arms}
    order = list(arms)
    for w in range(windows):
        for mode in order[w % 2:] + order[:w % 2]:
            ms[mode].append(window(mode, steps))
    spread = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}
    out = {"model": model_kind, "vit_linear_impl": "ftx_split", "batch": batch, "steps_per_window": steps, "windows": windows,
           "ms_per_step": {m: spread(v) for m, v in ms.items()}, "ms_per_step_windows": ms}
    for m in arms:
        out[m] = dict(info[m], host_issue_ms=spread(info[m]["host_issue_ms"]), reason=nets[m].native_stems_reason(),
                      graph_state=nets[m].backbone.graph_state())
    out["every_on_window_beats_every_off_window"] = bool(max(ms["on"]) < min(ms["off"]))
    out["every_off_window_beats_every_on_window"] = bool(max(ms["off"]) < min(ms["on"]))
    return out


def lidar_split_ab(batch, steps, warmup, windows=5):
    """LidarSeg step time with the default exact-fp32 sparse convolution and with SPVCNN.set_split (the three-piece split kernels): two
    models from one seed in one process, `windows` windows of `steps` steps each, alternating."""
    return _switch_ab("split", batch, steps, warmup, windows, "LidarSeg")


def native_train_steps(mode, steps):
    """`steps` untimed LidarSeg steps at batch 1 with the training executor on / off: run under a kernel trace with two step counts, the
    difference of the two launch counts is the launches of the extra steps."""
    from fusiontransformer_amd import config
    from fusiontransformer_amd.models.build import build_model
    from fusiontransformer_amd.trainer import TrainStep
    cfg = config.lidar_cfg()
    torch.manual_seed(0)
    model = build_model(cfg)[0].cuda().train()
    model.backbone.set_native_train(mode == "on")
    step = TrainStep(cfg, model)
    _, res = zip(*[_inputs(1, cycle, "cuda") for cycle in (0, 1)])
    for i in range(steps):
        step(res[i % 2], next_batch=res[(i + 1) % 2])
    torch.cuda.synchronize()
    return {"native_train": mode, "steps": steps, "last_loss": next(iter(step.last.values())).item()}


def kernel_times():
    from fusiontransformer_amd import _lib
    from fusiontransformer_amd._lib import check, ptr
    L = _lib.load()
    n, c = N_KERNEL, C_KERNEL
    torch.manual_seed(0)
    x = torch.randn(n, c, device="cuda")
    label = torch.randint(0, c, (n,), device="cuda")
    cw = torch.rand(c, device="cuda") + 0.5
    g, g2 = torch.empty_like(x), torch.empty_like(x)
    loss, losses = torch.zeros(1, device="cuda"), torch.zeros(2, device="cuda")
    ws = torch.empty(max(int(L.ftx_seg_loss_workspace_bytes()), int(L.ftx_fusion_loss_workspace_bytes())), dtype=torch.uint8, device="cuda")

    def seg(grad):
        check(L.ftx_seg_loss(ptr(x), ptr(label), ptr(cw), n, c, 0, ptr(loss), ptr(g) if grad else None, None, ptr(ws), ws.numel(), _lib.stream()),
              "ftx_seg_loss")

    def two_head():
        check(L.ftx_fusion_loss_mix(ptr(x), ptr(x), None, None, ptr(label), ptr(cw), 1.0, 0.0, n, c, 0, ptr(losses), ptr(g), ptr(g2), None, None,
                                    None, None, ptr(ws), ws.numel(), _lib.stream()), "ftx_fusion_loss_mix")

    variants = {"seg_loss_grad": lambda: seg(True), "seg_loss_forward_only": lambda: seg(False), "fusion_loss_mix_same_tensor_twice": two_head}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    two_head()
    seg(True)
    torch.cuda.synchronize()
    assert loss.item() == losses[1].item() == losses[0].item(), "the two kernels disagree on the loss"
    graphs = {}
    for name, fn in variants.items():
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(CALLS):
                fn()
        graphs[name] = gr

    def timed(run):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / CALLS

    def eager(fn):
        for _ in range(CALLS):
            fn()

    for name in variants:          # warm-up window
        timed(graphs[name].replay)
        timed(lambda: eager(variants[name]))
    us = {name: {"graph": [], "eager": []} for name in variants}
    for _ in range(WINDOWS):       # alternated: one window of each variant after the other
        for name in variants:
            us[name]["graph"].append(timed(graphs[name].replay))
        for name in variants:
            us[name]["eager"].append(timed(lambda: eager(variants[name])))
    out = {"n": n, "c": c, "calls_per_window": CALLS, "windows": WINDOWS, "unit": "us per call (3 launches)"}
    for name, d in us.items():
        out[name] = {how: {"median": statistics.median(v), "min": min(v), "max": max(v)} for how, v in d.items()}
    a, b = out["seg_loss_grad"]["graph"], out["fusion_loss_mix_same_tensor_twice"]["graph"]
    out["seg_loss_grad_not_slower_than_two_head_call"] = bool(a["median"] <= b["median"] + (b["max"] - b["min"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "single_modality_steps.json"))
    ap.add_argument("--image-stn", action="store_true", help="only: step time of ImageSeg (spatial transformers) beside ImageSegBilinear, batch 4 and 1")
    ap.add_argument("--stn-loc", default="library", choices=["library", "ftx", "both"],
                    help="with --image-stn: what runs ImageSeg's localisation nets (cfg.MODEL.stn_loc_impl); both = one after the other")
    ap.add_argument("--native-index-ab", action="store_true", help="only: LidarSeg step time with SPVCNN.set_native_index off / on, batch 1 and 4")
    ap.add_argument("--native-train-ab", action="store_true", help="only: step time with SPVCNN.set_native_train off / on, batch 1 and 4")
    ap.add_argument("--dropout", action="store_true", help="with --native-train-ab: the executor on in both arms, torch's Dropout / five segments "
                                                           "against SPVCNN.set_native_dropout / three segments, batch 1 and 4; then the kernel's time")
    ap.add_argument("--ab-model", default="LidarSeg", choices=["LidarSeg", "middle"], help="the model of --native-train-ab")
    ap.add_argument("--native-image-train-ab", action="store_true",
                    help="only: ImageSegBilinear and middle-fusion step time, vit_linear_impl=ftx_split, trunk as HIP graphs / eager / native training "
                         "executor (Image2DTransformer.set_native_train), batch 1 and 4")
    ap.add_argument("--native-stems-ab", action="store_true",
                    help="only: ImageSegBilinear and middle-fusion step time, vit_linear_impl=ftx_split, cfg.MODEL.image_native_stems off / on, "
                         "batch 1 and 4")
    ap.add_argument("--native-train-steps", choices=["on", "off"], help="only: --steps untimed LidarSeg batch-1 steps with the switch on / off")
    ap.add_argument("--lidar-split", action="store_true", help="only: LidarSeg step time with SPVCNN.set_split off / on, batch 4 and 1; --out writes the JSON")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_single: needs a GPU (there is no fallback)")
    if args.native_train_ab and args.dropout:
        for batch in (1, 4):
            print(json.dumps(native_dropout_ab(batch, args.steps, args.warmup)), flush=True)
        print(json.dumps(dropout_kernel_times()), flush=True)
        return
    if args.native_train_ab:
        for batch in (1, 4):
            print(json.dumps(native_train_ab(batch, args.steps, args.warmup, model_kind=args.ab_model)), flush=True)
        return
    if args.native_image_train_ab:
        for kind in ("ImageSegBilinear", "middle"):
            for batch in (1, 4):
                print(json.dumps(native_image_train_ab(batch, args.steps, args.warmup, model_kind=kind)), flush=True)
        return
    if args.native_stems_ab:
        for kind in ("ImageSegBilinear", "middle"):
            for batch in (1, 4):
                print(json.dumps(native_stems_ab(batch, args.steps, args.warmup, model_kind=kind)), flush=True)
        return
    if args.native_train_steps:
        print(json.dumps(native_train_steps(args.native_train_steps, args.steps)), flush=True)
        return
    if args.lidar_split:
        result = {"what": "LidarSeg train steps on synthetic KITTI-shaped frames (two alternating resident batches, HIP events, profiler off): the "
                          "default exact-fp32 sparse convolution (off) against lidar_split (on), two models from one seed in one process, five "
                          "windows each, alternating; median and min..max ms per step over the windows",
                  "device": torch.cuda.get_device_name(0), "ab": []}
        for batch in (4, 1):
            r = lidar_split_ab(batch, args.steps, args.warmup)
            print(json.dumps(r), flush=True)
            result["ab"].append(r)
        if args.out != ap.get_default("out"):
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
            print("wrote", args.out)
        return
    if args.native_index_ab:
        for batch in (1, 4):
            print(json.dumps(native_index_ab(batch, args.steps, args.warmup)), flush=True)
        return
    if args.steps < 50:
        raise SystemExit("bench_single: at least 50 timed steps")
    if args.image_stn:
        result = {"what": "image-only train steps on synthetic KITTI-shaped frames (two alternating resident batches, HIP events, profiler "
                          "off): ImageSeg (learned affine resampling, eager trunk; stn_loc_impl says what runs the localisation nets' "
                          "convolutions: torch's library, or the fused kernels of csrc/ftx_stn_loc.hip) beside ImageSegBilinear (fixed "
                          "nearest resampling, trunk as HIP graphs); one run each, no spread claimed",
                  "device": torch.cuda.get_device_name(0), "steps": []}
        runs = [("ImageSegBilinear", None)] + [("ImageSeg", impl) for impl in (("library", "ftx") if args.stn_loc == "both" else (args.stn_loc,))]
        for kind, impl in runs:
            for batch in (4, 1):
                r = step_time(kind, batch, args.steps, args.warmup, stn_loc=impl)
                print(json.dumps(r), flush=True)
                result["steps"].append(r)
        out = args.out if args.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "image_stn_steps.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(result, f, indent=1)
        print("wrote", out)
        return
    result = {"what": "single-modality train steps on synthetic KITTI-shaped frames (two alternating resident batches, HIP events, "
                      "profiler off) and the single-head loss kernel beside the fused two-head kernel fed one tensor twice",
              "device": torch.cuda.get_device_name(0), "steps": []}
    for kind in ("LidarSeg", "ImageSegBilinear"):
        for batch in (4, 1):
            r = step_time(kind, batch, args.steps, args.warmup)
            print(json.dumps(r), flush=True)
            result["steps"].append(r)
    result["loss_kernel"] = kernel_times()
    print(json.dumps(result["loss_kernel"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
