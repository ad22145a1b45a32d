"""Eval-mode forward of the LiDAR-only and the middle-fusion model with the native executor of the LiDAR branch off and on
(SPVCNN.set_native_eval), and -- mode `index` -- with the executor AND the native index build on (SPVCNN.set_native_index), profiler
off.  Two resident batches alternate, so every per-batch structure is rebuilt in every forward.

Per (model, batch, switch) and over `--windows` windows of `--steps` forwards, the switch alternating window by window in one process:
  wall ms / forward   host clock around the window, ending in a device synchronise
  issue ms / forward  host clock until the last launch of the window has returned, before the synchronise (the forwards are issued
                      back to back, so this is what the host needs per forward, host reads of the index build included)
  lidar ms / forward  HIP events on the stream that runs the LiDAR branch, from the end of the previous forward's work to the end of
                      this one's
  arena / peak bytes  the executor's arena, and torch's peak allocation above the resident state during a window
Mode `image` is a measurement of its own: the same eval workload on the fusion models with vit_linear_impl="ftx_split" (the fp32
linears the library owns), the native executor of the IMAGE branch (Net2DBillinear.set_native_eval) off and on, the LiDAR branch on its
default path.  It reports wall and issue ms as above and the HIP-event time of the stream that runs the image branch.
usage:
  python tools/bench_eval.py [--models lidar,middle] [--batches 1,4] [--windows 5] [--steps 20] [--modes off,on,index]
  python tools/bench_eval.py --modes image [--models middle] [--batches 1,4]       # A/B of the image branch's switch
      --modes off also runs on a checkout that has no executor (the baseline of the comparison)
      --mark-launches also traces one index build on its own per setting ("... index build" in the count)
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_eval.py --mark-launches   # one marked forward per setting
  python tools/bench_eval.py --count-launches DIR                                                     # kernel launches per forward
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
MARK = "cosh"        # a torch kernel nothing else in the program launches: one between forwards cuts the trace


def count_launches(trace_dir):
    kt = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(kt)), key=lambda r: int(r["Start_Timestamp"]))
    order = json.load(open(os.path.join(trace_dir, "order.json")))
    marks = [i for i, r in enumerate(rows) if MARK in r["Kernel_Name"]]
    assert len(marks) == 2 * len(order), (len(marks), len(order))
    for j, what in enumerate(order):
        lo, hi = marks[2 * j], marks[2 * j + 1]
        ours = sum(1 for r in rows[lo + 1:hi] if "ftx" in r["Kernel_Name"] or "spconv" in r["Kernel_Name"] or "bn_" in r["Kernel_Name"])
        print("%-40s %5d kernel launches per forward (%d with 'ftx' / 'spconv' / 'bn_' in the name)" % (what, hi - lo - 1, ours))
        if what.endswith("index build"):
            names = {}
            for r in rows[lo + 1:hi]:
                k = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").split("<")[0][-40:]
                names[k] = names.get(k, 0) + 1
            busy = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows[lo + 1:hi]) / 1e3
            span = (int(rows[hi - 1]["End_Timestamp"]) - int(rows[lo + 1]["Start_Timestamp"])) / 1e3 if hi - lo > 1 else 0.0
            print("    kernels busy %.1f us inside a span of %.1f us: %s" % (busy, span, ", ".join("%s x%d" % kv for kv in sorted(names.items(), key=lambda kv: -kv[1]))))


def image_ab(a):
    """Mode `image`: Net2DBillinear.set_native_eval off / on, alternating window by window in one process."""
    import torch
    from bench import build_inputs
    from fusiontransformer_amd import gemm_tuning
    from fusiontransformer_amd.config import fusion_cfg
    from fusiontransformer_amd.models._fusion_common import _branch_streams
    from fusiontransformer_amd.models.build import build_model
    assert torch.cuda.is_available(), "bench_eval measures on the GPU; there is no CPU figure"
    gemm_tuning.enable(0)
    dev = torch.device("cuda")
    fmt = lambda v: "%.3f (%.3f..%.3f)" % (statistics.median(v), min(v), max(v))
    for kind in (k for k in a.models.split(",") if k != "lidar"):
        cfg = fusion_cfg(kind)
        cfg.MODEL.vit_linear_impl = "ftx_split"
        torch.manual_seed(0)
        model = build_model(cfg)[0].cuda().eval()
        net = model.image_backbone
        if not hasattr(net, "set_native_eval"):
            sys.exit("this checkout has no native executor of the image branch")
        image_stream = _branch_streams(dev)[0]
        for batch in (int(b) for b in a.batches.split(",")):
            datas = [build_inputs(cfg, batch, "kitti", 0, dev, cycle=c)[1] for c in range(2)]
            with torch.no_grad():
                for on in (False, True):
                    net.set_native_eval(on)
                    for i in range(a.warmup):
                        model(datas[i % 2])
                    assert not on or net.native_eval_reason() is None, net.native_eval_reason()
                torch.cuda.synchronize()
                res = {on: {"wall": [], "issue": [], "image": []} for on in (False, True)}
                for w in range(a.windows):
                    for on in ((False, True) if w % 2 == 0 else (True, False)):
                        net.set_native_eval(on)
                        model(datas[1])
                        torch.cuda.synchronize()
                        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                        ev[0].record(image_stream)
                        t0 = time.perf_counter()
                        for i in range(a.steps):
                            model(datas[i % 2])
                        ev[1].record(image_stream)
                        t1 = time.perf_counter()
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                        r = res[on]
                        r["wall"].append((t2 - t0) / a.steps * 1e3)
                        r["issue"].append((t1 - t0) / a.steps * 1e3)
                        r["image"].append(ev[0].elapsed_time(ev[1]) / a.steps)
                        r["arena"] = sum(b.shape[0] for b in net._native.arenas.values()) if (on and net._native) else 0
                for on in (False, True):
                    r = res[on]
                    arena = r.get("arena", 0)
                    print("%-6s batch %d image native %-3s  wall %s ms  issue %s ms  image stream %s ms  arena %.1f MiB" % (
                        kind, batch, "on" if on else "off", fmt(r["wall"]), fmt(r["issue"]), fmt(r["image"]), arena / 2 ** 20), flush=True)
        del model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="lidar,middle")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--mark-launches", action="store_true")
    ap.add_argument("--count-launches", metavar="DIR")
    ap.add_argument("--order-file", default=None)
    a = ap.parse_args()
    if a.count_launches:
        return count_launches(a.count_launches)
    if a.modes == "image":
        return image_ab(a)

    import torch
    from bench import build_inputs
    from fusiontransformer_amd import gemm_tuning
    from fusiontransformer_amd.config import fusion_cfg, lidar_cfg
    from fusiontransformer_amd.models._fusion_common import _branch_streams
    from fusiontransformer_amd.models.build import build_model
    assert torch.cuda.is_available(), "bench_eval measures on the GPU; there is no CPU figure"
    gemm_tuning.enable(0)
    dev = torch.device("cuda")
    modes = a.modes.split(",")
    order = []
    marker = torch.zeros(8, device=dev)
    for kind in a.models.split(","):
        cfg = lidar_cfg() if kind == "lidar" else fusion_cfg(kind)
        torch.manual_seed(0)
        model = build_model(cfg)[0].cuda().eval()
        net = model.backbone if kind == "lidar" else model.lidar_backbone
        if "on" in modes and not hasattr(net, "set_native_eval"):
            sys.exit("this checkout has no native executor: run with --modes off")
        lidar_stream = torch.cuda.current_stream() if kind == "lidar" else _branch_streams(dev)[1]

        if "index" in modes and not hasattr(net, "set_native_index"):
            sys.exit("this checkout has no native index build: run without the mode `index`")

        def switch(mode):
            if hasattr(net, "set_native_eval"):
                net.set_native_eval(mode in ("on", "index"))
            if hasattr(net, "set_native_index"):
                net.set_native_index(mode == "index")

        for batch in (int(b) for b in a.batches.split(",")):
            datas = [build_inputs(cfg, batch, "kitti", 0, dev, cycle=c)[1] for c in range(2)]
            with torch.no_grad():
                for mode in modes:
                    switch(mode)
                    for i in range(a.warmup):
                        model(datas[i % 2])
                torch.cuda.synchronize()
                if a.mark_launches:
                    for mode in modes:
                        switch(mode)
                        torch.cuda.synchronize()
                        marker.cosh_()
                        model(datas[0])
                        torch.cuda.synchronize()
                        marker.cosh_()
                        order.append("%s batch %d %s" % (kind, batch, mode))
                        # the index build alone (coordinate structures of one batch, both host reads included)
                        from fusiontransformer_amd.sparse import drain
                        marker.cosh_()
                        drain(net._index_steps(datas[0]["lidar"], ahead=True))
                        torch.cuda.synchronize()
                        marker.cosh_()
                        order.append("%s batch %d %s index build" % (kind, batch, mode))
                    continue
                res = {m: {"wall": [], "issue": [], "lidar": [], "peak": 0} for m in modes}
                for w in range(a.windows):
                    for mode in (modes if w % 2 == 0 else modes[::-1]):
                        switch(mode)
                        model(datas[1])
                        torch.cuda.synchronize()
                        base = torch.cuda.memory_allocated()
                        torch.cuda.reset_peak_memory_stats()
                        ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps + 1)]
                        ev[0].record(lidar_stream)
                        t0 = time.perf_counter()
                        for i in range(a.steps):
                            model(datas[i % 2])
                            ev[i + 1].record(lidar_stream)
                        t1 = time.perf_counter()
                        torch.cuda.synchronize()
                        t2 = time.perf_counter()
                        r = res[mode]
                        r["wall"].append((t2 - t0) / a.steps * 1e3)
                        r["issue"].append((t1 - t0) / a.steps * 1e3)
                        r["lidar"].append(ev[0].elapsed_time(ev[-1]) / a.steps)
                        r["peak"] = max(r["peak"], torch.cuda.max_memory_allocated() - base)
                for mode in modes:
                    r = res[mode]
                    arena = sum(b.shape[0] for b in net._native.arenas.values()) if (mode != "off" and getattr(net, "_native", None)) else 0
                    fmt = lambda v: "%.3f (%.3f..%.3f)" % (statistics.median(v), min(v), max(v))
                    print("%-6s batch %d native %-3s  wall %s ms  issue %s ms  lidar stream %s ms  arena %.1f MiB  torch peak %.1f MiB" % (
                        kind, batch, mode, fmt(r["wall"]), fmt(r["issue"]), fmt(r["lidar"]), arena / 2 ** 20, r["peak"] / 2 ** 20), flush=True)
        del model
    if a.mark_launches:
        json.dump(order, open(a.order_file or "order.json", "w"))


if __name__ == "__main__":
    main()
