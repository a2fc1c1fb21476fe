"""The pillar SECOND from raw points (cfg.PILLAR.PLAN: vision3d_amd/pillar_plan.py, csrc/pillar.hip "the plan's front") on 16k-point
KITTI-like clouds (vision3d_amd.synth), on one device in one process, on the same inputs --
    frames/s at B = 1:  eager Second.inference(item) (the path without the key; the Preprocessor outside the clock), inference_points,
                        one captured-graph slot, the autotuned pipeline
    launches per graph replay, from a profiled pass
    the new kernel (clear + encode into planes) beside v3d_pillar_encode + .dense() + to_split_nhwc, the voxelizer in front of both
    the f16s error figures of tests/test_gpu_pillar_plan.py (fused head maps against float64 on the tiny grid)
and, given with --bench / --parent-bench, the result lines of `python bench.py --steps 300 --warmup 30` on this tree and on the parent.

    python tools/mb_pillar_plan.py [--out profiles/pillar_plan.txt] [--windows 7] [--reps 20] [--bench FILE --parent-bench FILE]

Device-plus-host time: a host clock around `reps` calls that end in a device synchronise, inputs resident on the device, medians
over repeated windows after a warm-up (lowest .. highest window given), the versions alternating window by window.  The output is
written to --out with the command line."""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from vision3d_amd import synth  # noqa: E402
from vision3d_amd.core import AnchorGenerator, Preprocessor  # noqa: E402
from vision3d_amd.core.config import pillar_car_cfg, pillar_plan_car_cfg  # noqa: E402
from vision3d_amd.detector import Second  # noqa: E402

LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def compare(named, windows, reps):
    """named: [(name, fn)] timed in alternating windows (all see the same drift of the host); ratios against the first."""
    for _, fn in named:
        fn(), fn(), fn()
    times = [[] for _ in named]
    for _ in range(windows):
        for t, (_, fn) in zip(times, named):
            t.append(window(fn, reps))
    med = [statistics.median(t) for t in times]
    for (name, _), t, m in zip(named, times, med):
        tail = "" if m is med[0] else f"   ratio {m / med[0]:.2f}x"
        say(f"  {name}: {m * 1e6:9.1f} us per call ({min(t) * 1e6:.1f} .. {max(t) * 1e6:.1f}), {1 / m:7.0f} per s{tail}")
    return med


def kernel_times(fn, calls=10):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    launches = 0
    for ev in prof.key_averages():
        total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
        if total <= 0:
            continue
        launches += ev.count
        name = (ev.key.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").strip() or ev.key)[:60]
        say(f"  kernel {name}: {total / max(ev.count, 1):7.1f} us per launch, {ev.count / calls:g} per call")
    say(f"  launches (kernels, fills and copies) per call: {launches / calls:g}")


def f16s_errors():
    """The figures of tests/test_gpu_pillar_plan.py::test_f16s_head_maps_against_float64, computed the same way."""
    import test_gpu_pillar_plan as T
    from vision3d_amd.detector.proposal import fused_convs
    cfg, model, anchors = T._model()
    clouds = T._clouds((0, 1))
    item = T._item(cfg, clouds, anchors)
    m64 = copy.deepcopy(model).cpu().double()
    with torch.no_grad():
        plan_maps = model.fused_head_from_points(clouds)
        module_maps = model.head.native_head(model.rpn(model.vfe(item)))
        item64 = dict(features=item["features"].cpu(), occupancy=item["occupancy"].cpu(), coordinates=item["coordinates"].cpu(), batch_size=2)
        feats = m64.rpn.fused_forward(m64.vfe.forward_torch(item64))
        want = torch.cat([c(feats) for c in fused_convs(m64.head)], 1)
    top = float(want.abs().max())
    err_plan = float((plan_maps.cpu().double() - want).abs().max()) / top
    err_module = float((module_maps.cpu().double() - want).abs().max()) / top
    say("f16s fused head maps against float64 (model.double() on the CPU), tiny grid 20 x 16, two clouds, largest |error| relative to the")
    say(f"  largest |reference| entry ({top:.3f}): plan path (fused_head_from_points) {err_plan:.3e}, module path head(rpn(vfe(item))) "
        f"{err_module:.3e}, ratio {err_plan / max(err_module, 1e-30):.2f} (the test's bar: 2)")


def bench_line(path):
    """The last JSON line of a bench.py output file -> its headline numbers as text."""
    if not path or not os.path.exists(path):
        return "not given"
    rec = None
    for line in open(path):
        line = line.strip()
        if line.startswith("{"):
            try:
                rec = json.loads(line)
            except ValueError:
                pass
    if rec is None:
        return "no result line"
    keep = {k: rec[k] for k in ("metric", "value", "unit", "ms_per_step", "single_frame_ms", "steps", "windows") if k in rec}
    return json.dumps(keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pillar_plan.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--bench", default=None, help="output of `python bench.py --steps 300 --warmup 30` on this tree")
    ap.add_argument("--parent-bench", default=None, help="... on the parent commit")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    say("$ python tools/mb_pillar_plan.py " + " ".join(sys.argv[1:]))
    say(f"device: {torch.cuda.get_device_name(0)}")
    f16s_errors()

    cfg = pillar_plan_car_cfg()
    anchors = AnchorGenerator(cfg).anchors.cuda()
    torch.manual_seed(0)
    model = Second(cfg).cuda().eval()
    cloud_np = synth.make_cloud(0, n_points=16384)
    cloud = torch.from_numpy(cloud_np).cuda()
    item = Preprocessor(pillar_car_cfg())(dict(points=[cloud_np], anchors=anchors))
    M, Pn, C = item["features"].shape
    say(f"B = 1, one 16k-point cloud: {M} pillars x {Pn} slots x {C} channels -> 200 x 176 x 128 map; arithmetic {model.precision}")

    # ---- the front alone: what stands between the voxelizer's outputs and the dense head's input
    from vision3d_amd import _lib as L
    from vision3d_amd.detector.pillar import pillar_encode
    from vision3d_amd.runtime import to_split_nhwc
    net = model.vfe
    plan = model.backbone_plan(1, 16384)
    with torch.no_grad():
        plan.forward_split(cloud, [0, 16384], persistent=True)  # (calibrates; leaves the frame's voxels in the plan)
        plan.forward_split(cloud, [0, 16384], persistent=True)
    scale, shift = net._folded()
    h, w = plan.map_shape
    lib = L.lib()

    def parent_front():
        with torch.no_grad():
            rows = pillar_encode(item["features"], item["occupancy"], item["coordinates"], net.geom, net.linear.weight.detach(), scale, shift)
            to_split_nhwc(net.canvas(rows, item["coordinates"], 1), model.precision)

    def plan_front():  # the persistent form a graph replays: clear by the kept list, encode into the plan's planes
        plan._clear(True)
        L.check(lib.v3d_pillar_encode_planes(L.ptr(plan.slots), L.ptr(plan.occupancy), L.ptr(plan.coords[1]), L.ptr(plan.counts[1:2]), plan.cap,
                                             plan.P, plan.C, L.host_f32(net.geom), L.ptr(net.linear.weight.detach()), 128, L.ptr(scale),
                                             L.ptr(shift), 1, h, w, L.PRECISIONS[plan.precision], L.ptr(plan.bev_entry()),
                                             L.ptr(plan.summary) if plan.f16s else None, L.ptr(plan.planes[0]), L.ptr(plan.planes[1]),
                                             L.ptr(plan.bitmap), L.stream_ptr()), "pillar_encode_planes")

    def plan_frame():
        with torch.no_grad():
            plan.forward_split(cloud, [0, 16384], persistent=True)
    say("the front alone (same pillars; the plan's side sized by its capacity, the count read on the device):")
    compare([("v3d_pillar_encode + .dense() + to_split_nhwc (f16s: + its entry)", parent_front),
             ("v3d_pillar_planes_clear + v3d_pillar_encode_planes            ", plan_front),
             ("... with v3d_voxelize in front (PillarPlan.forward_split)     ", plan_frame)], a.windows, a.reps)
    say("profiled pass, v3d_pillar_encode + .dense() + to_split_nhwc:")
    kernel_times(parent_front)
    say("profiled pass, PillarPlan.forward_split(persistent=True):")
    kernel_times(plan_frame)

    # ---- frames/s
    def eager_item():
        with torch.no_grad():
            model.inference(item)

    def points():
        with torch.no_grad():
            model.inference_points([cloud], anchors)
    with torch.no_grad():
        graphed = model.graphed_inference(anchors, [16384])
        n_eager, n_points, n_graph = len(model.inference(item)[0]), len(model.inference_points([cloud], anchors)[0]), len(graphed([cloud])[0])
    say(f"detections: inference(item) {n_eager}, inference_points {n_points}, graphed {n_graph}")

    def one_slot():
        graphed([cloud])
    say("frames/s, B = 1 (per call = per frame):")
    compare([("eager Second.inference(item), voxelizer outside the clock", eager_item),
             ("Second.inference_points (voxelizer inside)              ", points),
             ("one captured-graph slot (load + replay + finalize)      ", one_slot)], a.windows, a.reps)
    say("profiled pass, one graph replay (kernels of the graph, then the finalize's copies):")
    kernel_times(one_slot)
    with torch.no_grad():
        pipe = model.pipelined_inference(anchors, [16384], depth=4, autotune=True)
        pipe.tune([cloud], window_frames=64)
    say(f"autotuned pipeline: {pipe.tuned}")

    def pipelined(frames=200):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(frames):
            pipe([cloud])
        pipe.flush()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / frames
    pipelined(50)
    t = [pipelined() for _ in range(a.windows)]
    say(f"  autotuned pipeline, windows of 200 frames: {statistics.median(t) * 1e6:9.1f} us per frame ({min(t) * 1e6:.1f} .. {max(t) * 1e6:.1f}), "
        f"{1 / statistics.median(t):7.0f} per s")
    say("bench.py --steps 300 --warmup 30 (the flagship workload, sparse SECOND; this change does not touch its path):")
    say(f"  this tree: {bench_line(a.bench)}")
    say(f"  parent:    {bench_line(a.parent_bench)}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
