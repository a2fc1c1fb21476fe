"""Time per frame of cutting the GT-sampling database objects out of 64 KITTI-size frames (16 384 points, the 27 boxes of
synth.make_gt_boxes): the batched device path (`extract_objects`, csrc/database.hip) against the chain of existing operators it
replaces and against the reference's numpy expressions.

    python tools/mb_database.py [--frames 64] [--windows 7] [--numpy-frames 8]

Device-plus-host time: a host clock around calls that end in a device synchronise, clouds resident on the device, medians over
repeated windows after a warm-up of every shape.  The kernels' own times come from a separate profiled pass."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision3d_amd import synth  # noqa: E402
from vision3d_amd.core.geometry import points_in_boxes_mask  # noqa: E402
from vision3d_amd.dataset import extract_objects  # noqa: E402

MIN_PTS = 8


def operator_chain(points, boxes):
    """core.geometry.PointsInCuboids as it stands (mask -> .T -> one gather per box) + the keep rule + the de-mean, in torch."""
    mask = points_in_boxes_mask(points, boxes).T
    out = []
    for m, box in zip(mask, boxes):
        p = points[m]
        if p.shape[0] > MIN_PTS:
            out.append(torch.cat(((p[:, :2].double() - box[:2].double()).float(), p[:, 2:]), 1))
    return out


def numpy_reference(points, boxes):
    """The reference's expressions (geometry.py:4-51, augmentation.py:219-236) restated: float64 boxes, one CPU core."""
    xy, _, wl, _, yaw = np.split(boxes, [2, 3, 5, 6], 1)
    c, s = np.cos(yaw), np.sin(yaw)
    rot = np.stack([c, -s, s, c], -1).reshape(-1, 2, 2)
    unit = 0.5 * np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]])
    corners = np.einsum("ijk,imk->imj", rot, wl[:, None] * unit) + xy[:, None]
    z = points[:, None, 2]
    mask = (z > boxes[:, 2] - boxes[:, 5] / 2) & (z < boxes[:, 2] + boxes[:, 5] / 2)
    side = -(corners - np.roll(corners, 1, 1))[None]
    to = corners[None] - points[:, None, None, :2]
    mask &= (side[..., 0] * to[..., 1] - side[..., 1] * to[..., 0] > 0).all(2)
    out = []
    for m, box in zip(mask.T, boxes):
        p = points[m]
        if len(p) > MIN_PTS:
            out.append(np.concatenate((p[:, :2] - box[:2], p[:, 2:]), 1))
    return out


def median_window(fn, windows, reps):
    times = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / reps)
    return statistics.median(times), min(times), max(times)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--numpy-frames", type=int, default=8)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    F = args.frames
    clouds = [synth.make_cloud(s, 16384) for s in range(F)]
    boxes64 = [synth.make_gt_boxes(s).astype(np.float64) for s in range(F)]
    dev_clouds = [torch.from_numpy(c).cuda() for c in clouds]
    dev_boxes = [torch.from_numpy(b.astype(np.float32)).cuda() for b in boxes64]
    frames = [dict(points=p, boxes=b, class_idx=np.zeros(len(b), np.int64)) for p, b in zip(dev_clouds, boxes64)]
    n_points, n_boxes = sum(len(c) for c in clouds), sum(len(b) for b in boxes64)

    res = extract_objects(frames, MIN_PTS)
    rows, kept = int(res[0].shape[0]), int(res[1].shape[0])
    chain = [operator_chain(p, b) for p, b in zip(dev_clouds, dev_boxes)]
    assert sum(len(c) for c in chain) == kept and sum(int(o.shape[0]) for c in chain for o in c) == rows, "the two paths disagree"
    print(f"{F} frames, {n_points} points, {n_boxes} boxes -> {kept} objects, {rows} rows (min_pts {MIN_PTS})")

    def batched():
        extract_objects(frames, MIN_PTS)

    def frame_by_frame():
        for fr in frames:
            extract_objects([fr], MIN_PTS)

    def chained():
        for p, b in zip(dev_clouds, dev_boxes):
            operator_chain(p, b)

    for fn in (batched, frame_by_frame, chained):  # warm-up of every shape
        fn(), fn()
    results = {}
    for name, fn, reps in (("existing-operator chain (points_in_boxes + a gather per box)", chained, 1),
                           ("extract_objects, frame by frame", frame_by_frame, 2),
                           ("extract_objects, one batch", batched, 20)):
        med, lo, hi = median_window(fn, args.windows, reps)
        results[name] = med / F
        print(f"{name}: {med / F * 1e6:9.1f} us per frame (median of {args.windows} windows; {lo / F * 1e6:.1f} .. {hi / F * 1e6:.1f})")
    names = list(results)
    print(f"ratio chain / batch: {results[names[0]] / results[names[2]]:.1f}x   chain / frame by frame: "
          f"{results[names[0]] / results[names[1]]:.1f}x")

    k = max(1, min(args.numpy_frames, F))
    t0 = time.perf_counter()
    for c, b in zip(clouds[:k], boxes64[:k]):
        numpy_reference(c, b)
    t_np = (time.perf_counter() - t0) / k
    print(f"numpy reference expressions, one CPU core: {t_np * 1e6:9.1f} us per frame ({k} frames); / batch: {t_np / results[names[2]]:.0f}x")

    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(10):
            batched()
        torch.cuda.synchronize()
    per_kernel = {}
    for ev in prof.key_averages():
        if "db_" in ev.key:
            short = ev.key.split("(")[0].split("<")[0].split()[-1]
            total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            per_kernel[short] = per_kernel.get(short, 0.0) + total / 10
    for name, us in sorted(per_kernel.items()):
        line = f"{name}: {us:8.1f} us per batch"
        if "emit" in name:
            line += f"; reads 16 x {n_points} B + writes 20 x {rows} B -> {(16 * n_points + 20 * rows) / us * 1e-3:.1f} GB/s"
        if "count" in name:
            line += f"; reads 16 x {n_points} B -> {16 * n_points / us * 1e-3:.1f} GB/s"
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
