"""KITTI AP on a KITTI-val-sized synthetic set: times KittiEvaluator.compute() (csrc/kitti_eval.hip) and the float64 host
restatement of BEV / 3-D (tests/kitti_eval_ref.py), and prints the per-kernel split of one compute() (torch profiler device
events).  With bbox or aos in --metrics every detection near a ground truth gets a jitter of its image box and every box a
random alpha, so that the 2-D stages have matches to work on; the host restatement then covers BEV / 3-D only.

    python tools/mb_kitti_eval.py [--frames 3769] [--gt 20] [--dt 100] [--host-frames 3769] [--reps 5] [--metrics bev,3d]
                                  [--overlaps strict,loose]

With coco in --overlaps the ten-level sweep runs as well (the host restatement covers strict / loose only).

For kernel times of record run it under `rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import kitti_eval_ref as R  # noqa: E402

from vision3d_amd.evaluation import KittiEvaluator  # noqa: E402


def make_set(n_frames, n_gt, n_dt, seed=0):
    """~n_gt objects and ~n_dt detections per frame (jittered objects, misses, duplicates, false positives)."""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(n_frames):
        g = int(rng.poisson(n_gt))
        g = min(g, 100)
        fp = max(0, int(rng.poisson(n_dt)) - g)
        fp = min(fp, 144 - g)
        pairs.append(R.synthetic_frame(rng, g, fp, margins=False, spacing=6.0, grid=12))
    return pairs


def with_image_boxes(pairs, seed=1):
    """Each detection within 2 m (x, z) of a ground truth takes a jitter of that ground truth's image box; random alphas."""
    rng = np.random.default_rng(seed)
    out = []
    for g, d in pairs:
        b2 = d.box2d.copy()
        if len(g.names) and len(d.names):
            dist = np.hypot(d.location[:, None, 0] - g.location[None, :, 0], d.location[:, None, 2] - g.location[None, :, 2])
            near = dist.argmin(1)
            for j in np.nonzero(dist.min(1) < 2.0)[0]:
                x1, y1, x2, y2 = g.box2d[near[j]]
                w, h = x2 - x1, y2 - y1
                b2[j] = [x1 + rng.normal(0, 0.1 * w), y1 + rng.normal(0, 0.1 * h), x2 + rng.normal(0, 0.1 * w),
                         y2 + rng.normal(0, 0.1 * h)]
        out.append((g._replace(alpha=rng.uniform(-np.pi, np.pi, len(g.names))),
                    d._replace(box2d=b2, alpha=rng.uniform(-np.pi, np.pi, len(d.names)))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--gt", type=int, default=20)
    ap.add_argument("--dt", type=int, default=100)
    ap.add_argument("--host-frames", type=int, default=3769, help="frames given to the host restatement (timed separately)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--metrics", default="bev,3d", help="comma list of bbox, bev, 3d, aos (KittiEvaluator metrics)")
    ap.add_argument("--overlaps", default="strict,loose", help="comma list of strict, loose, coco (KittiEvaluator overlap sets)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mb_kitti_eval needs a GPU"
    t = time.perf_counter()
    metrics = tuple(m for m in args.metrics.split(",") if m)
    overlaps = tuple(o for o in args.overlaps.split(",") if o)
    pairs = make_set(args.frames, args.gt, args.dt)
    if "bbox" in metrics or "aos" in metrics:
        pairs = with_image_boxes(pairs)
    n_gt = sum(len(g.names) for g, _ in pairs)
    n_dt = sum(len(d.names) for _, d in pairs)
    print(f"set: {len(pairs)} frames, {n_gt} ground truths, {n_dt} detections (generated in {time.perf_counter() - t:.1f} s)")
    ev = KittiEvaluator(metrics=metrics, overlaps=overlaps)
    for g, d in pairs:
        ev.add_frame(g, d)
    for _ in range(2):
        res = ev.compute()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        ev.compute()  # ends in its one host read
        times.append(time.perf_counter() - t)
    print(f"device compute(): median {np.median(times) * 1e3:.2f} ms, min {min(times) * 1e3:.2f} ms over {args.reps} calls "
          f"(host packing + uploads + kernels + sort + one read; metrics {','.join(metrics)}; overlaps {','.join(overlaps)}; "
          f"{len(ev.combos)} combos)")
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        ev.compute()
        torch.cuda.synchronize()
    rows = [(e.key, e.device_time_total, e.count) for e in prof.key_averages() if e.device_time_total > 0]
    rows.sort(key=lambda r: -r[1])
    print("per-kernel device time of one compute() (us):" if rows else "per-kernel split: no device events recorded")
    for name, us, n in rows[:12]:
        print(f"  {us:10.1f}  x{n:<3d} {name[:100]}")
    hf = min(args.host_frames, len(pairs))
    if hf == 0:
        print(ev.summary())
        return
    t = time.perf_counter()
    frames = [R.make_frame(g, d) for g, d in pairs[:hf]]
    official = tuple(o for o in overlaps if o != "coco")
    want, _ = R.evaluate(frames, metrics=tuple(m for m in metrics if m in ("bev", "3d")), overlap_sets=official)
    host = time.perf_counter() - t
    print(f"host float64 restatement: {host:.1f} s for {hf} frames")
    if hf == len(pairs):
        diff = max((abs(a - b) for o in want for c in want[o] for m in want[o][c] for k in ("R11", "R40")
                    for a, b in zip(res[o][c][m][k], want[o][c][m][k])), default=0.0)
        print(f"largest |AP(device) - AP(host)|: {diff:.3g} (this set has no margin around the minimum overlaps)")
    print(ev.summary())


if __name__ == "__main__":
    main()
