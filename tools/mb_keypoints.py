"""Keypoint sampling: plain FPS against sector_point_sample ("sector": S chains, no proposals; "spc": among the points near the frame's
own stage-1 proposals), time per call by HIP events.

  KITTI-shaped cloud, 16 384 points -> 2 048 keypoints, S = 6: one cloud and a batch of 16
  Waymo-range sweep, 180 000 points -> 4 096 keypoints, S = 6: sector_point_sample only (plain FPS stops at 65 536 points)

    python tools/mb_keypoints.py [--out profiles/keypoint_sampling.txt] [--iters 20]

    python tools/mb_keypoints.py --launches [--out ...]      # second step, a run of its own: APPENDS the launches of a call one by one

--launches starts `rocprofv3 --kernel-trace --stats -- python tools/mb_keypoints.py --workload W --iters 5` once per workload (fresh
child processes; tracing slows the host, so the per-call times above come from the first step) and appends the average time of
kp_count / kp_scan / kp_emit (select + compact), kp_sector_fps, kp_pad and the plain FPS kernel from the kernel statistics."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision3d_amd import synth  # noqa: E402
from vision3d_amd.pointnet2.pointnet2_utils import furthest_point_sample, sector_point_sample  # noqa: E402


def time_call(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def stage1_proposals(clouds):
    """The (len(clouds), 100, 7) stage-1 proposals of a seeded, untrained car-only PV-RCNN, frame by frame."""
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    from vision3d_amd.core.config import second_car_cfg
    from vision3d_amd.detector import PV_RCNN
    cfg = second_car_cfg()
    torch.manual_seed(0)
    model = PV_RCNN(cfg).cuda().eval()
    anchors = AnchorGenerator(cfg).anchors.cuda()
    boxes = []
    with torch.no_grad():
        for cloud in clouds:
            item = Preprocessor(cfg, seed=0)(dict(points=[cloud], anchors=anchors))
            item["keypoints"] = item["points"][:, :cfg.NUM_KEYPOINTS, :3].contiguous()  # (stage 1 does not read them)
            boxes.append(model.stage1_proposals(model.proposal(item))[0])
    return torch.cat(boxes).contiguous()


WORKLOADS = ("kitti x1", "kitti x16", "waymo x1")


def measure(workload, iters):
    """-> the lines of one workload."""
    lines = []
    if workload.startswith("kitti"):
        n_frames = int(workload.split("x")[1])
        clouds = [synth.make_cloud(s) for s in range(n_frames)]
        pts = torch.from_numpy(np.stack(clouds)).cuda()
        xyz = pts[..., :3].contiguous()
        boxes = stage1_proposals(clouds)
        fps = furthest_point_sample(xyz, 2048)
        same = torch.equal(sector_point_sample(pts, 2048, 1), fps)
        _, c_sec = sector_point_sample(pts, 2048, 6, return_counts=True)
        _, c_spc = sector_point_sample(pts, 2048, 6, boxes, 1.6, return_counts=True)
        lines.append(f"{workload}: 16384 -> 2048; S = 1 equals plain FPS: {same}; candidates per frame: sector {c_sec.sum(1).float().mean():.0f}, "
                     f"spc {c_spc.sum(1).float().mean():.0f} (largest sector {int(c_sec.max())} / {int(c_spc.max())})")
        lines.append(f"  plain FPS (furthest_point_sample)      {time_call(lambda: furthest_point_sample(xyz, 2048), iters):9.1f}")
        lines.append(f"  sector, S = 6                          {time_call(lambda: sector_point_sample(pts, 2048, 6), iters):9.1f}")
        lines.append(f"  spc, S = 6, 100 proposals, r = 1.6     {time_call(lambda: sector_point_sample(pts, 2048, 6, boxes, 1.6), iters):9.1f}")
    else:
        pts = torch.from_numpy(synth.make_waymo_cloud(0)[None]).cuda()
        _, c_sec = sector_point_sample(pts, 4096, 6, return_counts=True)
        lines.append(f"{workload}: 180000 -> 4096 (plain FPS: unsupported above 65 536 points); largest sector {int(c_sec.max())} "
                     "(above 24 576: its chain streams its running distances)")
        lines.append(f"  sector, S = 6                          {time_call(lambda: sector_point_sample(pts, 4096, 6), max(3, iters // 4)):9.1f}")
    return lines


def launches(workload):
    """The kernels of `workload` under rocprofv3 in a fresh child: -> lines "kernel  calls  average us"."""
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "kp", "--", sys.executable, os.path.abspath(__file__),
                        "--workload", workload, "--iters", "5", "--out", os.path.join(tmp, "ignored.txt")], check=True, timeout=280,
                       stdout=subprocess.DEVNULL)
        found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not found:
            raise SystemExit("mb_keypoints: rocprofv3 left no kernel statistics")
        rows = list(csv.DictReader(open(found[0])))
    lines = [f"{workload}: launches under rocprofv3 --kernel-trace (average us per launch, every call of the run; the chain kernel's "
             "average mixes the sector / spc / S = 1 calls)"]
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        if "kp_" in name or "fps_" in name:
            avg = float(r.get("AverageNs") or r.get("Average") or "nan") / 1e3
            lines.append(f"  {name.split('(')[0][:60]:60s} {r.get('Calls', '?'):>6s} {avg:10.1f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "keypoint_sampling.txt"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--workload", choices=WORKLOADS, default=None, help="one workload only (default: all)")
    ap.add_argument("--launches", action="store_true", help="append the per-launch times (rocprofv3 children) to --out")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.launches:
        for wl in WORKLOADS:
            text = "\n".join(launches(wl)) + "\n"
            print(text, end="", flush=True)
            with open(args.out, "a") as f:
                f.write(text)
        return
    if not torch.cuda.is_available():
        raise SystemExit("mb_keypoints: needs a GPU")
    lines = [f"keypoint sampling, us per call (HIP events, {args.iters} calls after 3 warm-up calls); {torch.cuda.get_device_name(0)}"]
    for wl in ([args.workload] if args.workload else WORKLOADS):
        lines += measure(wl, args.iters)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
