"""Dynamic voxelization (cfg.DYNAMIC_VOXELIZATION, csrc/voxelize.hip "DYNAMIC") beside the hard voxelizer, on one device in one process
on the same clouds (vision3d_amd.synth) --
    KITTI   16k points per frame, 0.05 x 0.05 x 0.1 m voxels, hard form at MAX_OCCUPANCY 5
    Waymo   180k points per frame, the Waymo-range grid, hard form at 5
    pillar  16k points per frame, 0.4 x 0.4 x 4 m pillars (PILLAR_KITTI), hard form at 32 slots (its wide path)
each at B = 1 and B = 8: per call the device time between two events around `reps` back-to-back calls (median over windows, the
versions alternating window by window; a call includes its output allocations, the same for every version), the kernels' summed
time and the launches per call from a profiled pass of its own, the summation variants of the dynamic form (64-bit integer atomics
per point / a voxel's first point walks its voxel's list / hybrid: the walk up to 32 points, the atomics above), and the share of
in-range points the hard form drops at MAX_OCCUPANCY 5 and 32.  Results are compared before anything is timed: same cells as the hard form, every variant the same bits.

    python tools/mb_dynamic_voxelize.py [--out profiles/dynamic_voxelize.txt] [--windows 9] [--reps 50] [--append FILE ...]

--append: text files added verbatim at the end (the bench.py lines recorded in the same session)."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vision3d_amd import _lib as L  # noqa: E402
from vision3d_amd import synth  # noqa: E402
from vision3d_amd.core.config import pillar_car_cfg, second_car_cfg, waymo_range_cfg  # noqa: E402
from vision3d_amd.spconv.utils import voxelize_batch, voxelize_dynamic_batch  # noqa: E402

LINES = []
VARIANTS = ((0, "atomic"), (1, "walk"), (2, "hybrid"))


def say(text):
    print(text, flush=True)
    LINES.append(text)


def window(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) * 1e-3 / reps


def compare(named, windows, reps):
    """named: [(name, fn)] timed in alternating windows; ratios against the first."""
    for _, fn in named:
        fn(), fn(), fn()
    times = [[] for _ in named]
    for _ in range(windows):
        for t, (_, fn) in zip(times, named):
            t.append(window(fn, reps))
    med = [statistics.median(t) for t in times]
    for (name, _), t, m in zip(named, times, med):
        tail = "" if m is med[0] else f"   ratio {m / med[0]:.2f}x"
        say(f"    {name}: {m * 1e6:9.1f} us per call ({min(t) * 1e6:.1f} .. {max(t) * 1e6:.1f}){tail}")
    return med


def kernel_times(name, fn, calls=10):
    from torch.profiler import ProfilerActivity, profile
    fn()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    launches, busy, parts = 0, 0.0, []
    for ev in prof.key_averages():
        total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
        if total <= 0:
            continue
        launches += ev.count
        busy += total
        short = (ev.key.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").strip() or ev.key)[:40]
        parts.append(f"{short} {total / calls:.1f}")
    say(f"    {name}: {launches / calls:g} launches (kernels and copies) per call, {busy / calls:.1f} us of kernel time per call")
    say("      us per call by kernel: " + "; ".join(parts))


def with_variant(v, fn):
    def run():
        prev = L.lib().v3d_voxelize_dynamic_variant(v)
        try:
            return fn()
        finally:
            L.lib().v3d_voxelize_dynamic_variant(prev)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dynamic_voxelize.txt"))
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--append", nargs="*", default=[])
    a = ap.parse_args()
    torch.cuda.set_device(0)
    say("$ python tools/mb_dynamic_voxelize.py " + " ".join(sys.argv[1:]))
    say(f"device: {torch.cuda.get_device_name(0)}")
    say(f"default summation variant of this build: {dict(VARIANTS)[L.lib().v3d_voxelize_dynamic_variant(-1)]}")
    kitti, waymo, pillar = second_car_cfg(), waymo_range_cfg(), pillar_car_cfg()
    cases = (("KITTI 16k, 0.05 m voxels", kitti, lambda s: synth.make_cloud(s, n_points=16384), 5),
             ("Waymo-range 180k", waymo, lambda s: synth.make_waymo_cloud(s), 5),
             ("pillar grid 16k, 0.4 m pillars", pillar, lambda s: synth.make_cloud(s, n_points=16384), 32))
    for title, cfg, cloud_of, max_pts in cases:
        for B in (1, 8):
            clouds = [torch.from_numpy(cloud_of(s)).cuda() for s in range(B)]
            offsets = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).tolist()
            flat = torch.cat(clouds) if B > 1 else clouds[0]
            vs, bounds, mv = cfg.VOXEL_SIZE, cfg.GRID_BOUNDS, cfg.MAX_VOXELS

            def hard(want_voxels=True):
                return voxelize_batch(flat, offsets, vs, bounds, max_pts, mv, want_voxels)

            def dynamic():
                return voxelize_dynamic_batch(flat, offsets, vs, bounds, mv)
            outs = [with_variant(v, dynamic)() for v, _ in VARIANTS]
            m, status = outs[0][4].tolist()
            for other in outs[1:]:
                for k in range(5):
                    assert torch.equal(outs[0][k][:m] if k < 3 else outs[0][k], other[k][:m] if k < 3 else other[k]), "the variants differ"
            _, h_coords, h_occ, _, h_n = hard()
            occ = outs[0][1][:m]
            assert int(h_n.item()) == m and torch.equal(h_coords[:m], outs[0][0][:m]) and torch.equal(h_occ[:m], occ.clamp(max=max_pts))
            kept = int(occ.sum())
            say(f"{title}, B = {B}: {offsets[-1]} points, {kept} in range, {m} voxels, largest voxel {int(occ.max())} points, status {status}")
            say("  share of in-range points the hard form drops: "
                + ", ".join(f"{100.0 * int((occ - cap).clamp(min=0).sum()) / max(kept, 1):.2f} % at MAX_OCCUPANCY {cap}" for cap in (5, 32)))
            named = [(f"hard, {max_pts} slots, with the slot tensor", hard)]
            if max_pts <= 8:
                named.append((f"hard, {max_pts} slots, mean only (the plan)", lambda: hard(False)))
            named += [(f"dynamic, {name:6s}                      ", with_variant(v, dynamic)) for v, name in VARIANTS]
            say("  device time (events around back-to-back calls):")
            compare(named, a.windows, a.reps)
            say("  profiled pass:")
            for name, fn in named:
                kernel_times(name.strip(), fn)
    for path in a.append:
        with open(path) as f:
            for line in f.read().splitlines():
                say(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
