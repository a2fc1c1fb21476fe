"""Time per call of per-object ground-truth noise (cfg.AUG.OBJECT_NOISE) on the synthetic KITTI frame (synth.make_cloud / make_gt_boxes:
16 384 points, 27 boxes, NUM_TRY = 100), B = 1 and B = 8 frames per call: the native path (v3d_object_noise: two launches for the
whole batch) against the torch statement of the same class (ObjectNoiseAugmentation.torch_statement, frame by frame) on the same device
in the same process, on the same injected draws.

    python tools/mb_object_noise.py [--out profiles/object_noise.txt] [--windows 7] [--reps 20]

Device-plus-host time: a host clock around `reps` calls that end in a device synchronise, inputs and draws resident on the device,
medians over repeated windows after a warm-up, the versions alternating window by window.  The kernels' own times come from a separate
profiled pass.  Results are compared before anything is timed.  The output is written to --out with the command line."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from vision3d_amd import synth  # noqa: E402
from vision3d_amd.core.config import second_car_cfg  # noqa: E402
from vision3d_amd.dataset import ObjectNoiseAugmentation  # noqa: E402

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
        tail = "" if m is med[0] else f"   ratio {m / med[0]:.1f}x"
        say(f"  {name}: {m * 1e6:9.1f} us per call ({min(t) * 1e6:.1f} .. {max(t) * 1e6:.1f}){tail}")


def kernel_times(fn, needles, calls=10):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    for ev in prof.key_averages():
        if any(s in ev.key for s in needles):
            total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            say(f"  kernel {ev.key.split('(')[0].split()[-1]}: {total / max(ev.count, 1):7.1f} us per launch, {ev.count // calls} per call")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "object_noise.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("python tools/mb_object_noise.py " + " ".join(sys.argv[1:] if argv is None else argv))
    cfg = second_car_cfg()
    noise = ObjectNoiseAugmentation(cfg, np.random.RandomState(0))
    frames = []
    for seed in range(8):
        points = torch.from_numpy(synth.make_cloud(seed)).cuda()
        boxes = torch.from_numpy(synth.make_gt_boxes(seed)).cuda()
        trans, rot = noise.draw(boxes.shape[0])
        frames.append((points, boxes, torch.from_numpy(trans).cuda(), torch.from_numpy(rot).cuda()))
    for B in (1, 8):
        batch = frames[:B]
        pts, bxs, draws = [f[0] for f in batch], [f[1] for f in batch], [(f[2], f[3]) for f in batch]

        def native():
            return noise.batch(pts, bxs, draws)

        def stated():
            return [noise.torch_statement(*f) for f in batch]

        got_p, got_b = native()
        chosen = noise.last_chosen.clone()
        want = stated()
        assert torch.equal(chosen, torch.cat([w[2] for w in want])), "native and torch statement choose different tries"
        assert all(torch.equal(a, w[1]) for a, w in zip(got_b, want)), "native and torch statement disagree on the boxes"
        assert all(torch.allclose(a, w[0], rtol=1e-6, atol=1e-5) for a, w in zip(got_p, want)), "native and torch statement disagree on the points"
        c = chosen.cpu().numpy()
        say(f"object noise: B = {B}, {sum(p.shape[0] for p in pts)} points, {len(c)} boxes, NUM_TRY = {noise.num_try}: "
            f"{int((c == 0).sum())} boxes take try 0, {int((c > 0).sum())} a later one (latest {int(c.max())}), {int((c < 0).sum())} stay")
        compare([("native (2 launches)              ", native), ("torch statement (a loop over boxes)", stated)], args.windows, args.reps)
        kernel_times(native, ("on_select_kernel", "on_points_kernel"))
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
