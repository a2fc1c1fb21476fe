"""Time per call of PV-RCNN's Predicted Keypoint Weighting (cfg.PKW) at 2 048 and 16 x 2 048 keypoint rows of 512 channels: the native
weighting (one v3d_linear_rows launch for the hidden layer + one launch of csrc/keypoint_weight.hip, in place on the point-major
matrix) and the fused segmentation loss with its backward, each against the torch statements kept beside it
(KeypointWeighting.forward_torch, KeypointSegLoss.forward_torch) on the same device in the same process.

    python tools/mb_keypoint_weighting.py [--out profiles/keypoint_weighting.txt] [--windows 7] [--reps 50]

Device-plus-host time: a host clock around `reps` calls that end in a device synchronise, inputs resident on the device, medians over
repeated windows after a warm-up of every shape, the two versions alternating window by window.  The kernels' own times come from a
separate profiled pass.  Results are compared before anything is timed.  The output is written to --out with the command line."""
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
from vision3d_amd.core.config import _defaults  # noqa: E402
from vision3d_amd.detector import KeypointSegLoss, KeypointWeighting  # noqa: E402

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


def compare(name_a, fn_a, name_b, fn_b, windows, reps):
    for fn in (fn_a, fn_b):  # warm-up of every shape
        fn(), fn(), fn()
    ta, tb = [], []
    for _ in range(windows):  # alternating: both see the same drift of the host
        ta.append(window(fn_a, reps))
        tb.append(window(fn_b, reps))
    ma, mb = statistics.median(ta), statistics.median(tb)
    say(f"  {name_a}: {ma * 1e6:8.1f} us per call ({min(ta) * 1e6:.1f} .. {max(ta) * 1e6:.1f})")
    say(f"  {name_b}: {mb * 1e6:8.1f} us per call ({min(tb) * 1e6:.1f} .. {max(tb) * 1e6:.1f})   ratio {mb / ma:.1f}x")


def kernel_times(fn, needles, calls=20):
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "keypoint_weighting.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("python tools/mb_keypoint_weighting.py " + " ".join(sys.argv[1:] if argv is None else argv))
    cfg = _defaults()
    cfg.PKW.ENABLED = True
    k, c = cfg.NUM_KEYPOINTS, 512
    torch.manual_seed(0)
    head = KeypointWeighting(cfg, c).cuda().eval()
    loss = KeypointSegLoss(cfg)
    for batch in (1, 16):
        gen = torch.Generator(device="cuda").manual_seed(batch)
        feats = torch.randn(batch, k, c, device="cuda", generator=gen).relu_()
        with torch.no_grad():
            pm = feats.clone()
            logits = head.weight_point_major(pm)
            stated_w, stated_l = head.forward_torch(feats.transpose(1, 2))
        assert torch.allclose(logits, stated_l, rtol=1e-4, atol=1e-6) and torch.allclose(pm, stated_w.transpose(1, 2), rtol=1e-4, atol=1e-6), \
            "the two weightings disagree"
        say(f"{batch * k} rows x {c} channels (B = {batch}, K = {k}), hidden width {cfg.PKW.MLPS[0]}")
        work = feats.clone()  # (scaled again and again in place: the values shrink, the time does not depend on them)

        def native():
            with torch.no_grad():
                return head.weight_point_major(work)

        def stated():
            with torch.no_grad():
                return head.forward_torch(feats.transpose(1, 2))

        compare("weighting, native (2 launches) ", native, "weighting, forward_torch       ", stated, args.windows, args.reps)
        kernel_times(native, ("keypoint_weight_kernel", "linear_rows_kernel"))

        # loss: keypoints from synthetic clouds, the ground truth of synth.make_gt_boxes (as the train-step tests)
        rng = np.random.default_rng(batch)
        clouds = [synth.make_cloud(s) for s in range(batch)]
        kp = torch.from_numpy(np.stack([cl[rng.choice(len(cl), k, replace=False), :3] for cl in clouds])).cuda()
        boxes = [torch.from_numpy(synth.make_gt_boxes(s)).cuda() for s in range(batch)]
        cls = [torch.zeros(len(b), dtype=torch.long, device="cuda") for b in boxes]
        x0 = torch.randn(batch, k, device="cuda", generator=gen)

        def run(fn):
            x = x0.clone().requires_grad_(True)
            item = dict(K_cls=x, keypoints=kp, boxes=boxes, class_idx=cls)
            out = fn(item)
            out["loss"].backward()
            return out["loss"].detach(), x.grad, item["K_label"]

        (la, ga, ba), (lb, gb, bb) = run(loss), run(loss.forward_torch)
        assert torch.equal(ba, bb) and torch.allclose(la, lb, rtol=1e-5) and torch.allclose(ga, gb, rtol=1e-4, atol=1e-8), "the two losses disagree"
        say(f"  labels 0 / 1 / 255: {int((ba == 0).sum())} / {int((ba == 1).sum())} / {int((ba == 255).sum())}; "
            f"{sum(len(b) for b in boxes)} ground truths in {batch} frame(s)")
        compare("loss + backward, fused         ", lambda: run(loss), "loss + backward, torch         ", lambda: run(loss.forward_torch),
                args.windows, args.reps)
        kernel_times(lambda: run(loss), ("keypoint_seg_loss", "loss_scale_kernel"))
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
