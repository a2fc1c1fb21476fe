"""Time per call of the centre heatmap head (cfg.CENTERHEAD) at KITTI size (200 x 176 cells, 3 classes, TOPK 100), B = 1 and B = 8: each
native call of csrc/center_head.hip against its torch statement on the same device in the same process, on the same inputs --
    targets   v3d_center_targets (1 launch)             vs CenterTargetAssigner.forward_torch   (synth.make_gt_boxes, 27 boxes per frame)
    loss      v3d_center_loss_fwd_bwd + _scale           vs CenterLoss.forward_torch + autograd  (forward and gradient of the maps)
    decode    v3d_center_decode (2 launches)             vs CenterHead.decode_torch

    python tools/mb_center_head.py [--out profiles/center_head.txt] [--windows 7] [--reps 20]

Device-plus-host time: a host clock around `reps` calls that end in a device synchronise, inputs resident on the device, medians
over repeated windows after a warm-up, the versions alternating window by window.  The kernels' own times come from a separate
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
from vision3d_amd.core.center_targets import CenterTargetAssigner  # noqa: E402
from vision3d_amd.core.config import _defaults  # noqa: E402
from vision3d_amd.detector.center_head import CenterHead, CenterLoss  # noqa: E402

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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "center_head.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("python tools/mb_center_head.py " + " ".join(sys.argv[1:] if argv is None else argv))
    cfg = _defaults()
    cfg.CENTERHEAD.ENABLED = True
    n_cls = cfg.NUM_CLASSES
    head, assigner, loss = CenterHead(cfg).cuda(), CenterTargetAssigner(cfg), CenterLoss(cfg)
    H, W = head.map_shape
    rng = np.random.default_rng(0)
    for B in (1, 8):
        boxes = [torch.from_numpy(synth.make_gt_boxes(seed)).cuda() for seed in range(B)]
        classes = [torch.from_numpy(rng.integers(0, n_cls, len(b)).astype(np.int32)).cuda() for b in boxes]
        logits = (rng.permutation(B * n_cls * H * W).astype(np.float32) / (B * n_cls * H * W) * 8 - 4).reshape(B, n_cls, H, W)
        maps = torch.from_numpy(np.concatenate((logits, rng.normal(0, 0.5, (B, 8, H, W)).astype(np.float32)), 1)).cuda()
        say(f"centre head: B = {B}, {n_cls} classes, {H} x {W} cells, TOPK = {head.TOPK}, {sum(len(b) for b in boxes)} boxes")

        # ---- targets
        native_t = lambda: assigner.forward_native(boxes, classes)
        torch_t = lambda: assigner.forward_torch(boxes, classes)
        got, want = native_t(), torch_t()
        assert all(torch.equal(a, b) for a, b in zip(got[1:4], want[1:4])), "native and torch targets disagree on ind / mask / cls"
        e_heat, e_reg = float((got[0] - want[0]).abs().max()), float((got[4] - want[4]).abs().max())
        say(f"  targets: native against the torch statement: heat {e_heat:.2e}, reg {e_reg:.2e} (absolute)")
        # (the cell offsets carry two fp32 roundings at magnitude < 256, and torch divides by a scalar through its reciprocal: 4e-5)
        assert e_heat <= 1e-6 and e_reg <= 4e-5, "native and torch targets disagree"
        compare([("targets native (1 launch)     ", native_t), ("targets torch statement       ", torch_t)], args.windows, args.reps)
        kernel_times(native_t, ("ch_targets_kernel",))
        heat, ind, mask, _, reg = got

        # ---- loss, forward and gradient
        def run_loss(fused):
            m = maps.detach().requires_grad_()
            p_cls, p_reg = m[:, :n_cls], m[:, n_cls:]
            item = dict(P_cls=p_cls, P_reg=p_reg, G_heat=heat, G_ind=ind, G_mask=mask, G_creg=reg)
            if fused:
                item["_head_maps"] = (m, p_cls, p_reg)
            out = loss(item)
            out["loss"].backward()
            return out["loss"].detach(), m.grad

        (l1, g1), (l2, g2) = run_loss(True), run_loss(False)
        assert torch.allclose(l1, l2, rtol=1e-4) and float((g1 - g2).abs().max()) <= 1e-4 * float(g2.abs().max()), "native and torch loss disagree"
        compare([("loss native (3 + 1 launches)  ", lambda: run_loss(True)), ("loss torch + autograd         ", lambda: run_loss(False))],
                args.windows, args.reps)
        kernel_times(lambda: run_loss(True), ("ch_loss_", "loss_scale_kernel"))

        # ---- decode
        native_d, torch_d = lambda: head.decode(maps), lambda: head.decode_torch(maps)
        (b1, s1), (b2, s2) = native_d(), torch_d()
        assert torch.allclose(s1, s2, rtol=0, atol=1e-6) and torch.allclose(b1, b2, rtol=1e-5, atol=1e-4), "native and torch decode disagree"
        compare([("decode native (2 launches)    ", native_d), ("decode torch statement        ", torch_d)], args.windows, args.reps)
        kernel_times(native_d, ("ch_peaks_kernel", "ch_select_kernel"))
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
