"""Time per call of PV-RCNN's stage-2 target assignment and loss at B = 8 frames, n = 100 and n = 300 RoIs per frame (1 and 3
classes x TOPK 100, 8 ground truths per class and frame: synth.make_refine_case): the fused paths (csrc/refine_targets.hip) against
the op-by-op torch statements kept beside them.

    python tools/mb_refine_targets.py [--batch 8] [--windows 7] [--reps 50]

Device-plus-host time: a host clock around `reps` calls that end in a device synchronise, inputs resident on the device, medians over
repeated windows after a warm-up of every shape, the two versions alternating window by window.  The kernels' own times come from a
separate profiled pass.  Results are compared before anything is timed."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vision3d_amd import synth  # noqa: E402
from vision3d_amd.core import RefinementTargetAssigner  # noqa: E402
from vision3d_amd.core.config import _defaults  # noqa: E402
from vision3d_amd.detector import RefinementLoss  # noqa: E402

KEYS = ("R_iou", "R_match", "G_conf", "G_rreg", "M_rcls", "M_rreg")


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
    print(f"  {name_a}: {ma * 1e6:8.1f} us per call ({min(ta) * 1e6:.1f} .. {max(ta) * 1e6:.1f})")
    print(f"  {name_b}: {mb * 1e6:8.1f} us per call ({min(tb) * 1e6:.1f} .. {max(tb) * 1e6:.1f})   ratio {mb / ma:.1f}x")


def kernel_times(fn, needles, calls=20):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    for ev in prof.key_averages():
        if any(s in ev.key for s in needles):
            total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            print(f"  kernel {ev.key.split('(')[0].split()[-1]}: {total / max(ev.count, 1):7.1f} us per launch, {ev.count // calls} per call")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    cfg = _defaults()
    assigner, loss = RefinementTargetAssigner(cfg), RefinementLoss(cfg)
    for n_cls in (1, 3):
        p, pc, boxes, cls, draws = synth.make_refine_case(0, n_cls=n_cls, batch=args.batch)
        item = dict(proposals=torch.from_numpy(p).cuda(), proposal_class=torch.from_numpy(pc).cuda(),
                    boxes=[torch.from_numpy(b).cuda() for b in boxes], class_idx=[torch.from_numpy(c).cuda() for c in cls],
                    refine_draws=torch.from_numpy(draws).cuda())
        fused, stated = assigner(dict(item)), assigner.forward_torch(dict(item))
        assert all(torch.equal(fused[k], stated[k]) for k in ("R_iou", "R_match", "M_rcls", "M_rreg")), "the two assignments disagree"
        assert torch.allclose(fused["G_conf"], stated["G_conf"], rtol=0, atol=2e-7) and torch.allclose(fused["G_rreg"], stated["G_rreg"], rtol=1e-5, atol=1e-6)
        print(f"B = {args.batch}, n = {p.shape[1]} RoIs ({n_cls} class(es)), {len(boxes[0])} ground truths per frame; "
              f"{int(fused['M_rcls'].sum())} sampled, {int(fused['M_rreg'].sum())} with a box target")
        compare("targets, fused (1 launch)     ", lambda: assigner(dict(item)), "targets, forward_torch        ",
                lambda: assigner.forward_torch(dict(item)), args.windows, args.reps)
        kernel_times(lambda: assigner(dict(item)), ("refine_targets_kernel",))

        head = torch.randn(args.batch, p.shape[1], 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))

        def run(fn):
            x = head.clone().requires_grad_(True)
            r_reg, r_cls = x.split([7, 1], dim=-1)
            out = fn(dict(fused, R_reg=r_reg, R_cls=r_cls))
            out["loss"].backward()
            return out["loss"].detach(), x.grad

        (la, ga), (lb, gb) = run(loss), run(loss.forward_torch)
        assert torch.allclose(la, lb, rtol=1e-6) and torch.allclose(ga, gb, rtol=1e-5, atol=1e-7), "the two losses disagree"
        compare("loss + backward, fused        ", lambda: run(loss), "loss + backward, torch        ", lambda: run(loss.forward_torch),
                args.windows, args.reps)
        kernel_times(lambda: run(loss), ("refine_loss", "loss_scale_kernel"))
    return 0


if __name__ == "__main__":
    sys.exit(main())
