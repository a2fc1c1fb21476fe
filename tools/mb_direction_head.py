"""Time per call of the direction classifier + sine yaw loss of the anchor head (cfg.DIRECTION) on the 200 x 176 map of the car
config, on one device in one process, on the same inputs --
    loss       v3d_proposal_dir_loss_fwd_bwd + _scale   vs the torch expressions of ProposalLoss + autograd   (B = 1 and 8)
    proposals  v3d_proposals_dir_flag ([cls | reg | dir]) vs v3d_proposals_flag ([cls | reg]) on the same class / box channels (B = 1)
and the fp32 errors of the loss against float64 over the cases of tests/direction_cases.py: the fused kernel's and the fp32 torch
statement's, which set the bounds of tests/test_gpu_direction.py.

    python tools/mb_direction_head.py [--out profiles/direction_head.txt] [--windows 7] [--reps 20]

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
sys.path.insert(0, os.path.join(REPO, "tests"))
from vision3d_amd.core import AnchorGenerator  # noqa: E402
from vision3d_amd.core.config import second_car_cfg  # noqa: E402
from vision3d_amd.detector.proposal import ProposalLayer, ProposalLoss  # noqa: E402

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


def measured_errors():
    """The figures of tests/test_gpu_direction.py::test_loss_and_gradient_against_the_float64_statement, largest over its cases."""
    import direction_cases as DC
    import test_gpu_direction as T
    worst = {}
    for case in DC.LOSS_CASES:
        c = DC.loss_case(*case)
        ref, gref = T._statement(c, torch.float64)
        own, gown = T._statement(c, torch.float32)
        got, ggot = T._fused(c)
        got, ggot = {k: float(v.detach()) for k, v in got.items()}, ggot.double()
        gmax = max(float(gref.abs().max()), 1e-30)
        ch = T._channel_groups(c)
        rel = lambda a, k: abs(a[k] - ref[k]) / max(1.0, abs(ref[k]))
        gerr = lambda g, idx: float((g[:, idx] - gref[:, idx]).abs().max()) / gmax
        fig = dict(cls_loss=(0.0, rel(got, "cls_loss")), dir_loss=(rel(own, "dir_loss"), rel(got, "dir_loss")),
                   cls_gradient=(0.0, gerr(ggot, ch["cls"])), box6_gradient=(gerr(gown, ch["box6"]), gerr(ggot, ch["box6"])),
                   dir_gradient=(gerr(gown, ch["dir"]), gerr(ggot, ch["dir"])))
        sine = "sin" if c["sin_yaw"] else "plain"
        fig[f"reg_loss ({sine} yaw)"] = (rel(own, "reg_loss"), rel(got, "reg_loss"))
        fig[f"yaw_gradient ({sine} yaw)"] = (gerr(gown, ch["yaw"]), gerr(ggot, ch["yaw"]))
        for k, v in fig.items():
            worst[k] = tuple(max(a, b) for a, b in zip(worst.get(k, (0.0, 0.0)), v))
    say("fp32 errors against float64, largest over tests/direction_cases.py LOSS_CASES (loss terms: relative to max(1, |term|); gradients: "
        "relative to the largest gradient of the map, upstream gradients 2, 3, 5):")
    for k in sorted(worst):
        say(f"  {k:28s} fp32 torch statement {worst[k][0]:.2e}   fused kernel {worst[k][1]:.2e}")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "direction_head.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("python tools/mb_direction_head.py " + " ".join(sys.argv[1:] if argv is None else argv))
    measured_errors()
    cfg, plain_cfg = second_car_cfg(), second_car_cfg()
    cfg.DIRECTION.ENABLED = True
    head, plain, loss = ProposalLayer(cfg), ProposalLayer(plain_cfg), ProposalLoss(cfg)
    anchors = AnchorGenerator(cfg).anchors.cuda()
    n_cls, n_yaw, H, W = anchors.shape[:4]
    na = n_cls * n_yaw
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in (1, 8):
        shape = (B, n_cls, n_yaw, H, W)
        maps = torch.randn(B, na * 9, H, W, device="cuda", generator=g) * 1.5
        G_cls = (torch.rand(shape, device="cuda", generator=g) > 0.99).to(torch.int8)
        M_cls = torch.rand(shape, device="cuda", generator=g) > 0.1
        G_reg = torch.randn(shape + (7,), device="cuda", generator=g)
        M_reg = (G_cls == 1).unsqueeze(-1)
        G_dir = ((torch.rand(shape, device="cuda", generator=g) > 0.5) & M_reg[..., 0]).to(torch.int8)
        tg = dict(G_cls=G_cls, M_cls=M_cls, G_reg=G_reg, M_reg=M_reg, G_dir=G_dir)
        say(f"direction head: B = {B}, {n_cls} class(es) x {n_yaw} yaws, {H} x {W} cells, {int(M_reg.sum())} positives")

        def run_loss(fused):
            m = maps.detach().requires_grad_()
            p_cls, p_reg = head.maps_from_fused(m)
            p_dir = head.dir_from_fused(m)
            item = dict(tg, P_cls=p_cls, P_reg=p_reg, P_dir=p_dir)
            if fused:
                item["_head_maps"] = (m, p_cls, p_reg, p_dir)
            out = loss(item)
            out["loss"].backward()
            return out["loss"].detach(), m.grad

        (l1, g1), (l2, g2) = run_loss(True), run_loss(False)
        assert torch.allclose(l1, l2, rtol=1e-5) and float((g1 - g2).abs().max()) <= 1e-5 * float(g2.abs().max()), "native and torch loss disagree"
        compare([("loss native (4 + 3-4 launches)   ", lambda: run_loss(True)), ("loss torch + autograd            ", lambda: run_loss(False))],
                args.windows, args.reps)
        kernel_times(lambda: run_loss(True), ("pl_", "loss_scale_kernel"))
    # ---- proposal stage, B = 1: the same class / box channels with and without the direction channels
    maps = torch.randn(1, na * 9, H, W, device="cuda", generator=g)
    maps8 = maps[:, :na * 8].contiguous()
    with_dir, without = lambda: head.native_proposals(maps, anchors), lambda: plain.native_proposals(maps8, anchors)
    a, b = head.finalize_native(*with_dir()), plain.finalize_native(*without())
    assert torch.equal(a[0][:, :6], b[0][:, :6]) and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])), "the two stages keep different boxes"
    say(f"proposal stage: B = 1, TOPK = {head.TOPK}, {len(a[0])} proposals kept by both")
    compare([("proposals without direction     ", without), ("proposals with direction        ", with_dir)], args.windows, args.reps)
    kernel_times(with_dir, ("prop_",))
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
