"""The rotated 3-D IoU loss (csrc/iou_loss.hip, ops/iou_loss.py) measured: writes profiles/iou_loss.txt.

    python tools/mb_iou_loss.py [--out profiles/iou_loss.txt] [--windows 7] [--reps 50]

1. Tolerances (CPU, no GPU needed): the fp32 pair function compiled for the host (tests/host/iou_loss_host_shim.cpp) against the
   float64 restatement (tests/iou_loss_ref.py) over the committed cases (tests/iou_loss_cases.py): worst absolute IoU and term
   error over all pairs, worst gradient error relative to the pair's largest gradient over the smooth named pairs and the random
   pairs whose margin exceeds the cases' bar.  The GPU tests use four times these figures.
2. Time per call (GPU): the native stage-2 term, forward + backward, against the torch statement on the same device at B = 1 and
   B = 8 frames of 300 RoIs (3 classes x TOPK 100: synth.make_refine_case), and the aligned operator at N = 300 and N = 65 536,
   with the number of kernel launches of both sides.  Device-plus-host time as tools/mb_refine_targets.py takes it: a host clock
   around `reps` calls that end in a device synchronise, inputs resident, medians over repeated windows after a warm-up, the two
   versions alternating window by window.  Results are compared before anything is timed.  No target ratio is set."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import iou_loss_cases as cases  # noqa: E402
import iou_loss_ref as ref  # noqa: E402

LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def host_build():
    so = os.path.join(REPO, "tests", "host", "_build", "libiou_loss_host.so")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c++17", "-o", so,
                           os.path.join(REPO, "tests", "host", "iou_loss_host_shim.cpp")])
    lib = C.CDLL(so)

    def run(a, b, kind):
        n = len(a)
        term, iou, da, db = np.empty(n, np.float32), np.empty(n, np.float32), np.empty((n, 7), np.float32), np.empty((n, 7), np.float32)
        lib.host_iou3d_loss(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), n, kind, *(x.ctypes.data_as(C.c_void_p) for x in (term, iou, da, db)))
        return term, iou, da, db
    return run


def tolerances():
    run = host_build()
    _, na, nb, kink = cases.named_pairs()
    ra, rb = cases.random_pairs(cases.N_RANDOM)
    keep = ref.margin(torch.tensor(ra), torch.tensor(rb)).numpy() > cases.MARGIN
    a, b = np.ascontiguousarray(np.concatenate((na, ra))), np.ascontiguousarray(np.concatenate((nb, rb)))
    smooth = np.concatenate((~kink, keep))
    say(f"tolerances: fp32 host build against the float64 restatement, {len(na)} named + {len(ra)} random pairs "
        f"({1 - keep.mean():.1%} of the random pairs left out of the gradient figure by margin <= {cases.MARGIN})")
    worst = dict(iou=0.0, term=0.0, grad=0.0)
    for kind, code in (("iou", 0), ("diou", 1)):
        term, iou, da, db = run(a, b, code)
        ta, tb = torch.tensor(a, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True)
        w_term, w_iou = ref.iou3d_terms(ta, tb, kind)
        w_da, w_db = (g.numpy() for g in torch.autograd.grad(w_term.sum(), (ta, tb)))
        e_iou, e_term = np.abs(iou - w_iou.detach().numpy()).max(), np.abs(term - w_term.detach().numpy()).max()
        scale = np.maximum(np.abs(w_da).max(1), np.abs(w_db).max(1))
        err = np.maximum(np.abs(da - w_da).max(1), np.abs(db - w_db).max(1))[smooth] / np.maximum(scale[smooth], 1e-30)
        say(f"  {kind:4s}: worst |IoU error| {e_iou:.3e}   |term error| {e_term:.3e}   gradient error / largest gradient of the pair {err.max():.3e}")
        worst = dict(iou=max(worst["iou"], e_iou), term=max(worst["term"], e_term), grad=max(worst["grad"], err.max()))
    say(f"  measured: IoU {worst['iou']:.2e}, term {worst['term']:.2e}, gradient {worst['grad']:.2e}")
    say(f"  bars of tests/test_gpu_iou_loss.py (4 x measured): IoU {4 * worst['iou']:.2e}, term {4 * worst['term']:.2e}, gradient {4 * worst['grad']:.2e}")


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def launches(fn, calls=5):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    return sum(ev.count for ev in prof.key_averages()) // calls


def compare(name_a, fn_a, name_b, fn_b, windows, reps):
    for fn in (fn_a, fn_b):  # warm-up of every shape
        fn(), fn(), fn()
    ta, tb = [], []
    for _ in range(windows):  # alternating: both see the same drift of the host
        ta.append(window(fn_a, reps))
        tb.append(window(fn_b, max(reps // 5, 1)))
    ma, mb = statistics.median(ta), statistics.median(tb)
    say(f"  {name_a}: {ma * 1e6:9.1f} us per call ({min(ta) * 1e6:.1f} .. {max(ta) * 1e6:.1f}), {launches(fn_a)} launches")
    say(f"  {name_b}: {mb * 1e6:9.1f} us per call ({min(tb) * 1e6:.1f} .. {max(tb) * 1e6:.1f}), {launches(fn_b)} launches   ratio {mb / ma:.1f}x")


def timings(args):
    from vision3d_amd import synth
    from vision3d_amd.core import RefinementTargetAssigner
    from vision3d_amd.core.config import _defaults
    from vision3d_amd.detector import RefinementLoss
    from vision3d_amd.ops import iou3d_loss, iou3d_loss_torch
    say(f"time per call on {torch.cuda.get_device_name(0)} (device + host, medians of {args.windows} windows)")
    for kind in ("iou", "diou"):
        cfg = _defaults()
        cfg.TRAIN.REFINEMENT_IOU_LOSS.merge_from_dict(dict(ENABLED=True, KIND=kind))
        assigner, loss = RefinementTargetAssigner(cfg), RefinementLoss(cfg)
        for batch in (1, 8):
            p, pc, boxes, cls, draws = synth.make_refine_case(0, n_cls=3, batch=batch)
            item = dict(proposals=torch.from_numpy(p).cuda(), proposal_class=torch.from_numpy(pc).cuda(),
                        boxes=[torch.from_numpy(b).cuda() for b in boxes], class_idx=[torch.from_numpy(c).cuda() for c in cls],
                        refine_draws=torch.from_numpy(draws).cuda())
            item = assigner(item)
            head = 0.1 * torch.randn(batch, p.shape[1], 8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))

            def run(fn):
                x = head.clone().requires_grad_(True)
                r_reg, r_cls = x.split([7, 1], dim=-1)
                term = fn(dict(item, R_reg=r_reg, R_cls=r_cls))
                term.backward()
                return term.detach(), x.grad

            (la, ga), (lb, gb) = run(loss._iou_fused), run(loss.iou_term_torch)
            assert torch.allclose(la, lb, rtol=1e-6) and torch.allclose(ga, gb, rtol=1e-5, atol=1e-7), "the two statements of the term disagree"
            say(f" stage-2 term, KIND {kind}, B = {batch}, {p.shape[1]} RoIs per frame, {int(item['M_rreg'].sum())} rows counted, term {float(la):.4f}")
            compare("fused, forward + backward", lambda: run(loss._iou_fused), "torch, forward + backward", lambda: run(loss.iou_term_torch),
                    args.windows, args.reps)
    for n in (300, 65536):
        a, b = (torch.from_numpy(x).cuda() for x in cases.random_pairs(n, seed=1))

        def run_op(fn):
            x = a.clone().requires_grad_(True)
            term = fn(x, b, "iou")
            term.sum().backward()
            return term.detach(), x.grad

        (ta, ga), (tb, gb) = run_op(iou3d_loss), run_op(iou3d_loss_torch)
        assert torch.allclose(ta, tb, rtol=0, atol=1e-6), "the aligned operator and its torch statement disagree"
        say(f" aligned operator, KIND iou, N = {n}")
        compare("native, forward + backward", lambda: run_op(iou3d_loss), "torch, forward + backward ", lambda: run_op(iou3d_loss_torch),
                args.windows, args.reps)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "iou_loss.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args(argv)
    tolerances()
    say()
    if torch.cuda.is_available():
        timings(args)
    else:
        say("no GPU: the timings are not taken")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
