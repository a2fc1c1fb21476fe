"""Time per call of the pillar feature encoder (cfg.PILLAR, csrc/pillar.hip) on 16k-point KITTI-like clouds (vision3d_amd.synth), on one
device in one process, on the same inputs --
    eval     PillarFeatureNet.forward (one launch + the canvas scatter)            vs forward_torch           (B = 1 and 8)
    train    PillarFeatureNet.forward + backward (three + two launches, autograd)   vs forward_torch + autograd (B = 1 and 8)
the launches per native call from a profiled pass, the fp32 errors of the kernels and of the fp32 torch statement against float64
over the cases of tests/pillar_cases.py (the bounds of tests/test_gpu_pillar.py), and the eager frames/s of the pillar SECOND beside
the eager sparse SECOND (`Second.inference(item)` on a Preprocessor item, B = 1, the voxelizer not timed), and in a section of its own
the voxelizer alone at 32 slots (the wide path) beside the 5-slot register path.

    python tools/mb_pillar_encoder.py [--out profiles/pillar_encoder.txt] [--windows 7] [--reps 20]

Device-plus-host time: a host clock around `reps` calls that end in a device synchronise, inputs resident on the device, medians
over repeated windows after a warm-up, the versions alternating window by window.  Results are compared before anything is timed.
The output is written to --out with the command line."""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from vision3d_amd import synth  # noqa: E402
from vision3d_amd.core import AnchorGenerator, Preprocessor  # noqa: E402
from vision3d_amd.core.config import pillar_car_cfg, second_car_cfg  # noqa: E402
from vision3d_amd.detector import Second  # noqa: E402
from vision3d_amd.detector import pillar as P  # noqa: E402

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
    return med


def kernel_times(fn, calls=10):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    launches = 0
    for ev in prof.key_averages():
        total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
        if total <= 0:
            continue
        launches += ev.count
        name = (ev.key.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "").strip() or ev.key)[:60]
        say(f"  kernel {name}: {total / max(ev.count, 1):7.1f} us per launch, {ev.count / calls:g} per call")
    say(f"  launches (kernels and copies) per call: {launches / calls:g}")


def errors():
    import pillar_cases as cases
    import pillar_ref as ref
    from pillar_checks import grad_error, item_of, module_for, value_error
    worst = {}

    def keep(key, own, got):
        o, g = worst.get(key, (0.0, 0.0))
        worst[key] = (max(o, own), max(g, got))
    for name in cases.CASE_IDS:
        if cases.CASES[name][0] == 0:
            continue
        c = cases.build(name)
        for training in (False, True):
            r = ref.encode(c, training=training)
            want = ref.canvas(r["rows"], c, cases.H, cases.W).numpy()
            stated, native = module_for(c).cuda().train(training), module_for(c).cuda().train(training)
            with torch.no_grad():
                own = value_error(stated.forward_torch(item_of(c, "cuda")).cpu().numpy(), want)
            if training:
                got = value_error(native(item_of(c, "cuda")).detach().cpu().numpy(), want)
            else:
                with torch.no_grad():
                    got = value_error(native(item_of(c, "cuda")).cpu().numpy(), want)
            keep("rows (train)" if training else "rows (eval)", own, got)
            if training:
                for what in ("running_mean", "running_var"):
                    keep(what, value_error(getattr(stated.norm, what).cpu().numpy(), r[what].numpy()),
                         value_error(getattr(native.norm, what).cpu().numpy(), r[what].numpy()))
        it = item_of(c, "cuda")
        w, gamma, beta = (torch.from_numpy(c[k]).cuda() for k in ("weight", "gamma", "beta"))
        args = (it["features"], it["occupancy"], it["coordinates"], c["geom"])
        rows, winner, bn, moments = P.pillar_train_forward(*args, w, gamma, beta, c["eps"])
        r = ref.encode(c, training=True)
        keep("batch mean", 0.0, value_error(bn[0].cpu().numpy(), r["mean"].numpy()))
        keep("batch var", 0.0, value_error(bn[1].cpu().numpy(), r["var"].numpy()))
        got = P.pillar_train_backward(*args, w, gamma, c["eps"], rows, winner, torch.from_numpy(c["d_rows"]).cuda(), moments)
        given = winner.cpu().numpy()
        want = ref.gradients_given_winner(c, given)
        own = ref.gradients_given_winner(c, given, torch.float32)
        for what, g, t, o in zip(("dW", "d_gamma", "d_beta"), got, want, own):
            keep(what, grad_error(o.numpy(), t.numpy()), grad_error(g.cpu().numpy(), t.numpy()))
    say("fp32 errors against float64, largest over the live cases of tests/pillar_cases.py: (the fp32 torch statement, the kernels)")
    say("  values relative to max(1, largest |reference|), gradients (winners given) relative to the tensor's largest entry;")
    say("  batch mean / var have no fp32 torch figure of their own (nn.BatchNorm1d keeps them inside)")
    for key, (own, got) in worst.items():
        say(f"  {key:14s} ({own:.2e}, {got:.2e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pillar_encoder.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    say("$ python tools/mb_pillar_encoder.py " + " ".join(sys.argv[1:]))
    say(f"device: {torch.cuda.get_device_name(0)}")
    errors()
    cfg = pillar_car_cfg()
    anchors = AnchorGenerator(cfg).anchors.cuda()
    torch.manual_seed(0)
    model = Second(cfg).cuda()
    net = model.vfe
    for B in (1, 8):
        item = Preprocessor(cfg)(dict(points=[synth.make_cloud(s, n_points=16384) for s in range(B)], anchors=anchors))
        M, Pn, C = item["features"].shape
        say(f"B = {B}: {M} pillars x {Pn} slots x {C} channels -> ({B}, {net.channels}, {net.map_shape[0]}, {net.map_shape[1]})")
        net.eval()
        with torch.no_grad():
            d = float((net(item) - net.forward_torch(item)).abs().max())
        say(f"  eval: native against forward_torch, largest difference {d:.2e}")

        def native_eval():
            with torch.no_grad():
                net(item)

        def torch_eval():
            with torch.no_grad():
                net.forward_torch(item)
        say("  eval:")
        compare([("native       ", native_eval), ("forward_torch", torch_eval)], a.windows, a.reps)
        say("  profiled pass, eval native:")
        kernel_times(native_eval)
        net.train()
        up = torch.randn((B, net.channels) + net.map_shape, device="cuda")

        def step(fn):
            def run():
                for p in net.parameters():
                    p.grad = None
                (fn(item) * up).sum().backward()
            return run
        say("  train forward + backward:")
        compare([("native       ", step(net)), ("forward_torch", step(net.forward_torch))], a.windows, a.reps)
        say("  profiled pass, train native:")
        kernel_times(step(net))
    # the voxelizer in front of both models, B = 1 and 8: 32 slots take the wide path of csrc/voxelize.hip (a thread per point walks its
    # pillar's list: quadratic in a pillar's point count), 5 slots the register path
    from vision3d_amd.spconv.utils import voxelize_batch
    sparse_cfg = second_car_cfg()
    say("voxelizer alone (v3d_voxelize, no host read), the same 16k-point clouds:")
    for B in (1, 8):
        clouds = [torch.from_numpy(synth.make_cloud(s, n_points=16384)).cuda() for s in range(B)]
        flat, offsets = torch.cat(clouds), [16384 * b for b in range(B + 1)]

        def vox(c):
            return lambda: voxelize_batch(flat, offsets, c.VOXEL_SIZE, c.GRID_BOUNDS, c.MAX_OCCUPANCY, c.MAX_VOXELS)
        occ = vox(cfg)()[2][:int(vox(cfg)()[4].item())]
        say(f"  B = {B}: {len(occ)} pillars, {int((occ == cfg.MAX_OCCUPANCY).sum())} of them full")
        compare([(f"pillars, {cfg.MAX_OCCUPANCY} slots (wide path)   ", vox(cfg)), (f"voxels, {sparse_cfg.MAX_OCCUPANCY} slots (register path)", vox(sparse_cfg))], a.windows, a.reps)
    # eager frames/s, B = 1: Second.inference(item) of both models, the Preprocessor outside the clock
    sparse = Second(sparse_cfg).cuda().eval()
    model.eval()
    cloud = [synth.make_cloud(0, n_points=16384)]
    item_p = Preprocessor(cfg)(dict(points=cloud, anchors=anchors))
    item_s = Preprocessor(sparse_cfg)(dict(points=cloud, anchors=AnchorGenerator(sparse_cfg).anchors.cuda()))

    def frame(m, item):
        def run():
            with torch.no_grad():
                m.inference(item)
        return run
    say("eager Second.inference(item), B = 1, one 16k-point cloud (voxelizer outside the clock):")
    med = compare([("pillar SECOND", frame(model, item_p)), ("sparse SECOND", frame(sparse, item_s))], a.windows, a.reps)
    say(f"  frames/s: pillar {1 / med[0]:.0f}, sparse {1 / med[1]:.0f}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
