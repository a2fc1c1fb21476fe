"""Time per call of the dynamic pillar encoder (cfg.PILLAR.DYNAMIC, csrc/pillar.hip "dynamic encoder") on 16k-point KITTI-like clouds
(vision3d_amd.synth) of the pillar grid, B = 1 and 8, on one device in one process, on the same inputs --
    eval     DynamicPillarFeatureNet.forward (three launches + the canvas scatter)            vs forward_torch
    train    DynamicPillarFeatureNet.forward + backward (five + two launches, autograd)       vs forward_torch + autograd
    pair     dynamic voxelizer + dynamic encoder   vs   hard voxelizer at 32 slots + PillarFeatureNet   (eval; no host read in either)
the launches per native call from a profiled pass, the share of in-range points the hard form drops, and the fp32 errors of the
kernels and of the fp32 torch statement against float64 over the cases of tests/pillar_dynamic_cases.py (the bounds of
tests/test_gpu_pillar_dynamic.py).  One way of building the point lists was built (exclusive scan + integer cursor); no variant to compare.

    python tools/mb_pillar_dynamic.py [--out profiles/pillar_dynamic.txt] [--windows 7] [--reps 20]

Timing method and helpers: tools/mb_pillar_encoder.py (device-plus-host time, alternating windows, medians)."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import mb_pillar_encoder as base  # noqa: E402
from vision3d_amd import synth  # noqa: E402
from vision3d_amd.core import Preprocessor  # noqa: E402
from vision3d_amd.core.config import pillar_car_cfg, pillar_dynamic_car_cfg  # noqa: E402
from vision3d_amd.detector import pillar as P  # noqa: E402

say, compare, kernel_times = base.say, base.compare, base.kernel_times


def errors():
    import pillar_dynamic_cases as cases
    import pillar_dynamic_ref as ref
    from pillar_dynamic_checks import grad_error, item_of, module_for, value_error
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
                got = value_error(native(item_of(c, "cuda")).cpu().numpy(), want) if not training else None
            if training:
                got = value_error(native(item_of(c, "cuda")).detach().cpu().numpy(), want)
            keep("rows (train)" if training else "rows (eval)", own, got)
            if training:
                for what in ("running_mean", "running_var"):
                    keep(what, value_error(getattr(stated.norm, what).cpu().numpy(), r[what].numpy()),
                         value_error(getattr(native.norm, what).cpu().numpy(), r[what].numpy()))
                y32 = ref.encode(c, training=True, dtype=torch.float32)
                own_mean, own_var = value_error(y32["mean"].numpy(), r["mean"].numpy()), value_error(y32["var"].numpy(), r["var"].numpy())
        it = item_of(c, "cuda")
        w, gamma, beta = (torch.from_numpy(c[k]).cuda() for k in ("weight", "gamma", "beta"))
        args = (it["flat_points"], it["point_voxel"], it["voxel_mean"], it["occupancy"], it["coordinates"], c["geom"])
        rows, winner, bn, moments = P.pillar_dynamic_train_forward(*args, w, gamma, beta, c["eps"])
        r = ref.encode(c, training=True)
        keep("batch mean", own_mean, value_error(bn[0].cpu().numpy(), r["mean"].numpy()))
        keep("batch var", own_var, value_error(bn[1].cpu().numpy(), r["var"].numpy()))
        got = P.pillar_dynamic_train_backward(*(args[:3] + args[4:]), w, gamma, c["eps"], rows, winner, torch.from_numpy(c["d_rows"]).cuda(), moments)
        given = winner.cpu().numpy()
        want = ref.gradients_given_winner(c, given)
        own = ref.gradients_given_winner(c, given, torch.float32)
        for what, g, t, o in zip(("dW", "d_gamma", "d_beta"), got, want, own):
            keep(what, grad_error(o.numpy(), t.numpy()), grad_error(g.cpu().numpy(), t.numpy()))
    say("fp32 errors against float64, largest over the live cases of tests/pillar_dynamic_cases.py: (the fp32 statement, the kernels)")
    say("  values relative to max(1, largest |reference|), gradients (winners given) relative to the tensor's largest entry;")
    say("  the statement of batch mean / var and of the gradients is the fp32 run of tests/pillar_dynamic_ref.py")
    for key, (own, got) in worst.items():
        say(f"  {key:14s} ({own:.2e}, {got:.2e})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pillar_dynamic.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    say("$ python tools/mb_pillar_dynamic.py " + " ".join(sys.argv[1:]))
    say(f"device: {torch.cuda.get_device_name(0)}")
    errors()
    from vision3d_amd.spconv.utils import voxelize_batch, voxelize_dynamic_batch
    cfg, hard_cfg = pillar_dynamic_car_cfg(), pillar_car_cfg()
    torch.manual_seed(0)
    net = P.DynamicPillarFeatureNet(cfg).cuda()
    hard = P.PillarFeatureNet(hard_cfg).cuda()
    hard.load_state_dict(net.state_dict())
    for B in (1, 8):
        clouds = [synth.make_cloud(s, n_points=16384) for s in range(B)]
        item = Preprocessor(cfg)(dict(points=clouds))
        item_h = Preprocessor(hard_cfg)(dict(points=clouds))
        occ = item["occupancy"]
        kept, kept_h = int(occ.sum()), int(item_h["occupancy"].sum())
        say(f"B = {B}: {item['flat_points'].shape[0]} points, {kept} in range, {occ.shape[0]} pillars, largest {int(occ.max())} points; the hard form "
            f"at {hard_cfg.MAX_OCCUPANCY} slots keeps {kept_h} ({100.0 * (kept - kept_h) / kept:.1f} % of the in-range points dropped)")
        net.eval(), hard.eval()
        with torch.no_grad():
            d = float((net(item) - net.forward_torch(item)).abs().max())
        say(f"  eval: native against forward_torch, largest difference {d:.2e}")

        def native_eval():
            with torch.no_grad():
                net(item)

        def torch_eval():
            with torch.no_grad():
                net.forward_torch(item)

        def hard_eval():
            with torch.no_grad():
                hard(item_h)
        say("  eval (encoder alone; the hard encoder on its own item beside it):")
        compare([("native dynamic", native_eval), ("forward_torch ", torch_eval), ("native hard   ", hard_eval)], a.windows, a.reps)
        say("  profiled pass, eval native:")
        kernel_times(native_eval)
        net.train(), hard.train()
        up = torch.randn((B, net.channels) + net.map_shape, device="cuda")

        def step(module, fn, it):
            def run():
                for p in module.parameters():
                    p.grad = None
                (fn(it) * up).sum().backward()
            return run
        say("  train forward + backward:")
        compare([("native dynamic", step(net, net, item)), ("forward_torch ", step(net, net.forward_torch, item)), ("native hard   ", step(hard, hard, item_h))],
                a.windows, a.reps)
        say("  profiled pass, train native:")
        kernel_times(step(net, net, item))
        # voxelizer + encoder, eval, no host read in either: outputs at capacity, the live count stays on the device -- the hard
        # pair reads min(points, B * MAX_VOXELS) rows of which the rows beyond n_voxels are zero-filled pillars of occupancy 0
        net.eval(), hard.eval()
        flat = torch.cat([torch.from_numpy(c).cuda() for c in clouds])
        offsets = [16384 * b for b in range(B + 1)]
        M = int(occ.shape[0])
        scale, shift = net._folded()
        w = net.linear.weight.detach()

        def pair_dynamic():
            coords, o, mean, pv, _ = voxelize_dynamic_batch(flat, offsets, cfg.VOXEL_SIZE, cfg.GRID_BOUNDS, cfg.MAX_VOXELS)
            return P.pillar_dynamic_encode(flat, pv, mean[:M], o[:M], coords[:M], net.geom, w, scale, shift)

        def pair_hard():
            voxels, coords, o, _, _ = voxelize_batch(flat, offsets, hard_cfg.VOXEL_SIZE, hard_cfg.GRID_BOUNDS, hard_cfg.MAX_OCCUPANCY, hard_cfg.MAX_VOXELS)
            return P.pillar_encode(voxels[:M], o[:M], coords[:M], hard.geom, w, scale, shift)
        assert torch.equal(pair_dynamic(), P.pillar_dynamic_encode(item["flat_points"], item["point_voxel"], item["voxel_mean"], occ, item["coordinates"],
                                                                   net.geom, w, scale, shift))
        say(f"  voxelizer + encoder, eval, {M} pillars (the count known to the host beforehand, no read in the clock):")
        compare([("dynamic pair      ", pair_dynamic), (f"hard pair, {hard_cfg.MAX_OCCUPANCY} slots", pair_hard)], a.windows, a.reps)
        say("  profiled pass, dynamic pair:")
        kernel_times(pair_dynamic)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(base.LINES) + "\n")


if __name__ == "__main__":
    main()
