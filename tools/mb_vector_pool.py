"""Time per call of VectorPool aggregation (cfg.VECTORPOOL) on the synthetic KITTI frame, B = 1: for every feature source of the
keypoint stage (16 384 raw points and the four backbone levels around 2 048 keypoints) and for RoI-grid pooling (21 600 queries on the
2 048 keypoints: 216 grid points in each of 100 RoIs around the frame's objects), one group at a time: the native
search (v3d_vector_pool_query) against `query_torch`, the native embedding (v3d_vector_pool_embed) against the torch statements on
the same neighbours, and the whole module (native against forward_torch with native = False) -- on the same device in the same
process.  In a section of its own: the keypoint-feature stage of the enabled model against the default set-abstraction stage on the
same frame.

    python tools/mb_vector_pool.py [--out profiles/vector_pool.txt] [--windows 5] [--reps 10]

Device-plus-host time: a host clock around `reps` calls that end in a device synchronise, inputs resident on the device, medians over
repeated windows after a warm-up of every shape, the versions alternating window by window.  The kernels' own times come from a
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
from vision3d_amd.core import AnchorGenerator, Preprocessor  # noqa: E402
from vision3d_amd.core.config import second_car_cfg  # noqa: E402
from vision3d_amd.detector import PV_RCNN  # noqa: E402
from vision3d_amd.detector import vector_pool as V  # noqa: E402

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
    """named: [(name, fn, reps scale)] timed in alternating windows (all see the same drift of the host); ratios against the first."""
    for _, fn, _ in named:
        fn(), fn()
    times = [[] for _ in named]
    for _ in range(windows):
        for t, (_, fn, scale) in zip(times, named):
            t.append(window(fn, max(1, reps // scale)))
    med = [statistics.median(t) for t in times]
    for (name, _, _), t, m in zip(named, times, med):
        tail = "" if m is med[0] else f"   ratio {m / med[0]:.1f}x"
        say(f"  {name}: {m * 1e6:10.1f} us per call ({min(t) * 1e6:.1f} .. {max(t) * 1e6:.1f}){tail}")


def kernel_times(fn, needles, calls=5):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    for ev in prof.key_averages():
        if any(s in ev.key for s in needles):
            total = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0.0)
            say(f"  kernel {ev.key.split('(')[0].split()[-1]}: {total / max(ev.count, 1):8.1f} us per launch, {ev.count // calls} per call")


KERNELS = ("bq_grid_build_kernel", "vpq_query_kernel", "vp_embed_kernel", "vp_reduce_kernel", "linear_rows_kernel")


def time_module(name, mod, xyz, feat, q, args):
    """One module: per group the search and the embedding against their torch statements, then the whole module."""
    b, n, _ = xyz.shape
    m = q.shape[1]
    say(f"{name}: {n} support rows x {feat.shape[2]} channels (reduced to {mod.reduced}), {m} queries")
    with torch.no_grad():
        fr = V.vector_pool_reduce(feat.contiguous(), mod.reduced)
        folded = mod._folded()[0]
        for k, (g, (w_local, shift, _)) in enumerate(zip(mod.groups, folded)):
            idx, w = V.vector_pool_query(xyz, q, g.voxels, g.radius)
            idx_t, w_t = V.query_torch(xyz, q, g.voxels, g.radius)
            same = float((idx.long() == idx_t).float().mean())
            found = (idx >= 0).sum(-1).reshape(-1)
            say(f" group {k}: VOXELS {list(g.voxels)}, radius {g.radius:g} m, {m * g.nv} centres, neighbours found 0/1/2/3: "
                f"{torch.bincount(found, minlength=4).tolist()}, indices equal to query_torch on {100 * same:.3f} %")
            assert same > 0.999, "native search and query_torch disagree"
            out = torch.empty((b * m, g.nv * g.local), device="cuda")
            a = V.vector_pool_embed(fr, xyz, q, idx, w, g.voxels, g.radius, w_local, shift, out).clone()
            ref = mod.embed_torch(fr, xyz, q, idx.long(), w, g)
            assert torch.allclose(a, ref, rtol=1e-4, atol=1e-5 * float(ref.abs().max())), "native and torch embedding disagree"

            def query_native(g=g):
                with torch.no_grad():
                    return V.vector_pool_query(xyz, q, g.voxels, g.radius)

            def query_stated(g=g):
                with torch.no_grad():
                    return V.query_torch(xyz, q, g.voxels, g.radius)

            def embed_native(g=g, idx=idx, w=w, w_local=w_local, shift=shift, out=out):
                with torch.no_grad():
                    return V.vector_pool_embed(fr, xyz, q, idx, w, g.voxels, g.radius, w_local, shift, out)

            def embed_stated(g=g, idx=idx.long(), w=w):
                with torch.no_grad():
                    return mod.embed_torch(fr, xyz, q, idx, w, g)

            compare([("search, native (grid build + query)", query_native, 1), ("search, query_torch                ", query_stated, 10)], args.windows, args.reps)
            compare([("embedding, native          ", embed_native, 1), ("embedding, torch statements", embed_stated, 1)], args.windows, args.reps)

        def whole_native():
            with torch.no_grad():
                return mod.forward_native(xyz, feat, q)

        def whole_stated():
            mod.native = False
            try:
                with torch.no_grad():
                    return mod.forward_torch(xyz, feat, q)
            finally:
                del mod.native

        x, y = whole_native(), whole_stated()
        assert torch.allclose(x, y, rtol=1e-4, atol=1e-5 * float(y.abs().max())), "native and torch module disagree"
        say(" whole module (reduce, every group's search + embedding + MLP, MSG_POST)")
        compare([("native                      ", whole_native, 1), ("forward_torch, native = False", whole_stated, 10)], args.windows, args.reps)
        kernel_times(whole_native, KERNELS)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vector_pool.txt"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args(argv)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    say("python tools/mb_vector_pool.py " + " ".join(sys.argv[1:] if argv is None else argv))
    cloud = synth.make_cloud(0)
    cfg = second_car_cfg()
    cfg.VECTORPOOL.ENABLED = True
    anchors = AnchorGenerator(cfg).anchors.cuda()
    torch.manual_seed(0)
    model = PV_RCNN(cfg).cuda().eval()
    for mod in model.modules():  # (the initialisation's weights give outputs of 1e-5: the comparisons would be vacuous)
        if isinstance(mod, V.VectorPoolAggregationMSG):
            with torch.no_grad():
                for name, p in mod.named_parameters():
                    if p.dim() >= 2:
                        p.normal_(0.0, 1.5 / p.shape[-2 if p.dim() == 3 else -1] ** 0.5)
    make = lambda: Preprocessor(cfg, seed=0)(dict(points=[cloud], anchors=anchors))
    with torch.no_grad():
        item = model.proposal(make())
        torch.cuda.synchronize()
        kp = item["keypoints"].contiguous()
        xyz, reflectance = item["points"].split([3, 1], dim=-1)
        sources = [(xyz.contiguous(), reflectance), *item["_cnn_features"]]
        say(f"keypoint stage: B = 1, {kp.shape[1]} keypoints, sources " + ", ".join(f"{x.shape[1]} x {f.shape[2]}" for x, f in sources))
        for i, (pnet, (x, f)) in enumerate(zip(model.pnets, sources)):
            time_module(f"source {i}", pnet, x.contiguous(), f, kp, args)
        # RoI-grid pooling: 21 600 queries (100 RoIs around the frame's objects x 216 grid points) on the keypoints
        feats = model.point_feature_extract(item, item["_cnn_features"], item["_bev_map"])
        rois = torch.from_numpy(synth.jitter_rois(synth.make_gt_boxes(0), 100, np.random.default_rng(0))[None]).cuda()
        samples = torch.rand((1, 100, 216, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
        from vision3d_amd.detector.roi_grid_pool import gridpoints
        grid_q = gridpoints(rois, samples).reshape(1, -1, 3).contiguous()
        time_module("RoI-grid pooling", model.roi_grid_pool.pnet, kp, feats.transpose(1, 2).contiguous(), grid_q, args)

        # ---- the keypoint-feature stage: enabled model against the default set-abstraction stage, same frame, keypoints given
        say("keypoint-feature stage (PV_RCNN.point_feature_extract, keypoints given), same frame")

        def enabled():
            with torch.no_grad():
                return model.point_feature_extract(item, item["_cnn_features"], item["_bev_map"])

        cfg0 = second_car_cfg()
        torch.manual_seed(0)
        model0 = PV_RCNN(cfg0).cuda().eval()
        item0 = model0.proposal(Preprocessor(cfg0, seed=0)(dict(points=[cloud], anchors=anchors)))
        torch.cuda.synchronize()

        def default():
            with torch.no_grad():
                return model0.point_feature_extract(item0, item0["_cnn_features"], item0["_bev_map"])

        assert enabled().shape == default().shape
        compare([("set abstraction (default, fused single-matrix path)", default, 1), ("VectorPool aggregation (op-by-op branch)           ", enabled, 1)],
                args.windows, args.reps)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
