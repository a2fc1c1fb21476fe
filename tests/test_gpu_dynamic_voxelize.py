"""GPU: dynamic voxelization (csrc/voxelize.hip "DYNAMIC") against its numpy restatement (tests/dynamic_voxel_ref.py), bit for bit --
coords, occupancy, mean, point_voxel, n_out --, its relation to the hard voxelizer, order independence, the backbone plan and the
models built with cfg.DYNAMIC_VOXELIZATION.  Every case first checks, on the RESTATEMENT's output, that its input exercises what it
is there for (conditions, not tolerances)."""
import copy

import numpy as np
import pytest
import torch

import dynamic_voxel_ref as ref
from gpu_util import dev
from vision3d_amd import synth

pytestmark = pytest.mark.gpu
VS = [0.05, 0.05, 0.1]
TINY_BOUNDS = [0.0, -4.0, -3.0, 6.4, 4.0, 1.0]  # the tiny grid of tests/test_gpu_pillar.py: a 20 x 16 BEV map
PILLAR_VS = [0.4, 0.4, 4.0]
ATOMIC, WALK, HYBRID = 0, 1, 2


@pytest.fixture(params=[ATOMIC, WALK, HYBRID], ids=["atomic", "walk", "hybrid"])
def variant(request):
    """Every way of forming the integer sums (v3d_voxelize_dynamic_variant; hybrid, the default, walks voxels of at most 32 points and
    adds the points of larger ones atomically -- the cases hold cells of 8, 9, 64, 65 and hundreds of points): same bits."""
    from vision3d_amd import _lib as L
    prev = L.lib().v3d_voxelize_dynamic_variant(request.param)
    yield request.param
    L.lib().v3d_voxelize_dynamic_variant(prev)


def gpu_dynamic(clouds, vs, bounds, max_voxels, want_point_map=True):
    from vision3d_amd.spconv.utils import voxelize_dynamic_batch
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist()
    flat = dev(np.concatenate(clouds), torch.float32)
    coords, occ, mean, pv, n_out = voxelize_dynamic_batch(flat, offs, vs, bounds, max_voxels, want_point_map)
    n_out = n_out.cpu().numpy()
    m = int(n_out[0])
    assert 0 <= m <= coords.shape[0]
    return dict(coords=coords[:m].cpu().numpy(), occupancy=occ[:m].cpu().numpy(), mean=mean[:m].cpu().numpy(),
                point_voxel=None if pv is None else pv.cpu().numpy(), n_out=n_out)


def same(got, want):
    for k in ("n_out", "coords", "occupancy", "point_voxel"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (k, got[k].shape, want[k].shape)
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert got["mean"].shape == want["mean"].shape and got["mean"].dtype == np.float32
    np.testing.assert_array_equal(got["mean"], want["mean"], err_msg="mean")  # (NaN == NaN here)
    np.testing.assert_array_equal(got["mean"].view(np.int32), want["mean"].view(np.int32), err_msg="mean, bits")


def squeezed(seed, n=16384):
    """A synthetic KITTI sweep squeezed into the tiny grid's bounds (x in [0, 6.4), y in [-4, 4)), as test_gpu_pillar.py's _clouds."""
    cloud = synth.make_cloud(seed, n_points=n).copy()
    cloud[:, 0] = cloud[:, 0] / 70.4 * 6.4
    cloud[:, 1] = cloud[:, 1] / 40.0 * 4.0
    return cloud.astype(np.float32)


def ragged_batch():
    clouds = [synth.make_cloud(2)[:9000].copy(), None, synth.make_cloud(4).copy(), synth.make_cloud(5)[:12345].copy()]
    clouds[0][::5, 0] = 70.4          # on the upper bound: dropped
    clouds[0][::9, 1] = -40.0         # on the lower bound: kept
    clouds[1] = clouds[0][-1:].copy()  # the last point of frame 0 and the first of frame 1 in the same (z, y, x) cell: two rows
    clouds[3][7, 2] = np.nan
    # cells of exactly 8, 9, 64, 65 and 300 points, each one point written over strided rows (36 apart: the 300 span 42 chunks of 256)
    rows = np.arange(8 + 9 + 64 + 65 + 300) * 36 + 5
    at = 0
    for j, k in enumerate((8, 9, 64, 65, 300)):
        clouds[2][rows[at:at + k]] = np.array([1.02 + j, -39.93, 0.93, 0.5], np.float32) + clouds[2][rows[at:at + k]] * np.float32(1e-4)
        at += k
    return clouds


@pytest.fixture(scope="module")
def ragged():
    clouds = ragged_batch()
    return clouds, ref.voxelize_dynamic(clouds, VS, synth.KITTI_BOUNDS, 20000)


@pytest.fixture(scope="module")
def crowded():
    """0.4 x 0.4 x 4 m pillars on a 16 k cloud squeezed into 6.4 x 8 m."""
    clouds = [squeezed(20)]
    return clouds, ref.voxelize_dynamic(clouds, PILLAR_VS, TINY_BOUNDS, 12000)


# ------------------------------------------------------------------------------------------------------- the op against the restatement
def test_single_kitti_frame_chained_form(variant):
    clouds = [synth.make_cloud(0)]
    want = ref.voxelize_dynamic(clouds, VS, synth.KITTI_BOUNDS, 20000)
    assert len(clouds[0]) == 16384 and want["n_out"][0] > 5000 and want["occupancy"].max() > 1
    same(gpu_dynamic(clouds, VS, synth.KITTI_BOUNDS, 20000), want)


def test_ragged_batch_edges(ragged, variant):
    clouds, want = ragged
    assert [len(c) for c in clouds] == [9000, 1, 16384, 12345]
    flat = np.concatenate(clouds)
    pv, occ, coords = want["point_voxel"], want["occupancy"], want["coords"]
    assert (pv[:9000][::5] == -1).all() and (pv[:9000][::9][(np.arange(9000)[::9] % 5) != 0] >= 0).all()  # upper dropped, lower kept
    assert np.isnan(flat[9001 + 16384 + 7, 2]) and pv[9001 + 16384 + 7] == -1
    assert {8, 9, 64, 65, 300} <= set(occ.tolist()) and occ.max() > 256
    big = int(np.argmax(occ))
    members = np.nonzero(pv == big)[0]
    assert len(members) == occ[big] and len(set((members // 256).tolist())) > 1  # its points straddle 256-point chunk edges
    a, b = pv[8999], pv[9000]
    assert a >= 0 and b >= 0 and a != b and coords[a, 0] == 0 and coords[b, 0] == 1 and (coords[a, 1:] == coords[b, 1:]).all()
    same(gpu_dynamic(clouds, VS, synth.KITTI_BOUNDS, 20000), want)


def test_two_frames_of_more_than_256_chunks(variant):
    clouds = [synth.make_cloud(10, 33000), synth.make_cloud(11, 33000)]
    assert -(-sum(len(c) for c in clouds) // 256) == 258  # the second trip of the scan over the chunk counts
    same(gpu_dynamic(clouds, VS, synth.KITTI_BOUNDS, 40000), ref.voxelize_dynamic(clouds, VS, synth.KITTI_BOUNDS, 40000))


def test_max_voxels_clip(variant):
    clouds = [synth.make_cloud(6), synth.make_cloud(7)[:3000], synth.make_cloud(8)]
    want = ref.voxelize_dynamic(clouds, VS, synth.KITTI_BOUNDS, 2500)
    _, inside, _ = ref.cells_of(np.concatenate(clouds), VS, synth.KITTI_BOUNDS)
    cut = inside & (want["point_voxel"] == -1)
    assert cut.sum() > 1000 and (np.bincount(want["coords"][:, 0]) == 2500).all()  # every frame is clipped
    got = gpu_dynamic(clouds, VS, synth.KITTI_BOUNDS, 2500)
    same(got, want)
    assert (got["point_voxel"][cut] == -1).all() and got["point_voxel"].max() == want["n_out"][0] - 1


@pytest.mark.parametrize("C", [3, 5, 8])
def test_other_channel_counts(C, variant):
    rng = np.random.default_rng([21, C])
    clouds = []
    for seed, n in ((12, 5000), (13, 3001)):
        base = synth.make_cloud(seed)[:n]
        extra = rng.uniform(-100.0, 100.0, size=(n, max(C - 4, 0))).astype(np.float32)
        clouds.append(np.ascontiguousarray(np.concatenate([base, extra], axis=1)[:, :C]))
        clouds[-1][::4] = clouds[-1][0]  # crowded cells for every channel count
    want = ref.voxelize_dynamic(clouds, VS, synth.KITTI_BOUNDS, 20000)
    assert want["mean"].shape[1] == C and want["occupancy"].max() > 64
    same(gpu_dynamic(clouds, VS, synth.KITTI_BOUNDS, 20000), want)


def test_pillar_grid_with_crowded_cells(crowded, variant):
    clouds, want = crowded
    assert want["occupancy"].max() >= 200
    same(gpu_dynamic(clouds, PILLAR_VS, TINY_BOUNDS, 12000), want)


def test_empty_and_all_outside(variant):
    from vision3d_amd.spconv.utils import voxelize_dynamic_batch
    out = voxelize_dynamic_batch(torch.zeros(0, 4).cuda(), [0, 0], VS, synth.KITTI_BOUNDS, 20000)
    np.testing.assert_array_equal(out[4].cpu().numpy(), [0, 0])
    far = np.full((100, 4), 1e6, np.float32)
    got = gpu_dynamic([far], VS, synth.KITTI_BOUNDS, 20000)
    np.testing.assert_array_equal(got["n_out"], [0, 0])
    assert (got["point_voxel"] == -1).all()
    same(got, ref.voxelize_dynamic([far], VS, synth.KITTI_BOUNDS, 20000))


def test_refused_values_set_the_status_bit_and_only_their_means(variant):
    clean = [synth.make_cloud(14)[:6000].copy(), synth.make_cloud(15)[:4000].copy()]
    base = gpu_dynamic(clean, VS, synth.KITTI_BOUNDS, 20000)
    assert base["n_out"][1] == 0
    dirty = [c.copy() for c in clean]
    dirty[0][123, 3] = np.nan
    dirty[1][77, 3] = 1e6
    want = ref.voxelize_dynamic(dirty, VS, synth.KITTI_BOUNDS, 20000)
    got = gpu_dynamic(dirty, VS, synth.KITTI_BOUNDS, 20000)
    same(got, want)
    assert got["n_out"][1] & 1
    rows = [int(got["point_voxel"][123]), int(got["point_voxel"][6000 + 77])]
    assert min(rows) >= 0 and rows[0] != rows[1]
    nan = np.isnan(got["mean"])
    assert nan.sum() == 2 and nan[rows[0], 3] and nan[rows[1], 3]
    for k in ("coords", "occupancy", "point_voxel"):
        np.testing.assert_array_equal(got[k], base[k])
    np.testing.assert_array_equal(got["mean"][~nan].view(np.int32), base["mean"][~nan].view(np.int32))


# ------------------------------------------------------------------------------------------------- relation to the hard voxelizer
@pytest.mark.parametrize("case, max_pts", [("ragged", 5), ("crowded", 5), ("crowded", 32)])
def test_same_cells_as_the_hard_voxelizer(ragged, crowded, case, max_pts):
    from vision3d_amd.spconv.utils import voxelize_batch
    clouds, _ = ragged if case == "ragged" else crowded
    vs, bounds, mv = (VS, synth.KITTI_BOUNDS, 20000) if case == "ragged" else (PILLAR_VS, TINY_BOUNDS, 12000)
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).tolist()
    _, coords, occ, _, n = voxelize_batch(dev(np.concatenate(clouds), torch.float32), offs, vs, bounds, max_pts, mv)
    m = int(n.item())
    got = gpu_dynamic(clouds, vs, bounds, mv)
    assert got["n_out"][0] == m
    np.testing.assert_array_equal(got["coords"], coords[:m].cpu().numpy())
    np.testing.assert_array_equal(occ[:m].cpu().numpy(), np.minimum(got["occupancy"], max_pts))
    assert (got["occupancy"] > max_pts).any()


# ------------------------------------------------------------------------------------------------------------ order, repeatability
@pytest.mark.parametrize("case", ["ragged", "crowded"])
def test_repeatable_and_independent_of_the_point_order(ragged, crowded, case, variant):
    clouds, want = ragged if case == "ragged" else crowded
    vs, bounds, mv = (VS, synth.KITTI_BOUNDS, 20000) if case == "ragged" else (PILLAR_VS, TINY_BOUNDS, 12000)
    first, second = gpu_dynamic(clouds, vs, bounds, mv), gpu_dynamic(clouds, vs, bounds, mv)
    same(second, first)  # row order included
    rng = np.random.default_rng(31)
    shuffled = [c[rng.permutation(len(c))] for c in clouds]
    other = gpu_dynamic(shuffled, vs, bounds, mv)
    assert not np.array_equal(other["coords"], first["coords"])  # (the rows do move)
    for a, b in zip(ref.by_cell(other), ref.by_cell(first)):
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------------ the plan
def tiny_cfg(dynamic=True):
    from vision3d_amd.core.config import second_car_cfg
    cfg = second_car_cfg()
    cfg.merge_from_dict(dict(GRID_BOUNDS=list(TINY_BOUNDS), MAX_VOXELS=6000, DYNAMIC_VOXELIZATION=dict(ENABLED=dynamic)))
    return cfg


def tiny_clouds(seeds=(0, 1), n=4096):
    out = []
    for s in seeds:
        c = squeezed(s, n)
        c[::6] = c[1]  # a crowded cell whatever the cloud
        out.append(c)
    return out


def tiny_model(dynamic=True, seed=0):
    from gpu_util import randomize_bn
    from vision3d_amd.detector import Second
    cfg = tiny_cfg(dynamic)
    torch.manual_seed(seed)
    model = Second(cfg).cuda()
    randomize_bn(model, 0)
    return cfg, model


@pytest.mark.parametrize("dynamic", [True, False], ids=["dynamic", "default"])
def test_plan_from_points_equals_plan_from_the_ops_voxels(dynamic):
    """BackbonePlan.forward(points) against forward_voxels(mean, coords) fed with the op's output: the same kernels on the same stage-0
    arrays, so bit for bit -- in the default mode (the hard voxelizer's output) and in the dynamic mode alike."""
    from vision3d_amd.spconv.utils import voxelize_batch, voxelize_dynamic_batch
    cfg, model = tiny_model(dynamic)
    model.eval()
    clouds = tiny_clouds()
    offs = [0, len(clouds[0]), len(clouds[0]) + len(clouds[1])]
    flat = dev(np.concatenate(clouds), torch.float32)
    plan = model.backbone_plan(2, 16384)
    assert plan.dynamic_voxels == dynamic
    with torch.no_grad():
        from_points = plan.forward(flat, offs).clone()
        status = int(plan.voxel_status().item())
        n_plan = int(plan.layer_output(-1)[2].item())
        if dynamic:
            coords, occ, mean, _, n_out = voxelize_dynamic_batch(flat, offs, cfg.VOXEL_SIZE, cfg.GRID_BOUNDS, cfg.MAX_VOXELS, False)
            m = int(n_out[0].item())
            assert int(occ[:m].max()) > cfg.MAX_OCCUPANCY
        else:
            _, coords, occ, mean, n = voxelize_batch(flat, offs, cfg.VOXEL_SIZE, cfg.GRID_BOUNDS, cfg.MAX_OCCUPANCY, cfg.MAX_VOXELS, False)
            m = int(n.item())
        from_voxels = plan.forward_voxels(mean[:m], coords[:m], 2)
    assert status == 0 and n_plan == m and float(from_points.abs().max()) > 0
    np.testing.assert_array_equal(from_points.cpu().numpy(), from_voxels.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------------- the models
def test_second_inference_paths_agree():
    """inference(item), inference_points and graphed_inference on a model built with the key: the rule tests/test_gpu_dropin.py and
    tests/test_gpu_proposal.py apply to these paths in the default mode -- equal arrays."""
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    cfg, model = tiny_model()
    model.eval()
    assert model.dynamic_voxels
    anchors = AnchorGenerator(cfg).anchors.cuda()
    clouds = tiny_clouds()
    dev_clouds = [torch.from_numpy(c).cuda() for c in clouds]
    with torch.no_grad():
        item = Preprocessor(cfg, seed=0)(dict(points=clouds, anchors=anchors))
        assert "features" not in item and item["point_voxel"].shape == (sum(len(c) for c in clouds),)
        assert int(item["occupancy"].max()) > cfg.MAX_OCCUPANCY
        assert item["voxel_mean"].shape == (item["coordinates"].shape[0], cfg.C_IN) and item["batch_size"] == 2
        want = ref.voxelize_dynamic(clouds, cfg.VOXEL_SIZE, cfg.GRID_BOUNDS, cfg.MAX_VOXELS)
        np.testing.assert_array_equal(item["voxel_mean"].cpu().numpy().view(np.int32), want["mean"].view(np.int32))
        np.testing.assert_array_equal(item["point_voxel"].cpu().numpy(), want["point_voxel"])
        from_item = [t.clone() for t in model.inference(item)]
        from_points = [t.clone() for t in model.inference_points(dev_clouds, anchors)]
        graphed = model.graphed_inference(anchors, [len(c) for c in clouds])
        from_graph = [t.clone() for t in graphed(dev_clouds)]
    assert from_item[0].shape[1] == 7 and len(from_item[0]) == len(from_item[3]) > 0
    for other in (from_points, from_graph):
        for got, want_t in zip(other, from_item):
            np.testing.assert_array_equal(got.cpu().numpy(), want_t.cpu().numpy())


def test_second_preprocessor_raises_on_a_refused_value():
    from vision3d_amd.core import Preprocessor
    cfg = tiny_cfg()
    clouds = tiny_clouds((2,))
    clouds[0][10, 3] = np.inf
    assert ref.voxelize_dynamic(clouds, cfg.VOXEL_SIZE, cfg.GRID_BOUNDS, cfg.MAX_VOXELS)["n_out"][1] == 1
    with pytest.raises(ValueError, match="2\\^16"):
        Preprocessor(cfg, seed=0)(dict(points=clouds))


def test_second_trains_on_the_native_plans():
    """One training step of a model built with the key: forward + ProposalLoss + backward on the native plans."""
    from vision3d_amd.core import Preprocessor, ProposalTargetAssigner
    from vision3d_amd.detector import ProposalLoss
    cfg, model = tiny_model()
    model.train()
    assigner = ProposalTargetAssigner(cfg)
    gts = [np.array([[2.2, -1.1, -1.0, 1.6, 3.9, 1.56, 0.05]], np.float32), np.array([[4.1, 0.7, -1.0, 1.6, 3.9, 1.56, 1.5]], np.float32)]
    targets = [assigner(dict(boxes=torch.from_numpy(g), class_idx=torch.zeros(len(g), dtype=torch.long),
                             box_ignore=torch.zeros(len(g), dtype=torch.bool))) for g in gts]
    item = Preprocessor(cfg, seed=0)(dict(points=[torch.from_numpy(c).cuda() for c in tiny_clouds()]))
    assert "features" not in item
    item.update({k: torch.stack([t[k] for t in targets]) for k in ("G_cls", "G_reg", "M_cls", "M_reg")})
    assert int(item["M_reg"].sum()) > 0
    out = model(item)
    assert isinstance(out["_head_maps"], tuple) and out["_head_maps"][0].dtype == torch.float32
    losses = ProposalLoss(cfg)(out)
    assert torch.isfinite(losses["loss"])
    losses["loss"].backward()
    assert model.torch_dense_fallbacks == 0
    first_conv = [p for n, p in model.cnn.named_parameters() if p.dim() > 1][0]
    for p in (first_conv, model.rpn.down_block[1].weight):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0


def test_pv_rcnn_inference_runs_and_is_independent_of_the_point_order():
    """PV_RCNN built with the key: `inference` runs; fed the same clouds permuted it computes the same STAGE-1 head maps.  Stage 2 is
    not compared: the keypoints are a farthest-point chain started at input point 0 and the padding resamples by input position, so
    its inputs depend on the point order by definition.  The voxel means are bit-identical under the permutation (tests above); the
    rows of the sparse tensors move with the first-touch order, which may reorder fp32 sums inside the backbone -- the head maps are
    held to the project's feature bar (gpu_util.assert_features_close), not to bit equality."""
    from gpu_util import assert_features_close, randomize_bn
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    from vision3d_amd.core.config import second_car_cfg
    from vision3d_amd.detector import PV_RCNN
    cfg = second_car_cfg()
    cfg.merge_from_dict(dict(DYNAMIC_VOXELIZATION=dict(ENABLED=True)))
    torch.manual_seed(0)
    model = PV_RCNN(cfg).cuda()
    randomize_bn(model, 1)
    model.eval()
    assert model.dynamic_voxels
    anchors = AnchorGenerator(cfg).anchors.cuda()
    cloud = synth.make_cloud(16)
    cloud[::8] = cloud[2]
    shuffled = cloud[np.random.default_rng(5).permutation(len(cloud))]
    maps = []
    with torch.no_grad():
        for pts in (cloud, shuffled):
            item = Preprocessor(cfg, seed=0)(dict(points=[pts], anchors=anchors))
            assert "features" not in item and int(item["occupancy"].max()) > cfg.MAX_OCCUPANCY
            boxes, bidx, cidx, scores = model.inference(item)
            assert boxes.shape == (len(bidx), 7) and len(bidx) == len(cidx) == len(scores)
            maps.append((item["P_cls"].float().cpu().numpy(), item["P_reg"].float().cpu().numpy()))
    for name, a, b in zip(("P_cls", "P_reg"), maps[1], maps[0]):
        print("dynamic-pvrcnn-figures", dict(map=name, max_abs_diff=float(np.abs(a - b).max()), largest=float(np.abs(b).max())))
        assert_features_close(a, b, name)


# ----------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from vision3d_amd.core import Preprocessor
    from vision3d_amd.core.config import pillar_car_cfg
    from vision3d_amd.detector import PV_RCNN, Second
    from vision3d_amd.spconv.utils import voxelize_dynamic_batch
    cfg = pillar_car_cfg()
    cfg.merge_from_dict(dict(DYNAMIC_VOXELIZATION=dict(ENABLED=True)))
    for build in (Second, Preprocessor):
        with pytest.raises(ValueError, match="DYNAMIC_VOXELIZATION"):
            build(cfg)
    with pytest.raises(ValueError, match="PILLAR"):
        PV_RCNN(cfg)
    pts = torch.zeros((8, 4), device="cuda")
    with pytest.raises(RuntimeError, match="unsupported"):
        voxelize_dynamic_batch(pts, [0, 8], [100.0, 100.0, 100.0], [-1e5, -1e5, -1e5, 1e5, 1e5, 1e5], 100)
    with pytest.raises(RuntimeError, match="unsupported"):
        voxelize_dynamic_batch(pts, [0, 8], VS, [0, -40, -3, 70.4, 65536.0, 1], 100)
    old = copy.deepcopy(tiny_cfg(False))
    del old["DYNAMIC_VOXELIZATION"]  # a configuration written before the key existed: disabled
    assert not Preprocessor(old).dynamic and not Second(old).dynamic_voxels
