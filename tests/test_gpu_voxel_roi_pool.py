"""GPU: voxel RoI pooling for PV-RCNN's stage 2 (csrc/voxel_pool.hip, detector/voxel_roi_pool.py) -- the native query exactly against
the float64 restatement (tests/voxel_roi_pool_ref.py) on hand-built levels, the fused pooling against it under the bar of the torch
float32 statements' own error, the module (native against its torch path, row permutations, graph capture) and PV_RCNN with the
pooling enabled (inference, the pipelined form, a train step) and disabled (outputs unchanged)."""
import numpy as np
import pytest
import torch

import voxel_roi_pool_ref as R
from gpu_util import assert_fp32_class, dev
from test_host_voxel_roi_pool import as_levels, pool_cfg, randomize, small_cfg, small_levels
from vision3d_amd import synth
from vision3d_amd.core.config import second_car_cfg

pytestmark = pytest.mark.gpu

RANGE, RADIUS, NSAMPLE = (1, 2, 2), 1.1, 4


def _device_level(level, extra=37, n=None, seed=0):
    """VoxelLevel on the GPU with `extra` garbage rows behind the live ones (coordinates of OTHER live sites of frame 0 and values
    far outside the grid, NaN features) and the live count in device memory."""
    from vision3d_amd.detector.voxel_roi_pool import VoxelLevel
    rng = np.random.default_rng(seed)
    coords, feats = level["coords"], level["feats"]
    n = coords.shape[0] if n is None else n
    junk = coords[rng.integers(0, max(coords.shape[0], 1), extra)].copy() if coords.shape[0] else np.zeros((extra, 4), np.int32)
    junk[::2] = [0, 1, 3, 3] if coords.shape[0] else [0, 0, 0, 0]
    junk[1::3, 1:] += 1000
    all_coords = np.concatenate([coords[:n], junk]).astype(np.int32)
    all_feats = np.concatenate([feats[:n], np.full((extra, feats.shape[1]), np.nan, np.float32)])
    return VoxelLevel(dev(all_feats), dev(all_coords), torch.tensor([n], dtype=torch.int32).cuda(), level["shape"], 2)


@pytest.mark.parametrize("grid", [2, 6])
def test_voxel_query_equals_the_restatement_exactly(grid):
    """B = 2, 3 RoIs per frame (inside / on the site frame 0 alone owns, straddling the edge, wholly outside), (5, 24, 24) level with
    ~300 sites per frame, NSAMPLE 4 (truncation), RANGE (1, 2, 2), n < cap with garbage rows behind n -- some of them repeating a
    live coordinate with another row index, which must never be returned.  Undecidable points (<= 2 %) are left out."""
    from vision3d_amd.detector.voxel_roi_pool import voxel_query
    level = R.make_level(11)
    rois = R.make_rois(12, level)
    boxes = dev(rois)
    samples = dev(np.broadcast_to(R.grid_samples(grid), (2, 3, grid ** 3, 3)).copy())
    from vision3d_amd.detector.roi_grid_pool import gridpoints
    pts = gridpoints(boxes, samples).reshape(-1, 3)
    pts64 = R.grid_points(rois, grid).reshape(-1, 3)
    assert float(np.abs(pts.cpu().numpy() - pts64).max()) < 1e-5
    frames = np.repeat(np.arange(2), 3 * grid ** 3)
    want, want_empty, und = R.voxel_query(pts64, frames, level["coords"], level["shape"], level["scale"], level["offset"], RANGE, RADIUS, NSAMPLE)
    print(f"[voxel query G={grid}] {len(pts64)} points, {int(und.sum())} undecidable, {int(want_empty.sum())} empty")
    assert und.mean() <= 0.02
    lv = _device_level(level)
    idx, empty = voxel_query(pts, 3 * grid ** 3, lv, level["scale"].tolist(), level["offset"].tolist(), RANGE, RADIUS, NSAMPLE)
    idx, empty = idx.cpu().numpy(), empty.cpu().numpy().astype(bool)
    assert idx.max() < level["coords"].shape[0] and idx.min() >= -1
    keep = ~und
    np.testing.assert_array_equal(idx[keep], want[keep])
    np.testing.assert_array_equal(empty[keep], want_empty[keep])
    assert empty.reshape(2, 3, -1)[:, 2].all() and (idx[empty] == -1).all()
    # storage order: the same level with its rows permuted gives the same SITES (rows mapped through the permutation)
    perm = np.random.default_rng(1).permutation(level["coords"].shape[0])
    shuffled = dict(level, coords=level["coords"][perm], feats=level["feats"][perm])
    idx_p, empty_p = voxel_query(pts, 3 * grid ** 3, _device_level(shuffled), level["scale"].tolist(), level["offset"].tolist(), RANGE, RADIUS, NSAMPLE)
    idx_p = idx_p.cpu().numpy()
    np.testing.assert_array_equal(np.where(idx_p >= 0, perm[np.maximum(idx_p, 0)], -1), idx)
    np.testing.assert_array_equal(empty_p.cpu().numpy().astype(bool), empty)


def test_voxel_query_of_a_level_without_rows():
    from vision3d_amd.detector.voxel_roi_pool import VoxelLevel, voxel_query
    level = R.make_level(11)
    pts = dev(R.grid_points(R.make_rois(12, level), 2).reshape(-1, 3).astype(np.float32))
    for lv in (_device_level(level, n=0), VoxelLevel(torch.empty((0, 8), device="cuda"), torch.empty((0, 4), dtype=torch.int32, device="cuda"), None,
                                                     level["shape"], 2)):
        idx, empty = voxel_query(pts, 3 * 8, lv, level["scale"].tolist(), level["offset"].tolist(), RANGE, RADIUS, NSAMPLE)
        assert bool((idx == -1).all()) and bool(empty.all())


@pytest.mark.parametrize("k,col", [(0, 0), (1, 32)])
def test_voxel_pool_pair_against_float64(k, col):
    """The fused pooling of one level (first-layer products per voxel on v3d_linear_rows + v3d_voxel_pool_pair) on the native query's
    indices against the float64 restatement on the same indices, under gpu_util's strict rule: 2e-4 or twice the error the torch
    float32 statements show against float64 on the same inputs (a K <= 35 and a K = 32 dot product summed in another order, the
    BatchNorm folded into the weights instead of applied behind the product).  Widths (16 -> 32) and (32 -> 32); the level's block is
    written at column `col` of a (rows, 64) matrix whose other columns keep their sentinel; empty points read exact zeros.
    Measured on an MI355X (strict relative error against float64, levels 0 / 1): native 8.5e-6 / 1.8e-5, torch float32 1.4e-5 / 3.0e-5."""
    from vision3d_amd.detector import VoxelRoiPool
    from vision3d_amd.detector.voxel_roi_pool import voxel_pool_pair, voxel_query
    from vision3d_amd.pointnet2.pointnet2_utils import linear_rows
    pool = randomize(VoxelRoiPool(small_cfg(3)), 7).cuda().eval()
    level = small_levels(3)[k]
    rois = R.make_rois(5, small_levels(3)[0])
    pts64 = R.grid_points(rois, 3).reshape(-1, 3)
    pts = dev(pts64.astype(np.float32))
    lv = _device_level(level)
    scale, offset = pool.level_geometry(k)
    idx, empty = voxel_query(pts, 3 * 27, lv, scale, offset, pool.ranges[k], pool.radii[k], pool.nsample)
    assert 0 < int(empty.sum()) < empty.numel()
    w1f, wx, b1, w2, b2 = pool._folded(k)
    wide = torch.full((pts.shape[0], 64), -7.0, device="cuda")
    p = linear_rows(lv.features, w1f)  # (the garbage rows' NaN products are never gathered)
    voxel_pool_pair(p, lv.coords, pts, idx, scale, offset, wx, b1, w2, b2, wide[:, col:col + 32])
    other = wide[:, 32:] if col == 0 else wide[:, :32]
    assert bool((other == -7.0).all()), "columns outside the block changed"
    got = wide[:, col:col + 32].cpu().numpy()
    state = {n: v.cpu().numpy() for n, v in pool.state_dict().items()}
    want = R.pool_level(pts.cpu().numpy(), idx.cpu().numpy(), level["coords"], level["feats"], np.asarray(scale, np.float32), np.asarray(offset, np.float32),
                        R.mlp_layers(state, f"mlps.{k}."))
    with torch.no_grad():
        own = pool.pool_torch(pts, idx.long(), dev(level["feats"]), dev(level["coords"]), k).cpu().numpy()
    from gpu_util import strict_rel_err
    print(f"[voxel pool level {k}] strict rel err native {strict_rel_err(got, want):.3e}, torch fp32 {strict_rel_err(own, want):.3e}")
    assert float(np.abs(want).max()) > 0.1
    assert_fp32_class(got, own, f"pooled rows of level {k}", ref64=want, own_factor=2.0)
    assert (got[empty.cpu().numpy().astype(bool)] == 0.0).all() and (want[empty.cpu().numpy().astype(bool)] == 0.0).all()
    wide2 = torch.full((pts.shape[0], 64), -7.0, device="cuda")
    voxel_pool_pair(p, lv.coords, pts, idx, scale, offset, wx, b1, w2, b2, wide2[:, col:col + 32])
    assert torch.equal(wide, wide2), "two runs differ"


def _module_case(grid=3):
    from vision3d_amd.detector import VoxelRoiPool
    pool = randomize(VoxelRoiPool(small_cfg(grid)), 7).cuda().eval()
    levels = small_levels(3)
    rois = R.make_rois(5, levels[0])
    return pool, levels, rois


def test_module_native_against_torch_and_float64():
    pool, levels, rois = _module_case()
    state = {n: v.cpu().numpy() for n, v in pool.state_dict().items()}
    want, und = R.voxel_roi_pool(rois, levels, dict(GRID=3, RANGE=pool.ranges, RADIUS=pool.radii, NSAMPLE=pool.nsample), state)
    boxes, lv = dev(rois), as_levels(levels, pool.strides, "cuda")
    with torch.no_grad():
        assert pool.native_ok(boxes, lv)
        got = pool(boxes, lv)
        own = pool.forward_torch(boxes, lv)
    assert torch.is_grad_enabled() and not pool.native_ok(boxes, lv)  # under autograd: the torch statements
    keep = ~und
    assert keep.sum() >= 3 and got.shape == (2, 3, 256)
    assert_fp32_class(got.cpu().numpy()[keep], own.cpu().numpy()[keep], "pooled RoI features", ref64=want[keep], own_factor=2.0)
    # storage order does not matter: rows of every level permuted (coordinates and features together) -> the same bits
    g = np.random.default_rng(2)
    shuffled = []
    for level in levels:
        perm = g.permutation(level["coords"].shape[0])
        shuffled.append(dict(level, coords=level["coords"][perm], feats=level["feats"][perm]))
    with torch.no_grad():
        again = pool(boxes, as_levels(shuffled, pool.strides, "cuda"))
    assert torch.equal(got, again)


def test_native_query_and_pool_replay_in_a_captured_graph():
    """One level's query + first-layer products + pooling captured as one linear chain: a host read of the row count would fail the
    capture; the replay on OTHER boxes and another live count equals the eager result on them."""
    from vision3d_amd.detector.voxel_roi_pool import voxel_pool_pair, voxel_query
    from vision3d_amd.pointnet2.pointnet2_utils import linear_rows
    pool, levels, rois = _module_case()
    level = levels[0]
    lv = _device_level(level)
    feats = lv.features
    scale, offset = pool.level_geometry(0)
    w1f, wx, b1, w2, b2 = pool._folded(0)
    boxes = dev(rois)

    def run(out):
        pts = pool.grid_points(boxes).reshape(-1, 3)
        idx, _ = voxel_query(pts, 3 * 27, lv, scale, offset, pool.ranges[0], pool.radii[0], pool.nsample)
        voxel_pool_pair(linear_rows(feats, w1f), lv.coords, pts, idx, scale, offset, wx, b1, w2, b2, out)
        return out

    out = torch.zeros((2 * 3 * 27, 32), device="cuda")
    with torch.no_grad():
        run(out)  # (warm-up: caches, workspaces)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            run(out)
        other = dev(R.make_rois(6, level))
        boxes.copy_(other)
        lv.n.fill_(level["coords"].shape[0] - 50)
        graph.replay()
        torch.cuda.synchronize()
        replayed = out.clone()
        eager = run(torch.zeros_like(out))
    assert bool(replayed.ne(0).any()) and torch.equal(replayed, eager)


# ---- PV_RCNN
def _model_cfg():
    return pool_cfg(GRID=3)


def _pv_rcnn(cfg, seed):
    from vision3d_amd.detector import PV_RCNN
    torch.manual_seed(seed)
    model = PV_RCNN(cfg).cuda().eval()
    with torch.no_grad():  # scores that straddle the class threshold and overlapping boxes, as tests/test_gpu_pointops.py sets them
        model.proposal_layer.conv_cls.bias.fill_(0.3)
        model.refinement_layer.mlp[-1].bias[7] = 0.2
        model.refinement_layer.mlp[-1].weight.mul_(30.0)
        if model.voxel_pool:
            randomize(model.voxel_roi_pool, 3)
    return model


def _frame(cfg, seed=40, n_points=16384):
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    anchors = AnchorGenerator(cfg).anchors.cuda()
    cloud = synth.make_cloud(seed, n_points)
    return lambda: Preprocessor(cfg, seed=0)(dict(points=[cloud], anchors=anchors))


def test_pv_rcnn_with_voxel_pooling_inference_and_its_pipelined_form():
    """Stage 1 of an untrained model scores every anchor alike (BEV features of ~1e-7 under the initialisation's weights), so its
    top-k is the first row of the map, outside the sensor's field of view, where every grid point is empty and the pooled features
    are exact zeros.  The RoIs are therefore set around the frame's objects (synth.jitter_rois, as the train-step tests do); stage 1,
    the pooling, the refinement head and the native tail run as in any frame."""
    cfg = _model_cfg()
    model = _pv_rcnn(cfg, 21)
    make = _frame(cfg)
    n = cfg.NUM_CLASSES * cfg.PROPOSAL.TOPK
    rois = torch.from_numpy(synth.jitter_rois(synth.make_gt_boxes(40), n, np.random.default_rng(123))[None]).cuda()
    model.stage1_proposals = lambda it: (rois, torch.ones(rois.shape[:2], device=rois.device), torch.zeros(n, dtype=torch.long, device=rois.device))
    with torch.no_grad():
        item = make()
        dets = [t.clone() for t in model.inference(item)]
        assert "keypoints" not in item and item["pooled_features"].shape == (1, n, 256) and item["boxes_refined"].shape == (1, n, 7)
        assert 0 < len(dets[0]) <= n and dets[0].shape[1] == 7 and bool(torch.isfinite(dets[0]).all())
        assert float(item["pooled_features"].std()) > 1e-4  # (the RoIs pool different voxels)
        # the torch statements of the pooling inside the same model
        native_pooled = item["pooled_features"].clone()
        model.voxel_roi_pool.native = False
        item_t = make()
        model.inference(item_t)
        model.voxel_roi_pool.native = True
        torch.testing.assert_close(native_pooled, item_t["pooled_features"], rtol=1e-4, atol=1e-5 * float(native_pooled.abs().max()))
        st = model.inference_begin(make(), 0)
        got = model.inference_collect(model.inference_end(st))
    assert len(got) == len(dets)
    for a, b in zip(got, dets):
        assert torch.equal(a, b)
    # the unpatched chain once: the model's own native top-k boxes into the pooling and the native tail.  The pooled features may
    # all be zero there (see above); the result has the right shapes and is finite, and the pipelined form equals it
    del model.stage1_proposals
    with torch.no_grad():
        item = make()
        own = [t.clone() for t in model.inference(item)]
        assert item["proposals"].shape == (1, n, 7) and item["pooled_features"].shape == (1, n, 256) and item["R_reg"].shape == (1, n, 7)
        assert all(bool(torch.isfinite(item[k]).all()) for k in ("proposals", "pooled_features", "R_reg", "R_cls", "boxes_refined"))
        assert own[0].shape[1:] == (7,) and len(own[0]) == len(own[1]) == len(own[2]) == len(own[3]) <= n and bool(torch.isfinite(own[0]).all())
        piped = model.inference_collect(model.inference_end(model.inference_begin(make(), 1)))
    for a, b in zip(piped, own):
        assert torch.equal(a, b)


def test_pv_rcnn_with_voxel_pooling_train_step():
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    from vision3d_amd.detector import PV_RCNN, RefinementLoss
    cfg = _model_cfg()
    gt = torch.from_numpy(synth.make_gt_boxes(0))
    item = Preprocessor(cfg, seed=0)(dict(points=synth.make_kitti_batch(1)))
    item["anchors"] = AnchorGenerator(cfg).anchors.cuda()
    item["boxes"], item["class_idx"] = [gt], [torch.zeros(len(gt), dtype=torch.long)]
    rng = np.random.default_rng(123)
    topk = cfg.PROPOSAL.TOPK
    rois = torch.from_numpy(synth.jitter_rois(gt.numpy(), topk, rng)[None]).cuda()
    item["refine_draws"] = torch.from_numpy(rng.random((1, topk)).astype(np.float32)).cuda()
    torch.manual_seed(0)
    model = PV_RCNN(cfg).cuda().train()
    model.stage1_proposals = lambda it: (rois, torch.ones(rois.shape[:2], device=rois.device), torch.zeros(topk, dtype=torch.long, device=rois.device))
    out = model.train_forward(dict(item))
    assert out["pooled_features"].requires_grad and out["R_reg"].shape == (1, topk, 7)
    RefinementLoss(cfg)(out)["loss"].backward()
    for name, p in model.voxel_roi_pool.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert any(bool(p.grad.ne(0).any()) for p in model.voxel_roi_pool.parameters())
    first = next(model.cnn.parameters())
    assert first.grad is not None and bool(torch.isfinite(first.grad).all())  # the backbone learns from stage 2 through the levels


def test_pv_rcnn_disabled_equals_a_configuration_without_the_key():
    """ENABLED = False against a configuration without the key: the switch itself changes nothing.  Both sides run the code as it
    stands, so this cannot show a change against earlier versions of the default path -- that guarantee is carried by the existing
    PV_RCNN tests (tests/test_gpu_pointops.py, test_gpu_keypoint_weighting.py, test_gpu_keypoint_sampling.py, test_gpu_pvrcnn_train.py),
    which compare the default model against its op-by-op statements and the float64 restatements."""
    make = _frame(second_car_cfg())
    outs = []
    for drop in (True, False):
        cfg = second_car_cfg()
        if drop:
            del cfg["VOXELPOOL"]
        model = _pv_rcnn(cfg, 21)
        model.cnn.pad_generator = torch.Generator(device="cuda").manual_seed(23)
        n = cfg.NUM_CLASSES * cfg.PROPOSAL.TOPK
        samples = torch.rand((1, n, cfg.GRIDPOOL.NUM_GRIDPOINTS, 3), generator=torch.Generator().manual_seed(22)).cuda()
        with torch.no_grad():
            item = make()
            dets = model.inference(item, samples)
        outs.append([t.clone() for t in dets] + [item["keypoint_features"].clone(), item["pooled_features"].clone(), item["R_reg"].clone(),
                                                 item["R_cls"].clone()])
    assert len(outs[0][0]) > 0
    for a, b in zip(*outs):
        assert torch.equal(a, b)
