"""GPU: VectorPool aggregation (csrc/vector_pool.hip, detector/vector_pool.py) -- the native search exactly against the float64
restatement (tests/vector_pool_ref.py) on the seeded cases (tests/vector_pool_cases.py), its weights within 16 ulp, the embedding and
the module against float64 under the bar of the torch float32 statements' own error, the over-limit fallback, a training step, and
PV_RCNN with the aggregation enabled (inference, the pipelined form, a train step) and disabled (outputs unchanged)."""
import functools

import numpy as np
import pytest
import torch

import vector_pool_cases as C
import vector_pool_ref as R
from gpu_util import FP32_CLASS_FLOOR, assert_features_close, assert_fp32_class, dev, strict_rel_err
from test_host_vector_pool import small_module, vp_cfg
from vision3d_amd import synth
from vision3d_amd.core.config import second_car_cfg

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(kind, g):
    xyz, q = C.make_case(kind)
    voxels, radius = C.GROUPS[g]
    return (xyz, q) + R.query(xyz, q, voxels, radius)


def _native(xyz, q, voxels, radius):
    from vision3d_amd.detector.vector_pool import vector_pool_query
    idx, w = vector_pool_query(dev(xyz), dev(q), voxels, radius)
    return idx.cpu().numpy().astype(np.int64), w.cpu().numpy()


def _points(xyz, idx):
    """Coordinates of the rows idx (B, M, nv, 3) refers to, as bits; missing neighbours read as all ones."""
    bits = np.ascontiguousarray(xyz).view(np.uint32)
    out = bits[np.arange(xyz.shape[0])[:, None, None, None], np.maximum(idx, 0)]
    return np.where((idx >= 0)[..., None], out, np.uint32(0xFFFFFFFF))


@pytest.mark.parametrize("g", range(len(C.GROUPS)))
@pytest.mark.parametrize("kind", C.KINDS)
def test_query_equals_the_restatement_exactly(kind, g):
    """idx (the -1 patterns included) on every decidable centre (at most 2 % are left out); no index refers to a duplicate's higher
    row; permuted rows give the same points; more appended duplicates change nothing; two runs are bit-equal; N = 317 is no multiple
    of 64.  The weights: two subtractions, a sum of squares, a square root, a reciprocal and a normalisation, about eight float32
    roundings -- bar 16 ulp of the value.  Largest observed on an MI355X over the eight cases: 3.45 ulp."""
    voxels, radius = C.GROUPS[g]
    xyz, q, want, _, und = _reference(kind, g)
    assert und.mean() <= 0.02
    idx, w = _native(xyz, q, voxels, radius)
    keep = ~und
    assert idx.min() >= -1 and idx.max() < xyz.shape[1]
    np.testing.assert_array_equal(idx[keep], want[keep])
    canon = np.stack([R.canonical(f) for f in xyz])
    frames = np.broadcast_to(np.arange(C.B)[:, None, None, None], idx.shape)
    assert (canon[frames[idx >= 0], idx[idx >= 0]] == idx[idx >= 0]).all(), "a duplicate's higher row was returned"
    # weights against float64 on the native neighbours (every centre)
    w64 = R.weights(xyz, q, voxels, radius, idx)
    ulps = np.abs(w.astype(np.float64) - w64) / np.spacing(np.maximum(np.abs(w64), 1e-30).astype(np.float32)).astype(np.float64)
    print(f"[vector pool query {kind} {voxels} R={radius}] undecidable {und.mean():.4f}, largest weight error {ulps[idx >= 0].max():.2f} ulp")
    assert (w[idx < 0] == 0.0).all() and ulps[idx >= 0].max() <= 16.0
    # two runs
    idx2, w2 = _native(xyz, q, voxels, radius)
    assert np.array_equal(idx, idx2) and np.array_equal(w.view(np.uint32), w2.view(np.uint32))
    # permuted rows: the same points and weights
    rng = np.random.default_rng(9)
    perm = np.stack([rng.permutation(xyz.shape[1]) for _ in range(C.B)])
    xyz_p = np.stack([f[p] for f, p in zip(xyz, perm)])
    idx_p, w_p = _native(xyz_p, q, voxels, radius)
    assert np.array_equal(_points(xyz_p, idx_p)[keep], _points(xyz, idx)[keep])
    assert np.array_equal(w_p[keep].view(np.uint32), w[keep].view(np.uint32))
    mapped = np.where(idx_p >= 0, perm[frames, np.maximum(idx_p, 0)], -1)  # (a duplicated point may come back through its twin)
    sel = keep[..., None] & (idx >= 0)
    assert (mapped[sel] >= 0).all() and (canon[frames[sel], mapped[sel]] == idx[sel]).all()
    # more duplicates behind the rows: nothing changes
    more = np.concatenate([xyz, np.stack([f[rng.integers(0, f.shape[0], 40)] for f in xyz])], 1)
    idx_m, w_m = _native(more, q, voxels, radius)
    assert np.array_equal(idx_m, idx) and np.array_equal(w_m.view(np.uint32), w.view(np.uint32))


def test_query_of_a_database_elsewhere_and_of_an_empty_one():
    xyz, q = C.make_case("uniform")
    far = q.copy()
    far[0] += np.array([100.0, -60.0, 0.0], np.float32)
    idx, w = _native(xyz, far, (3, 3, 3), 0.8)
    own, own_w = _native(xyz, q, (3, 3, 3), 0.8)
    assert (idx[0] == -1).all() and (w[0].view(np.uint32) == 0).all()
    assert np.array_equal(idx[1], own[1]) and np.array_equal(w[1], own_w[1]) and (own[1] >= 0).any()
    idx, w = _native(np.zeros((2, 0, 3), np.float32), q, (2, 2, 2), 0.4)
    assert idx.shape == (2, C.M, 8, 3) and (idx == -1).all() and (w.view(np.uint32) == 0).all()
    # rows that are not finite are never neighbours
    bad = xyz.copy()
    bad[:, ::3] = np.nan
    bad[:, 1::3, 0] = np.inf
    idx, _ = _native(bad, q, (3, 3, 3), 0.8)
    assert ((idx % 3 == 2) | (idx == -1)).all() and (idx >= 0).any()


def test_query_of_two_corner_clusters_and_an_empty_frame():
    """The scan over the cells of a frame's grid (16 384 cells, 17 to each of the build's 1 024 threads) where a base can go wrong: the support rows
    in two clusters at opposite corners of their bounds, 127.5 reaches apart along x and y, so that the grid has 128 x 128 cells of
    which the first and the last are occupied -- the last thread's base is every row before its own --; the second frame holds no
    finite row.  idx exactly against the restatement on the decidable centres; the empty frame finds nothing."""
    voxels, radius = (3, 3, 3), 0.4
    reach = radius * (2.0 - 1.0 / 3.0) * (1.0 + 1e-5) + 1e-3  # the cell edge vector_pool.hip derives from (voxels, radius)
    span = 127.5 * reach
    rng = np.random.default_rng(5)
    n = C.N_ROWS + C.N_DUP
    lo = np.array([20.0, -3.0, -2.0])
    rows = lo + rng.random((n, 3)) * np.array([0.5, 0.5, 1.2])
    rows[n // 2:, :2] += span - 0.5
    rows[0, :2], rows[-1, :2] = lo[:2], lo[:2] + span  # the corners of the bounds
    rows[-C.N_DUP:-1] = rows[rng.integers(0, C.N_ROWS, C.N_DUP - 1)]
    xyz = np.stack([rows, np.full((n, 3), np.nan)]).astype(np.float32)
    q = rows[rng.integers(0, n, (C.B, C.M))] + rng.uniform(-0.3, 0.3, (C.B, C.M, 3))
    q = q.astype(np.float32)
    want, _, und = R.query(xyz[:1], q[:1], voxels, radius)
    assert und.mean() <= 0.02
    idx, w = _native(xyz, q, voxels, radius)
    np.testing.assert_array_equal(idx[:1][~und], want[~und])
    for half in (slice(0, n // 2), slice(n // 2, n)):  # both corners are found
        assert ((idx[0] >= half.start) & (idx[0] < half.stop)).any()
    assert (idx[1] == -1).all() and (w[1].view(np.uint32) == 0).all()


# ---- the search over the shared cell grid (csrc/cell_grid.hip): every instantiation of the build, the growth loop, the single cell
def _assert_equals_the_restatement(xyz, q, voxels, radius):
    """As test_query_equals_the_restatement_exactly: idx (the -1 patterns included) on every decidable centre, no index of a
    duplicate's higher row, the weights within 16 ulp of float64 on the native neighbours, two runs bit-equal."""
    want, _, und = R.query(xyz, q, voxels, radius)
    assert und.mean() <= C.GRID_CAP
    idx, w = _native(xyz, q, voxels, radius)
    assert idx.min() >= -1 and idx.max() < xyz.shape[1]
    np.testing.assert_array_equal(idx[~und], want[~und])
    canon = np.stack([R.canonical(f) for f in xyz])
    frames = np.broadcast_to(np.arange(xyz.shape[0])[:, None, None, None], idx.shape)
    assert (canon[frames[idx >= 0], idx[idx >= 0]] == idx[idx >= 0]).all(), "a duplicate's higher row was returned"
    w64 = R.weights(xyz, q, voxels, radius, idx)
    ulps = np.abs(w.astype(np.float64) - w64) / np.spacing(np.maximum(np.abs(w64), 1e-30).astype(np.float32)).astype(np.float64)
    found = np.bincount((idx >= 0).sum(-1).reshape(-1), minlength=4).tolist()
    print(f"[vector pool grid N={xyz.shape[1]} {voxels} R={radius}] neighbours found 0/1/2/3: {found}, undecidable {und.mean():.4f}, "
          f"largest weight error {ulps[idx >= 0].max() if (idx >= 0).any() else 0.0:.2f} ulp")
    assert (w[idx < 0] == 0.0).all() and (not (idx >= 0).any() or ulps[idx >= 0].max() <= 16.0)
    idx2, w2 = _native(xyz, q, voxels, radius)
    assert np.array_equal(idx, idx2) and np.array_equal(w.view(np.uint32), w2.view(np.uint32))
    return idx


@pytest.mark.parametrize("voxels,radius", C.GRID_GROUPS)
@pytest.mark.parametrize("n", C.GRID_BUILD_N)
def test_query_through_every_instantiation_of_the_grid_build(n, voxels, radius):
    """The build keeps 4, 12 or 20 points per thread in registers or reads them again (more than 20 480): the last size of the first
    kind, and the first size of each of the others."""
    idx = _assert_equals_the_restatement(*C.grid_build_case(n), voxels, radius)
    assert (idx[0] >= 0).any() and (idx[1] >= 0).any()


def test_query_where_the_grid_has_to_grow():
    xyz, q = C.grid_growth_case()
    idx = _assert_equals_the_restatement(xyz, q, (2, 2, 2), 0.2)
    assert ((idx >= 0).sum(-1) == 3).any()


@pytest.mark.parametrize("kind", C.GRID_SINGLE_KINDS)
def test_query_of_a_single_cell(kind):
    xyz, q = C.grid_single_cell_case(kind)
    idx = _assert_equals_the_restatement(xyz, q, (2, 2, 2), 0.2)
    assert (idx[..., 0] >= 0).any()
    if kind == "equal":  # one canonical row per centre at most
        assert (idx[..., 0] <= 0).all() and (idx[..., 1:] == -1).all()


@pytest.mark.parametrize("cr,cl,g", [(1, 16, 0), (4, 32, 1), (32, 16, 2), (32, 32, 3), (4, 16, 3), (1, 32, 2)])
def test_embed_against_float64(cr, cl, g):
    """Reduction + embedding of one group on the native neighbours against the float64 restatement on the same neighbours, under
    gpu_util's strict rule: 2e-4 or twice the error the torch float32 statements show against float64 on the same inputs (a K <= 41
    dot product summed in another order, the BatchNorm folded into the weights instead of applied behind the product).  The block is
    written at column 16 of a wider matrix whose other columns keep their sentinel; empty sub-voxels read exactly relu(shift)."""
    from vision3d_amd.detector.vector_pool import vector_pool_embed, vector_pool_query, vector_pool_reduce
    voxels, radius = C.GROUPS[g]
    mod = small_module(c_in=2 * cr, reduced=cr, local=cl, groups=[C.GROUPS[g]], seed=11 + cr + cl).cuda()
    group = mod.groups[0]
    xyz, q = C.make_case("uniform" if g % 2 else "lattice")
    feat = C.make_features(2 * cr)
    x, qq, f = dev(xyz), dev(q), dev(feat)
    with torch.no_grad():
        idx, w = vector_pool_query(x, qq, voxels, radius)
        fr = vector_pool_reduce(f, cr)
        assert torch.equal(fr, mod.reduce_torch(f))  # (one float32 add per value in both)
        (w_local, shift, _), = mod._folded()[0]
        width = group.nv * cl
        wide = torch.full((C.B * C.M, width + 32), -7.0, device="cuda")
        vector_pool_embed(fr, x, qq, idx, w, voxels, radius, w_local, shift, wide[:, 16:16 + width])
        assert bool((wide[:, :16] == -7.0).all()) and bool((wide[:, 16 + width:] == -7.0).all()), "columns outside the block changed"
        got = wide[:, 16:16 + width].cpu().numpy()
        own = mod.embed_torch(fr, x, qq, idx.long(), w, group).cpu().numpy()
        wide2 = torch.full_like(wide, -7.0)
        vector_pool_embed(fr, x, qq, idx, w, voxels, radius, w_local, shift, wide2[:, 16:16 + width])
        assert torch.equal(wide, wide2), "two runs differ"
    state = {k: v.cpu().numpy() for k, v in mod.state_dict().items()}
    ii = idx.cpu().numpy().astype(np.int64)
    want = R.embed(R.rows(R.reduce(feat, cr), xyz, q, voxels, radius, ii, R.weights(xyz, q, voxels, radius, ii)), state, "groups.0.")
    print(f"[vector pool embed Cr={cr} CL={cl} {voxels}] strict rel err native {strict_rel_err(got, want):.3e}, torch fp32 {strict_rel_err(own, want):.3e}")
    assert float(np.abs(want).max()) > 0.1
    assert_fp32_class(got, own, f"embedded rows Cr={cr} CL={cl}", ref64=want, own_factor=2.0)
    empty = (ii < 0).all(-1).reshape(C.B * C.M, group.nv)
    assert empty.any() and not empty.all()
    relu_shift = np.broadcast_to(torch.relu(shift).cpu().numpy().reshape(1, group.nv, cl), (C.B * C.M, group.nv, cl))
    assert np.array_equal(got.reshape(-1, group.nv, cl)[empty], relu_shift[empty])


def _module_neighbours(mod, xyz, q):
    from vision3d_amd.detector.vector_pool import vector_pool_query
    return [vector_pool_query(dev(xyz), dev(q), g.voxels, g.radius)[0].cpu().numpy() for g in mod.groups]


@pytest.mark.parametrize("kind", C.KINDS)
def test_module_native_against_torch_and_float64(kind):
    mod = small_module().cuda()
    xyz, q = C.make_case(kind)
    feat = C.make_features(8)
    state = {k: v.cpu().numpy() for k, v in mod.state_dict().items()}
    x, qq, f = dev(xyz), dev(q), dev(feat)
    want, _ = R.module(state, xyz, feat, q, 4, C.GROUPS[:2], neighbours=_module_neighbours(mod, xyz, q))
    with torch.no_grad():
        assert mod.native_ok(x, f, qq)
        _, got = mod(x, None, qq, features_pm=f)
        own = mod.forward_torch(x, f, qq)
        _, again = mod(x, f.transpose(1, 2).contiguous(), qq)  # channel-major features
    assert torch.is_grad_enabled() and not mod.native_ok(x, f, qq)  # under autograd: the torch statements
    assert got.shape == (C.B, 24, C.M) and torch.equal(got, again)
    print(f"[vector pool module {kind}] strict rel err native {strict_rel_err(got.cpu().numpy(), want):.3e}, "
          f"torch fp32 {strict_rel_err(own.cpu().numpy(), want):.3e}")
    assert_fp32_class(got.cpu().numpy(), own.cpu().numpy(), "module output", ref64=want, own_factor=2.0)
    # native = False: the search in torch statements too -- the same neighbours on the decidable queries
    want_own, und = R.module(state, xyz, feat, q, 4, C.GROUPS[:2])
    mod.native = False
    with torch.no_grad():
        assert not mod.native_ok(x, f, qq)
        _, plain = mod(x, None, qq, features_pm=f)
    keep = ~und
    assert_fp32_class(got.cpu().numpy().transpose(0, 2, 1)[keep], plain.cpu().numpy().transpose(0, 2, 1)[keep], "native against native = False",
                      ref64=want_own.transpose(0, 2, 1)[keep], own_factor=2.0)


def test_over_limit_takes_the_torch_path():
    groups = [((4, 1, 1), 0.4)]
    mod = small_module(groups=groups).cuda()
    xyz, q = C.make_case("uniform")
    feat = C.make_features(8)
    x, qq, f = dev(xyz), dev(q), dev(feat)
    state = {k: v.cpu().numpy() for k, v in mod.state_dict().items()}
    want, und = R.module(state, xyz, feat, q, 4, groups)
    with torch.no_grad():
        assert not mod.native_ok(x, f, qq)
        _, got = mod(x, None, qq, features_pm=f)
        _, cpu = mod.cpu()(torch.from_numpy(xyz), None, torch.from_numpy(q), features_pm=torch.from_numpy(feat))
    keep = ~und
    assert keep.mean() > 0.9
    assert_fp32_class(got.cpu().numpy().transpose(0, 2, 1)[keep], cpu.numpy().transpose(0, 2, 1)[keep], "over-limit module", ref64=want.transpose(0, 2, 1)[keep],
                      own_factor=2.0)


def test_training_step_through_the_module():
    """Train mode: the native search gives the neighbours, the rest is torch under autograd.  Gradients reach every parameter and the
    support features; output and feature gradient agree with the pure torch path (native = False) under the float32-class bar, the
    float64 yardstick being the same module in double on the CPU."""
    groups = [C.GROUPS[0], C.GROUPS[2]]  # (no undecidable centre in the uniform case: tests/test_host_vector_pool.py prints them)
    xyz, q = C.make_case("uniform")
    assert not any(R.query(xyz, q, v, r)[2].any() for v, r in groups)
    feat = C.make_features(8)
    outs = []
    for native, device, dtype in ((True, "cuda", torch.float32), (False, "cuda", torch.float32), (False, "cpu", torch.float64)):
        mod = small_module(groups=groups).to(device, dtype).train()
        mod.native = native
        f = torch.from_numpy(feat).to(device, dtype).requires_grad_()
        _, out = mod(torch.from_numpy(xyz).to(device), None, torch.from_numpy(q).to(device), features_pm=f)
        assert out.requires_grad
        out.square().sum().backward()
        for name, p in mod.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.ne(0).any()), name
        assert bool(torch.isfinite(f.grad).all()) and bool(f.grad.ne(0).any())
        outs.append((out.detach().cpu().numpy(), f.grad.cpu().numpy(), mod.groups[1].local_weight.grad.cpu().numpy()))
    for k, what in enumerate(("output", "feature gradient", "local weight gradient")):
        assert_fp32_class(outs[0][k], outs[1][k], f"training {what}", ref64=outs[2][k], own_factor=2.0)


# ---- PV_RCNN
def _model_cfg():
    cfg = vp_cfg()
    cfg.NUM_KEYPOINTS = 256  # (the torch statements of the search hold M * nv * N distances)
    return cfg


def _pv_rcnn(cfg, seed):
    from vision3d_amd.detector import PV_RCNN
    from vision3d_amd.detector.vector_pool import VectorPoolAggregationMSG
    torch.manual_seed(seed)
    model = PV_RCNN(cfg).cuda().eval()
    with torch.no_grad():  # scores that straddle the class threshold and overlapping boxes, as tests/test_gpu_pointops.py sets them
        model.proposal_layer.conv_cls.bias.fill_(0.3)
        model.refinement_layer.mlp[-1].bias[7] = 0.2
        model.refinement_layer.mlp[-1].weight.mul_(30.0)
    for k, m in enumerate(mod for mod in model.modules() if isinstance(mod, VectorPoolAggregationMSG)):
        C.randomize(m, 30 + k)
    return model


def _frame(cfg, seed=40, n_points=16384):
    from vision3d_amd.core import AnchorGenerator, Preprocessor
    anchors = AnchorGenerator(cfg).anchors.cuda()
    cloud = synth.make_cloud(seed, n_points)
    return lambda: Preprocessor(cfg, seed=0)(dict(points=[cloud], anchors=anchors))


def test_pv_rcnn_with_vector_pool_inference_and_its_pipelined_form():
    """An untrained stage 1 proposes the map's empty edge row, so the RoIs are set around the frame's objects (synth.jitter_rois, as the
    voxel RoI pooling tests do); stage 1, the keypoint features, RoI-grid pooling, the refinement head and the native tail run as in
    any frame."""
    from vision3d_amd.detector.vector_pool import VectorPoolAggregationMSG
    cfg = _model_cfg()
    model = _pv_rcnn(cfg, 21)
    make = _frame(cfg)
    n = cfg.NUM_CLASSES * cfg.PROPOSAL.TOPK
    rois = torch.from_numpy(synth.jitter_rois(synth.make_gt_boxes(40), n, np.random.default_rng(123))[None]).cuda()
    model.stage1_proposals = lambda it: (rois, torch.ones(rois.shape[:2], device=rois.device), torch.zeros(n, dtype=torch.long, device=rois.device))
    samples = torch.rand((1, n, cfg.GRIDPOOL.NUM_GRIDPOINTS, 3), generator=torch.Generator().manual_seed(22)).cuda()
    with torch.no_grad():
        item = make()
        model.cnn.pad_generator = torch.Generator(device="cuda").manual_seed(23)
        dets = [t.clone() for t in model.inference(item, samples)]
        assert item["keypoint_features"].shape == (1, 512, 256) and item["pooled_features"].shape == (1, n, 256)
        assert 0 < len(dets[0]) <= n and dets[0].shape[1] == 7 and bool(torch.isfinite(dets[0]).all())
        assert float(item["pooled_features"].std()) > 1e-4 and float(item["keypoint_features"][:, :384].std()) > 1e-3
        native = [item["keypoint_features"].clone(), item["pooled_features"].clone()]
        # the torch statements of the aggregation (the search included) inside the same model
        VectorPoolAggregationMSG.native = False
        try:
            item_t = make()
            model.cnn.pad_generator = torch.Generator(device="cuda").manual_seed(23)
            model.inference(item_t, samples)
        finally:
            VectorPoolAggregationMSG.native = True
        for a, b, what in zip(native, (item_t["keypoint_features"], item_t["pooled_features"]), ("keypoint features", "pooled features")):
            assert_features_close(a.cpu().numpy(), b.cpu().numpy(), what, floor=FP32_CLASS_FLOOR)
        model.cnn.pad_generator = torch.Generator(device="cuda").manual_seed(23)
        st = model.inference_begin(make(), 0)
        got = model.inference_collect(model.inference_end(st, samples))
    assert len(got) == len(dets)
    for a, b in zip(got, dets):
        assert torch.equal(a, b)


def test_pv_rcnn_with_vector_pool_train_step():
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
    assert out["pooled_features"].requires_grad and out["R_reg"].shape == (1, topk, 7) and out["keypoint_features"].shape == (1, 512, 256)
    RefinementLoss(cfg)(out)["loss"].backward()
    for part in (model.pnets, model.roi_grid_pool.pnet):
        for name, p in part.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        assert any(bool(p.grad.ne(0).any()) for p in part.parameters())
    first = next(model.cnn.parameters())
    assert first.grad is not None and bool(torch.isfinite(first.grad).all())  # the backbone learns from stage 2 through the levels


def test_pv_rcnn_disabled_equals_a_configuration_without_the_key():
    """ENABLED = False against a configuration without the key: the switch itself changes nothing.  Both sides run the code as it
    stands; that the default path equals earlier versions is carried by the existing PV_RCNN tests, which compare the default model
    against its op-by-op statements and the float64 restatements."""
    make = _frame(second_car_cfg())
    outs = []
    for drop in (True, False):
        cfg = second_car_cfg()
        if drop:
            del cfg["VECTORPOOL"]
        from vision3d_amd.detector import PV_RCNN
        torch.manual_seed(21)
        model = PV_RCNN(cfg).cuda().eval()
        with torch.no_grad():
            model.proposal_layer.conv_cls.bias.fill_(0.3)
            model.refinement_layer.mlp[-1].bias[7] = 0.2
            model.refinement_layer.mlp[-1].weight.mul_(30.0)
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
