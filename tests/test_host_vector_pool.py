"""CPU: VectorPool aggregation (vision3d_amd/detector/vector_pool.py) -- the float64 restatement (tests/vector_pool_ref.py) on hand
cases, `query_torch` and the module's torch path against it on the seeded cases, the configuration errors, and the model's
state_dict with the key off (today's list: tests/golden/pv_rcnn_state_dict_keys.txt) and on."""
import os

import numpy as np
import pytest
import torch

import vector_pool_cases as C
import vector_pool_ref as R
from vision3d_amd.core.config import second_car_cfg

HERE = os.path.dirname(os.path.abspath(__file__))


def vp_cfg(**kw):
    cfg = second_car_cfg()
    cfg.VECTORPOOL.merge_from_dict(dict(ENABLED=True, **kw))
    return cfg


def small_module(c_in=8, reduced=4, local=16, groups=C.GROUPS[:2], post=(32, 16), msg_post=(24,), seed=5):
    from vision3d_amd.detector.vector_pool import VectorPoolAggregationMSG
    mod = VectorPoolAggregationMSG(c_in, reduced, local, [dict(VOXELS=v, RADIUS=r, POST=list(post)) for v, r in groups], list(msg_post))
    return C.randomize(mod, seed).eval()


# ---- the restatement on hand cases
def test_offsets_and_centres():
    off = R.offsets32((2, 1, 3), 0.6)
    assert off.shape == (6, 3) and off.dtype == np.float32
    np.testing.assert_array_equal(off[0], np.array([-0.3, 0.0, -0.4], np.float64).astype(np.float32))
    np.testing.assert_array_equal(off[5], np.array([0.3, 0.0, 0.4], np.float64).astype(np.float32))
    from vision3d_amd.detector.vector_pool import subvoxel_offsets
    for voxels, radius in C.GROUPS:
        np.testing.assert_array_equal(subvoxel_offsets(voxels, radius).numpy(), R.offsets32(voxels, radius))


def test_order_duplicates_and_missing_neighbours():
    """One sub-voxel (centre = query): rows by ascending (d^2, row); a bit-equal duplicate takes no slot and never shows; an exact
    tie of distinct rows goes to the lower row; strict radius."""
    q = np.zeros((1, 1, 3), np.float32)
    xyz = np.array([[[0.5, 0, 0], [0.25, 0, 0], [0.25, 0, 0], [-0.25, 0, 0], [0, 0.75, 0], [0, 0, 1.0]]], np.float32)
    idx, w, und = R.query(xyz, q, (1, 1, 1), 1.0)
    assert idx[0, 0, 0].tolist() == [1, 3, 0] and und[0, 0, 0]  # (rows 1 and 3 tie exactly; row 5 lies ON the radius)
    u = np.array([4.0, 4.0, 2.0])
    np.testing.assert_allclose(w[0, 0, 0], u / u.sum(), rtol=1e-7)
    idx, w, _ = R.query(xyz[:, [4, 5]], q, (1, 1, 1), 1.0)
    assert idx[0, 0, 0].tolist() == [0, -1, -1] and w[0, 0, 0].tolist() == [1.0, 0.0, 0.0]
    idx, w, _ = R.query(xyz[:, [5]], q, (1, 1, 1), 1.0)
    assert idx[0, 0, 0].tolist() == [-1, -1, -1] and not w.any()
    # rows of another frame are not seen
    idx, _, _ = R.query(np.concatenate([xyz + 50, xyz]), np.zeros((2, 1, 3), np.float32), (1, 1, 1), 1.0)
    assert (idx[0] == -1).all() and idx[1, 0, 0].tolist() == [1, 3, 0]


def test_rows_of_an_empty_subvoxel_are_zero_and_embed_to_relu_of_the_shift():
    mod = small_module(groups=[((2, 2, 2), 0.2)])
    state = {k: v.numpy() for k, v in mod.state_dict().items()}
    xyz, q = C.make_case("uniform")
    idx, w, _ = R.query(xyz, q, (2, 2, 2), 0.2)
    fr = R.reduce(C.make_features(8), 4)
    rows = R.rows(fr, xyz, q, (2, 2, 2), 0.2, idx, w)
    empty = (idx < 0).all(-1)
    assert empty.any() and not rows[empty].any()
    out = R.embed(rows, state, "groups.0.").reshape(C.B, C.M, 8, 16)
    g, beta = state["groups.0.local_bn.weight"].astype(np.float64), state["groups.0.local_bn.bias"].astype(np.float64)
    shift = beta - state["groups.0.local_bn.running_mean"] / np.sqrt(state["groups.0.local_bn.running_var"].astype(np.float64) + 1e-3) * g
    want = np.broadcast_to(np.maximum(shift, 0).reshape(8, 16), out.shape)
    np.testing.assert_allclose(out[empty], want[empty], rtol=1e-12, atol=1e-15)


# ---- the seeded cases
@pytest.mark.parametrize("kind", C.KINDS)
def test_cases_cover_every_neighbour_count(kind):
    xyz, q = C.make_case(kind)
    assert xyz.shape == (C.B, 317, 3) and xyz.dtype == np.float32 and q.shape == (C.B, C.M, 3)
    assert all(len(np.unique(f, axis=0)) < len(f) for f in xyz)  # (the duplicates are there)
    for voxels, radius in C.GROUPS:
        idx, w, und = R.query(xyz, q, voxels, radius)
        counts = np.bincount((idx >= 0).sum(-1).reshape(-1), minlength=4)
        print(f"[{kind} {voxels} R={radius}] centres by neighbour count {counts.tolist()}, undecidable {und.mean():.4f}, "
              f"wholly empty queries {((idx < 0).all((2, 3))).mean():.2f}")
        assert (counts > 0).all() and und.mean() <= 0.02
        canon = np.stack([R.canonical(f) for f in xyz])
        picked = idx[idx >= 0]
        frames = np.broadcast_to(np.arange(C.B)[:, None, None, None], idx.shape)[idx >= 0]
        assert (canon[frames, picked] == picked).all()  # no index refers to a duplicate's higher row


def test_grid_cases_are_decidable_and_shaped_as_stated():
    """The cases of the search over the shared cell grid (tests/test_gpu_vector_pool.py): the restatement alone leaves at most
    GRID_CAP of a case's centres undecided, and each case has the shape its test is about."""
    reach = lambda voxels, radius: radius * (2.0 - 1.0 / max(voxels[:2])) * (1.0 + 1e-5) + 1e-3  # the cell edge vector_pool.hip asks for
    cases = [(f"build N={n}", C.grid_build_case(n), g) for n in C.GRID_BUILD_N for g in C.GRID_GROUPS]
    cases += [("growth", C.grid_growth_case(), ((2, 2, 2), 0.2))]
    cases += [(f"single cell, {k}", C.grid_single_cell_case(k), ((2, 2, 2), 0.2)) for k in C.GRID_SINGLE_KINDS]
    for name, (xyz, q), (voxels, radius) in cases:
        idx, _, und = R.query(xyz, q, voxels, radius)
        counts = np.bincount((idx >= 0).sum(-1).reshape(-1), minlength=4)
        extent = (xyz[:, :, :2].max(1) - xyz[:, :, :2].min(1)).astype(np.float64)
        cells = np.prod(np.floor(extent / reach(voxels, radius)) + 1, axis=1)
        print(f"[{name} {voxels} R={radius}] centres by neighbour count {counts.tolist()}, undecidable {und.mean():.4f}, cells at the first try {cells.tolist()}")
        assert und.mean() <= C.GRID_CAP and (idx >= 0).any()
        assert (np.abs(q[:, :4, None, :] - xyz[:, None, :, :]).max(-1).min(-1) == 0).all()  # (queries on support rows)
        if name == "growth":
            assert (cells > 400000).all() and xyz.shape == (2, 2320, 3) and q.shape == (2, 16, 3)
        elif name.startswith("single"):
            assert (cells == 1).all()
        else:
            assert (cells <= 32768).all() and (cells > 1).all() and q.shape == (2, 8, 3)


@pytest.mark.parametrize("kind", C.KINDS)
def test_query_torch_equals_the_restatement(kind):
    from vision3d_amd.detector import vector_pool as V
    xyz, q = C.make_case(kind)
    for voxels, radius in C.GROUPS + [((4, 1, 1), 0.4)]:
        want, want_w, und = R.query(xyz, q, voxels, radius)
        idx, w = V.query_torch(torch.from_numpy(xyz), torch.from_numpy(q), voxels, radius)
        keep = ~und
        np.testing.assert_array_equal(idx.numpy()[keep], want[keep])
        np.testing.assert_allclose(w.numpy()[keep], want_w[keep], rtol=1e-5, atol=1e-7)
    old = V.QUERY_TORCH_BYTES
    V.QUERY_TORCH_BYTES = 4 * 4 * 317 * 5  # chunks of five queries: the same result
    try:
        again, again_w = V.query_torch(torch.from_numpy(xyz), torch.from_numpy(q), voxels, radius)
    finally:
        V.QUERY_TORCH_BYTES = old
    assert torch.equal(again, idx) and torch.equal(again_w, w)


def test_query_torch_without_support_rows():
    from vision3d_amd.detector.vector_pool import query_torch
    idx, w = query_torch(torch.zeros((2, 0, 3)), torch.zeros((2, 5, 3)), (2, 2, 2), 0.4)
    assert idx.shape == (2, 5, 8, 3) and bool((idx == -1).all()) and not bool(w.any())


@pytest.mark.parametrize("kind", C.KINDS)
def test_torch_module_equals_the_restatement_in_float64(kind):
    """The module's torch path on CPU tensors (query_torch + torch operations) in float64 parameters against the restatement: the
    same neighbours on the decidable queries, then only summation order differs."""
    mod = small_module().double()
    xyz, q = C.make_case(kind)
    feat = C.make_features(8)
    state = {k: v.numpy() for k, v in mod.state_dict().items()}
    want, und = R.module(state, xyz, feat, q, 4, C.GROUPS[:2])
    with torch.no_grad():
        new_xyz, got = mod(torch.from_numpy(xyz), None, torch.from_numpy(q), features_pm=torch.from_numpy(feat).double())
    assert new_xyz.shape == (C.B, C.M, 3) and got.shape == (C.B, 24, C.M) == want.shape and mod.out_channels() == [24]
    keep = ~und
    assert keep.mean() > 0.9 and float(np.abs(want).max()) > 0.1
    # (the float32 weights of query_torch against float64 ones: 1e-6 of a weight)
    np.testing.assert_allclose(got.numpy().transpose(0, 2, 1)[keep], want.transpose(0, 2, 1)[keep], rtol=1e-5, atol=1e-6)
    # channel-major features give the same result
    with torch.no_grad():
        _, again = mod(torch.from_numpy(xyz), torch.from_numpy(feat).double().transpose(1, 2).contiguous(), torch.from_numpy(q))
    assert torch.equal(again, got)


def test_torch_path_is_differentiable_in_features_and_parameters():
    mod = small_module().train()
    xyz, q = C.make_case("uniform")
    feat = torch.from_numpy(C.make_features(8)).requires_grad_()
    _, out = mod(torch.from_numpy(xyz), None, torch.from_numpy(q), features_pm=feat)
    out.square().sum().backward()
    assert bool(torch.isfinite(feat.grad).all()) and bool(feat.grad.ne(0).any())
    for name, p in mod.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.ne(0).any()), name


# ---- configuration
def test_config_errors():
    from vision3d_amd.detector import PV_RCNN
    from vision3d_amd.detector.vector_pool import VectorPoolAggregationMSG
    with pytest.raises(ValueError, match="REDUCED"):
        VectorPoolAggregationMSG(8, 3, 16, [dict(VOXELS=[2, 2, 2], RADIUS=0.4, POST=[16])], [16])
    with pytest.raises(ValueError, match="REDUCED"):
        PV_RCNN(vp_cfg(PSA=dict(REDUCED=[1, 4, 16, 24, 32])))  # 24 does not divide 64
    with pytest.raises(ValueError, match="MLPS_REDUCTION"):
        PV_RCNN(vp_cfg(GRIDPOOL=dict(MSG_POST=[128])))
    with pytest.raises(ValueError, match="one entry per feature source"):
        PV_RCNN(vp_cfg(PSA=dict(REDUCED=[1, 4, 16, 32])))
    both = vp_cfg()
    both.VOXELPOOL.ENABLED = True
    with pytest.raises(ValueError, match="VOXELPOOL"):
        PV_RCNN(both)


def test_disabled_model_has_todays_state_dict_keys():
    from vision3d_amd.detector import PV_RCNN
    with open(os.path.join(HERE, "golden", "pv_rcnn_state_dict_keys.txt")) as f:
        today = f.read().split()
    cfg = second_car_cfg()
    assert cfg.VECTORPOOL.ENABLED is False
    assert list(PV_RCNN(cfg).state_dict().keys()) == today
    del cfg["VECTORPOOL"]  # a configuration written before the key existed
    assert list(PV_RCNN(cfg).state_dict().keys()) == today


def test_enabled_model_keys_and_widths():
    from vision3d_amd.detector import PV_RCNN
    from vision3d_amd.detector.vector_pool import VectorPoolAggregationMSG
    with open(os.path.join(HERE, "golden", "pv_rcnn_state_dict_keys.txt")) as f:
        today = f.read().split()
    model = PV_RCNN(vp_cfg())
    keys = list(model.state_dict().keys())
    assert len(model.pnets) == 5 and all(isinstance(p, VectorPoolAggregationMSG) for p in model.pnets)
    assert isinstance(model.roi_grid_pool.pnet, VectorPoolAggregationMSG)
    assert [sum(p.out_channels()) for p in model.pnets] == [32, 32, 64, 128, 128] and model.roi_grid_pool.pnet.out_channels() == [192]
    assert sum(sum(p.out_channels()) for p in model.pnets) + model.cfg.PROPOSAL.C_IN == 512 == model.roi_grid_pool.pnet.c_in
    assert [g.radius for g in model.pnets[2].groups] == [0.6, 1.2] and [g.radius for g in model.roi_grid_pool.pnet.groups] == [0.8, 1.6]
    assert [p.reduced for p in model.pnets] == [1, 4, 16, 32, 32]
    point_net = lambda k: k.startswith("pnets.") or k.startswith("roi_grid_pool.pnet.")
    assert [k for k in keys if not point_net(k)] == [k for k in today if not point_net(k)]
    new = [k for k in keys if point_net(k)]
    assert "pnets.0.groups.0.local_weight" in new and "pnets.4.groups.1.post.linear_1.weight" in new
    assert "roi_grid_pool.pnet.msg_post.linear_0.weight" in new and "roi_grid_pool.pnet.groups.1.local_bn.running_var" in new
    assert tuple(model.state_dict()["pnets.2.groups.1.local_weight"].shape) == (27, 16 + 9, 32)
    assert not any(".mlps." in k or ".groupers." in k for k in new)
    # predicted keypoint weighting keeps working: it only needs out_channels()
    cfg = vp_cfg()
    cfg.PKW.ENABLED = True
    assert hasattr(PV_RCNN(cfg), "keypoint_weighting")


def test_keypoint_features_are_512_wide_on_cpu_tensors():
    """The op-by-op branch of the keypoint feature extraction carries the module (CPU tensors: its torch path): five small sources."""
    from vision3d_amd.detector import PV_RCNN
    model = PV_RCNN(vp_cfg()).eval()
    g = torch.Generator().manual_seed(3)
    kp = torch.rand((1, 9, 3), generator=g) * 2
    sources = [(torch.rand((1, 40, 3), generator=g) * 2, torch.randn((1, 40, c), generator=g)) for c in (1, 4, 32, 64, 64)]
    assert not model._fused_features_ok(sources, torch.zeros(1, 128, 4, 4), kp)
    with torch.no_grad():
        pooled = model._pointnets(sources, kp)
    assert [tuple(p.shape) for p in pooled] == [(1, 32, 9), (1, 32, 9), (1, 64, 9), (1, 128, 9), (1, 128, 9)]
    assert sum(p.shape[1] for p in pooled) + model.cfg.PROPOSAL.C_IN == 512
