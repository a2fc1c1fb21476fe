"""GPU: the host copies of the two geometry buffer pairs follow their buffers (vision3d_amd/stamp.py): the fused launches that take
them as scalars stay bit-identical to the torch statements, which read the buffers on every call.  (The captured-graph side of the
same rule: tests/test_gpu_plan.py.)"""
import pytest
import torch

from vision3d_amd.core.config import second_car_cfg

pytestmark = pytest.mark.gpu


def test_voxel_centers_follow_the_geometry_buffers():
    """SparseCNNBase.to_global == to_global_torch bit for bit, before and after an in-place edit of voxel_offset, a load_state_dict
    and a replaced base_voxel_size; two strides (two keys of the cache) each time."""
    from vision3d_amd import spconv
    from vision3d_amd.detector import sparse_cnn
    cfg = second_car_cfg()
    cnn = sparse_cnn.CNN_FACTORY[cfg.CNN](cfg).cuda()
    g = torch.Generator().manual_seed(0)
    n = 300
    ind = torch.stack([torch.zeros(n, dtype=torch.int32), torch.randint(0, 41, (n,), generator=g, dtype=torch.int32),
                       torch.randint(0, 1600, (n,), generator=g, dtype=torch.int32),
                       torch.randint(0, 1408, (n,), generator=g, dtype=torch.int32)], dim=1).cuda()
    vol = spconv.SparseConvTensor(torch.randn(n, 16, device="cuda"), ind, cnn.grid_shape, 1)

    def check():
        out = []
        for stride in cfg.STRIDES[:2]:
            xyz, feat = cnn.to_global(stride, vol)
            ref_xyz, ref_feat = cnn.to_global_torch(stride, vol)
            assert torch.equal(xyz, ref_xyz) and torch.equal(feat, ref_feat)
            out.append(xyz.clone())
        return out

    first = check()
    assert all(torch.equal(a, b) for a, b in zip(check(), first))  # (the steady state: cache hits)
    cnn.voxel_offset.add_(0.25)
    moved = check()
    assert not any(torch.equal(a, b) for a, b in zip(moved, first))
    # the two buffers are not persistent: a state dict does not carry them, and one that names them (strict=False) leaves them alone
    state = cnn.state_dict()
    assert "base_voxel_size" not in state
    cnn.load_state_dict(dict(state, base_voxel_size=cnn.base_voxel_size * 1.5), strict=False)
    assert all(torch.equal(a, b) for a, b in zip(check(), moved))
    # ... a loader that wants another voxel size replaces the buffer on the module: a new tensor at another address
    cnn.base_voxel_size = cnn.base_voxel_size * 1.5
    assert not any(torch.equal(a, b) for a, b in zip(check(), moved))


def test_bev_gather_follows_the_geometry_buffers():
    """BEVFeatureGatherer.gather_point_major == forward_torch bit for bit, before and after an in-place edit of pixel_offset:
    B = 1, C = 8, a 16 x 16 map, 5 keypoints (one on a pixel centre, one outside the map: the clamp)."""
    from vision3d_amd.detector.layers import BEVFeatureGatherer
    cfg = second_car_cfg()
    bev = BEVFeatureGatherer(cfg, torch.tensor(cfg.GRID_BOUNDS[:3]), torch.tensor(cfg.VOXEL_SIZE)).cuda().eval()
    g = torch.Generator().manual_seed(1)
    fmap = torch.randn(1, 8, 16, 16, generator=g).cuda()
    pixel = bev.base_pixel_size * cfg.STRIDES[-1]
    kp = torch.zeros(1, 5, 3)
    kp[0, :, :2] = torch.rand(5, 2, generator=g) * 15.0
    kp[0, 0, :2] = torch.tensor([3.0, 7.0])
    kp[0, 4, :2] = torch.tensor([-4.0, 40.0])
    kp = kp.cuda()
    kp[0, :, :2] = kp[0, :, :2] * pixel + bev.pixel_offset
    with torch.no_grad():
        first = bev.gather_point_major(fmap, kp).transpose(1, 2).clone()
        assert first.shape == (1, 8, 5) and torch.equal(first, bev.forward_torch(fmap, kp))
        assert torch.equal(bev.gather_point_major(fmap, kp).transpose(1, 2), first)  # (the steady state: a cache hit)
        bev.pixel_offset.add_(0.3 * pixel)
        moved = bev.gather_point_major(fmap, kp).transpose(1, 2)
        assert torch.equal(moved, bev.forward_torch(fmap, kp)) and not torch.equal(moved, first)
