"""The device voxelizer (csrc/voxelize.hip) against tests/geometry_ref.py at its chunk, frame, channel, clipping and grid edges, bit
for bit: point slots, coordinates, occupancy, the fused mean (the same fp32 sum in the same order) and the voxel count.

Which run reaches what (run ids of tests/geometry_cases.py VOXEL_RUNS):
  one_frame_{1,255,256,257,511,512,513}-p{1,5,8}  n_points around VOX_CHUNK = 256 on the one-frame chained scan
  one_frame_66000-p*                              258 chunks: the second trip of the chained scan's wait for its predecessors
  one_frame_clip-mv{1,255,256,257,2000}           max_voxels on the chained scan: the count's min() and the drop of later voxels
  batch_chunk_boundaries                          frame boundaries on chunk boundaries, an empty frame in the middle
  batch_trailing_empty, batch_leading_empty       frames that start at n_points; a first frame without points
  batch_64_frames                                 B = 64, the most the frame table holds
  *-mv3                                           every frame of a batch clipped
  channels_{3,5,7}-p{1,8}                         the narrow generic channel loop (C != 4, max_pts <= 8); channels_4 beside it
  face                                            points on cell faces, one ulp either side, on both bounds, +-0.0: true fp32 division
  big_grid                                        4096 x 4096 x 512 cells: keys above 2^32
"""
import functools

import numpy as np
import pytest
import torch

import geometry_cases as cases
import geometry_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu
NAMES = ("voxels", "coords", "occupancy", "mean")


@functools.lru_cache(maxsize=None)
def reference(name, max_pts, max_voxels):
    c = cases.build(name)
    out = ref.voxelize(c["frames"], c["voxel_size"], c["bounds"], max_pts, max_voxels)
    for a in out:
        a.setflags(write=False)
    return out


def gpu_voxelize(c, max_pts, max_voxels, want_voxels=True):
    """-> (voxels | None, coords, occupancy, mean) cut to the device's count, and the count"""
    from vision3d_amd.spconv.utils import voxelize_batch
    frames = c["frames"]
    offs = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).tolist()
    vox, coords, occ, mean, n = voxelize_batch(dev(np.concatenate(frames), torch.float32), offs, c["voxel_size"], c["bounds"], max_pts,
                                               max_voxels, want_voxels=want_voxels)
    m = int(n.item())
    assert 0 <= m <= coords.shape[0]
    return (None if vox is None else vox[:m].cpu().numpy(), coords[:m].cpu().numpy(), occ[:m].cpu().numpy(), mean[:m].cpu().numpy()), m


def compare(got, want, names=NAMES):
    for g, w, name in zip(got, want, names):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize("run", cases.VOXEL_RUNS, ids=cases.VOXEL_RUN_IDS)
def test_voxelize_edges(run):
    _, name, max_pts, max_voxels = run
    want = reference(name, max_pts, max_voxels)
    got, m = gpu_voxelize(cases.build(name), max_pts, max_voxels)
    assert m == len(want[1]), ("count", m, len(want[1]))
    compare(got, want)


@pytest.mark.parametrize("name,max_voxels", [("one_frame_513", 70000), ("one_frame_clip", 256), ("batch_chunk_boundaries", 20000),
                                             ("batch_trailing_empty", 40)])
def test_without_the_point_slots(name, max_voxels):
    """want_voxels=False (a null `voxels`): coordinates, occupancy, mean and count as with the slots, and as the reference's."""
    c = cases.build(name)
    want = reference(name, 5, max_voxels)
    full, m_full = gpu_voxelize(c, 5, max_voxels)
    bare, m_bare = gpu_voxelize(c, 5, max_voxels, want_voxels=False)
    assert bare[0] is None and m_bare == m_full == len(want[1])
    compare(bare[1:], full[1:], NAMES[1:])
    compare(bare[1:], want[1:], NAMES[1:])
