"""furthest_point_sample (csrc/pointops.hip) against tests/fps_ref.py at the dispatcher's sizes, on clouds where the slab skip decides
something, and on engineered ties: the picks equal fps_f32 bit for bit, are farthest points in float64, and -- on the slab sizes, where
the order inside a bin comes from LDS atomics -- come out the same from a second call.  tests/test_host_fps_ref.py shows on the host that
the reference is the oracle's, that the cases would see a wrong slab bound, and that the tie cases tie where they say.

Which run reaches what (run ids of tests/fps_cases.py):
  cube-n{1,2,64,65,1023,1024}            fps_kernel<1> up to its last point
  cube-n{1025,4096 | 4097,8192 | 8193,16384}   fps_slab_kernel<16 | 32 | 64> at both ends of each
  cube-n{16385,24576 | 24577,32768 | 32769,65535,65536}   fps_kernel<24 | 32 | 64> at both ends of each (the last two spill to scratch)
  {line,road,comb,clusters}-n*           elongated along x: the skip leaves 70-95 % of the slabs alone; comb ties at every step
  tie_{slots,lanes,waves}-n*             equal candidates in the slots of one thread, the lanes of one wave, different waves
  tie_{slabs,bin}-n*                     equal candidates in different slabs (the lowest index in the last one), in one bin
  outlier*, offset, tiny_span, heavy_bin one point at x = 1e6 (also as point 0), x + 1e5, x * 1e-25, 90 % of the points in ten bins
  lattice, doubled, all_equal            many ties, every point twice, one point n times
  cube-n*-k{1,2}, doubled-n{1024,1025,1300}-k=n   the shortest chains; K = N, where the copies drive the maximum to exactly 0
  line+all_equal+lattice-n*              three different frames in one launch
"""
import functools

import numpy as np
import pytest
import torch

import fps_cases as cases
import fps_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def want(rid):
    _, families, n, k = cases.RUNS[cases.RUN_IDS.index(rid)]
    out = ref.fps_f32(cases.build(families, n), k)
    out.setflags(write=False)
    return out


def gpu_fps(xyz, k):
    from vision3d_amd.pointnet2.pointnet2_utils import furthest_point_sample
    return furthest_point_sample(xyz if torch.is_tensor(xyz) else dev(xyz), k)


@pytest.mark.parametrize("run", cases.RUNS, ids=cases.RUN_IDS)
def test_fps_edges(run):
    rid, families, n, k = run
    xyz = cases.build(families, n)
    on_gpu = dev(xyz)
    idx = gpu_fps(on_gpu, k)
    assert idx.dtype == torch.int32 and idx.shape == (len(families), k)
    got = idx.cpu().numpy()
    np.testing.assert_array_equal(got, want(rid))
    for b in range(len(families)):
        ref.check_farthest_f64(xyz[b], got[b])
    if cases.is_slab(n):  # the scatter inside a bin may differ from call to call; the picks may not
        assert torch.equal(gpu_fps(on_gpu, k), idx)


@pytest.mark.parametrize("c", [1, 5])
def test_gather_on_the_picks_past_one_grid(c):
    """gather_operation launches at most 4 096 x 256 threads and strides beyond: B C K = 2 x 5 x 131 072 is 1.25 grids; C = 1 is a quarter
    of one.  The picks are checked first, so the gather only ever sees indices inside the cloud."""
    from vision3d_amd.pointnet2.pointnet2_utils import gather_operation
    n, k, families = 1024, 1024, ("doubled", "lattice")
    xyz = cases.build(families, n)
    idx = gpu_fps(xyz, k)
    np.testing.assert_array_equal(idx.cpu().numpy(), ref.fps_f32(xyz, k))
    idx = idx.repeat(1, 128)  # (2, 131 072): every pick 128 times
    feat = np.random.default_rng(5).standard_normal((2, c, n)).astype(np.float32)
    assert (c == 5) == (2 * c * idx.shape[1] > 4096 * 256)
    got = gather_operation(dev(feat), idx).cpu().numpy()
    at = idx.cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(got, np.stack([feat[b][:, at[b]] for b in range(2)]))


def test_refusals_and_the_empty_batch():
    cloud = dev(cases.build(("cube",), 1025))
    for k in (0, 1026):
        with pytest.raises(RuntimeError, match="furthest_point_sample"):
            gpu_fps(cloud, k)
    with pytest.raises(RuntimeError, match="furthest_point_sample"):  # 65 536 is the most one workgroup's registers hold
        gpu_fps(torch.zeros((1, 65537, 3), device="cuda"), 4)
    empty = gpu_fps(torch.zeros((0, 1025, 3), device="cuda"), 7)
    assert empty.shape == (0, 7) and empty.dtype == torch.int32


@pytest.mark.parametrize("n", [1024, 4097, 16385])
def test_a_column_view_gives_the_picks_of_its_copy(n):
    xyz = cases.build(("road", "lattice"), n)
    cloud = dev(np.concatenate([xyz, np.full((2, n, 1), 7.0, np.float32)], 2))
    view = cloud[..., :3]
    assert not view.is_contiguous()
    got = gpu_fps(view, 64)
    assert torch.equal(got, gpu_fps(view.contiguous(), 64))
    np.testing.assert_array_equal(got.cpu().numpy(), ref.fps_f32(xyz, 64))
