"""CPU: the definition of the dynamic voxelizer's mean (tests/dynamic_voxel_ref.py) against a plain float64 mean, within the bound
derived from the definition (2^-25 + half an fp32 ulp of the mean), and bit for bit invariant under permutation."""
import numpy as np
import pytest

import dynamic_voxel_ref as ref

KS = [1, 2, 5, 8, 9, 64, 65, 257, 1000]


def _cell(rng, k, C=4):
    """k points of one KITTI-range cell neighbourhood: x in [0, 70.4), y in [-40, 40), z in [-3, 1), intensity in [0, 1)."""
    v = rng.uniform(0.0, 1.0, size=(k, C)).astype(np.float32)
    v[:, 0] *= np.float32(70.4)
    v[:, 1] = v[:, 1] * np.float32(80.0) - np.float32(40.0)
    v[:, 2] = v[:, 2] * np.float32(4.0) - np.float32(3.0)
    return v


@pytest.mark.parametrize("k", KS)
def test_mean_within_the_derived_bound_of_the_float64_mean(k):
    rng = np.random.default_rng([11, k])
    worst = 0.0
    for _ in range(50):
        v = _cell(rng, k)
        got, refused = ref.mean_of(v)
        true = v.astype(np.float64).sum(axis=0) / k  # (fp32 values of this range: the float64 sum of 1000 of them is exact to 2^-43)
        err = np.abs(got.astype(np.float64) - true)
        bound = ref.mean_error_bound(true)
        worst = max(worst, float((err / bound).max()))
        assert not refused and (err <= bound).all(), (k, err, bound)
    print("dynamic-mean-figures", dict(k=k, worst_ratio_to_bound=worst))


@pytest.mark.parametrize("k", KS)
def test_mean_is_invariant_under_permutation_bit_for_bit(k):
    rng = np.random.default_rng([12, k])
    v = _cell(rng, k)
    want, _ = ref.mean_of(v)
    for _ in range(8):
        got, _ = ref.mean_of(v[rng.permutation(k)])
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))


def test_refused_values_make_that_mean_nan_and_nothing_else():
    v = _cell(np.random.default_rng(13), 9)
    want, _ = ref.mean_of(v)
    for bad in (np.nan, np.inf, -np.inf, 65536.0, 1e6):
        w = v.copy()
        w[4, 3] = bad
        got, refused = ref.mean_of(w)
        assert refused and np.isnan(got[3])
        np.testing.assert_array_equal(got[:3], want[:3])
    w = v.copy()
    w[4, 3] = np.float32(65535.996)  # the largest fp32 below 2^16: inside the range
    assert not ref.mean_of(w)[1]


def test_batch_restatement_equals_the_definition_cell_by_cell():
    """voxelize_dynamic sums every row at once (reduceat); mean_of is the definition.  Rows, counts, the point map and the clip too."""
    rng = np.random.default_rng(14)
    clouds = []
    for n in (700, 1, 300):
        p = rng.uniform(0.0, 1.0, size=(n, 5)).astype(np.float32)
        p[:, 0] = p[:, 0] * 2.2 - 0.1
        p[:, 1] = p[:, 1] * 2.2 - 1.1
        p[:, 2] = p[:, 2] * 1.2 - 0.1
        clouds.append(p)
    clouds[0][5, 2] = np.nan
    clouds[0][::7, :3] = clouds[0][3, :3]
    clouds[2][10] = [1.0, 0.1, 0.6, 0.5, np.inf]  # inside the bounds
    vs, bounds = [0.25, 0.25, 0.5], [0.0, -1.0, 0.0, 2.0, 1.0, 1.0]
    for max_voxels in (1000, 40):
        out = ref.voxelize_dynamic(clouds, vs, bounds, max_voxels)
        flat = np.concatenate(clouds)
        m, status = out["n_out"]
        assert m == len(out["coords"]) == len(out["occupancy"]) == len(out["mean"]) and status == 1
        c, ok, grid = ref.cells_of(flat, vs, bounds)
        frame = np.repeat(np.arange(3), [len(p) for p in clouds])
        seen = -1
        for i in range(len(flat)):  # the sequential loop: rows in first-touch order, frame-major
            r = out["point_voxel"][i]
            if not ok[i]:
                assert r == -1
                continue
            if r > seen:
                assert r == seen + 1  # a new row is the next row
                seen = r
            if r >= 0:
                np.testing.assert_array_equal(out["coords"][r], [frame[i], c[i, 2], c[i, 1], c[i, 0]])
        assert seen == m - 1
        per_frame = [len(np.unique(out["coords"][out["coords"][:, 0] == b], axis=0)) for b in range(3)]
        assert max(per_frame) <= max_voxels and (max_voxels == 1000 or per_frame[0] == 40)
        nan_rows = 0
        for r in range(m):
            mem = np.nonzero(out["point_voxel"] == r)[0]
            assert out["occupancy"][r] == len(mem)
            want, refused = ref.mean_of(flat[mem])
            nan_rows += refused
            np.testing.assert_array_equal(out["mean"][r].view(np.int32), want.view(np.int32))
        assert out["point_voxel"][701 + 10] >= 0 and nan_rows == 1  # (the infinite value sits in one of its frame's first rows)
