"""numpy restatement of dynamic voxelization (include/vision3d_hip.h "T1d", csrc/voxelize.hip "DYNAMIC").

Cells by the hard voxelizer's own statements -- IEEE fp32 floor((q - lo) / vs) and its bounds test, a NaN coordinate drops the point --,
rows frame-major in first-touch order with the "continue" rule for max_voxels, occupancy = the true count, point_voxel = the row of
every point (-1: dropped), and the order-independent mean over S = 24 fractional bits:

    q_ic      = rint(double(v_ic) * 2^S)                          exact product, round half to even, int64
    mean[v,c] = float(double(sum_i q_ic) / (double(k) * 2^S))     the int64 sum is exact; every conversion and the division round to
                                                                  nearest even

A kept point's value that is not finite or not below 2^16 in magnitude contributes nothing; that (row, channel) mean is NaN and bit 0
of the status word is set.
"""
import numpy as np

S = 24
SCALE = float(2 ** S)
LIMIT = np.float32(2.0 ** 16)
MAX_POINTS = 1 << 22


def mean_of(values):
    """(k, C) float32 values of ONE cell -> ((C,) float32 mean, any value refused).  The definition, nothing else."""
    v = np.asarray(values, np.float32)
    with np.errstate(invalid="ignore"):
        good = np.abs(v) < LIMIT  # False for NaN and the infinities
    q = np.rint(np.where(good, v, np.float32(0)).astype(np.float64) * SCALE).astype(np.int64)
    total = q.sum(axis=0)  # int64: exact, associative
    mean = (total.astype(np.float64) / (np.float64(len(v)) * SCALE)).astype(np.float32)
    refused = ~good.all(axis=0)
    mean[refused] = np.nan
    return mean, bool(refused.any())


def mean_error_bound(true_mean):
    """The derived bound against the true float64 mean of the fp32 inputs: every term is off by at most 2^-(S+1), so their mean is;
    the int64 -> double conversion and the division are exact to 2^-53 relative (nothing at this scale); the final rounding to fp32
    adds half an ulp of the result."""
    m = np.abs(np.asarray(true_mean, np.float64))
    ulp = np.spacing(m.astype(np.float32)).astype(np.float64)
    return 2.0 ** -(S + 1) + ulp / 2


def cells_of(points, voxel_size, bounds):
    """-> ((N, 3) int64 cells (x, y, z), (N,) bool inside) by the insert kernel's fp32 statements."""
    pts = np.asarray(points, np.float32)
    vs = np.asarray(voxel_size, np.float32)
    lo = np.asarray(bounds[:3], np.float32)
    hi = np.asarray(bounds[3:], np.float32)
    grid = np.array([int(np.floor(np.float32(hi[j] - lo[j]) / vs[j] + np.float32(0.5))) for j in range(3)], np.int64)  # lroundf, fp32
    with np.errstate(invalid="ignore"):
        f = np.floor((pts[:, :3] - lo) / vs)  # fp32 subtraction and IEEE fp32 division
        ok = np.all((f >= 0) & (f < grid.astype(np.float32)), axis=1)
    c = np.where(ok[:, None], f, 0).astype(np.int64)
    return c, ok, grid


def voxelize_dynamic(clouds, voxel_size, bounds, max_voxels):
    """clouds: list of (N_b, C) float32.  -> dict(coords (M, 4) int32 (b, z, y, x), occupancy (M,) int32, mean (M, C) float32,
    point_voxel (sum N_b,) int32, n_out (2,) int32 = {M, status})."""
    C = clouds[0].shape[1] if len(clouds) else 4
    coords, occ, means, pv_all = [], [], [], []
    status, base = 0, 0
    for b, cloud in enumerate(clouds):
        cloud = np.asarray(cloud, np.float32)
        c, ok, grid = cells_of(cloud, voxel_size, bounds)
        key = (c[:, 2] * grid[1] + c[:, 1]) * grid[0] + c[:, 0]
        pv = np.full(len(cloud), -1, np.int64)
        idx = np.nonzero(ok)[0]
        if len(idx):
            uniq, first, inverse, counts = np.unique(key[idx], return_index=True, return_inverse=True, return_counts=True)
            order = np.argsort(first, kind="stable")            # first-touch order of the frame's cells
            rank = np.empty(len(uniq), np.int64)
            rank[order] = np.arange(len(uniq))
            local = rank[inverse]                               # row of every kept point inside its frame, before the clip
            kept = local < max_voxels                           # the "continue" rule: later cells are skipped, their points dropped
            pv[idx[kept]] = base + local[kept]
            n_rows = min(len(uniq), int(max_voxels))
            by_row = np.argsort(local[kept], kind="stable")
            members = idx[kept][by_row]
            k = counts[order][:n_rows]
            starts = np.concatenate([[0], np.cumsum(k)])[:-1]
            # mean_of for every row at once (tests/test_host_dynamic_voxel_ref.py holds the two against each other)
            v = cloud[members]
            with np.errstate(invalid="ignore"):
                good = np.abs(v) < LIMIT
            q = np.rint(np.where(good, v, np.float32(0)).astype(np.float64) * SCALE).astype(np.int64)
            total = np.add.reduceat(q, starts, axis=0)
            refused = np.add.reduceat((~good).astype(np.int64), starts, axis=0) > 0
            m = (total.astype(np.float64) / (k.astype(np.float64)[:, None] * SCALE)).astype(np.float32)
            m[refused] = np.nan
            status |= int(refused.any())
            means.append(m)
            cell = c[idx[first[order[:n_rows]]]]
            coords.append(np.stack([np.full(n_rows, b), cell[:, 2], cell[:, 1], cell[:, 0]], axis=1))
            occ.append(k)
            base += n_rows
        pv_all.append(pv)
    coords = np.concatenate(coords) if coords else np.zeros((0, 4), np.int64)
    M = len(coords)
    return dict(coords=coords.astype(np.int32), occupancy=(np.concatenate(occ) if occ else np.zeros(0, np.int64)).astype(np.int32),
                mean=np.concatenate(means) if means else np.zeros((0, C), np.float32),
                point_voxel=(np.concatenate(pv_all) if pv_all else np.zeros(0, np.int64)).astype(np.int32),
                n_out=np.asarray([M, status], np.int32))


def by_cell(out):
    """{cell -> (count, mean)} as arrays sorted by (b, z, y, x): what must not depend on the order of the points."""
    m = int(out["n_out"][0])
    order = np.lexsort(out["coords"][:m].T[::-1])
    return out["coords"][:m][order], out["occupancy"][:m][order], out["mean"][:m][order]
