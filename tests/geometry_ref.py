"""Plain numpy restatements of the three integer-exact builders every later stage rests on: the voxelizer with its fused mean
(csrc/voxelize.hip), the submanifold and strided rulebooks (csrc/rulebook.hip, csrc/rb_device.h) and the transposed table.

Independent of the C oracle (oracle/v3d_oracle.c walks the points and tickets one by one through a hash table) and of the kernels:
every sequential rule ("first touch", "first max_pts points", "first cap_out outputs") is restated on sorted int64 keys with np.unique.
numpy only; the only Python loops run over frames, kernel offsets and point slots, never over points or sites.
"""
import numpy as np

MAX_BATCH = 64  # a coordinate row with b outside [0, 64) has no key (csrc/rb_device.h)


def _triple(v):
    return [int(v)] * 3 if np.isscalar(v) else [int(x) for x in v]


# ------------------------------------------------------------------------------------------------ voxelizer
def grid_of(voxel_size, bounds):
    """Cells per axis (x, y, z): round((hi - lo) / vs), the quotient in fp32, halves away from zero."""
    vs = np.asarray(voxel_size, np.float32)
    b = np.asarray(bounds, np.float32)
    q = (b[3:] - b[:3]) / vs
    return np.floor(q.astype(np.float64) + 0.5).astype(np.int64)


def cells_of(points, voxel_size, bounds):
    """-> (cells (N, 3) int64 as x, y, z; kept (N,) bool): floor((p - lo) / vs) in fp32, kept iff 0 <= f < grid on every axis (NaN and
    +-inf fail a comparison and are dropped).  Cells of dropped points are meaningless."""
    vs = np.asarray(voxel_size, np.float32)
    lo = np.asarray(bounds, np.float32)[:3]
    grid = grid_of(voxel_size, bounds)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((np.asarray(points, np.float32)[:, :3] - lo) / vs)
        kept = np.all((f >= np.float32(0)) & (f < grid.astype(np.float32)), axis=1)
    cells = np.where(kept[:, None], f, np.float32(0)).astype(np.int64)
    return cells, kept


def _voxelize_frame(points, voxel_size, bounds, max_pts, max_voxels):
    points = np.ascontiguousarray(points, np.float32)
    C = points.shape[1]
    grid = grid_of(voxel_size, bounds)
    cells, kept = cells_of(points, voxel_size, bounds)
    src = np.nonzero(kept)[0]  # input index of every kept point, ascending
    c = cells[src]
    key = (c[:, 2] * grid[1] + c[:, 1]) * grid[0] + c[:, 0]
    uniq, first, inv, counts = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")  # the distinct cells in first-touch order
    number = np.empty(len(uniq), np.int64)
    number[order] = np.arange(len(uniq))
    vid = number[inv]  # voxel number of every kept point, before the max_voxels cut
    M = min(len(uniq), int(max_voxels))
    # slot of a point inside its voxel = how many earlier points share the voxel: stable sort by voxel, position inside the run
    by_voxel = np.argsort(vid, kind="stable")
    run_start = np.concatenate([[0], np.cumsum(counts[order])])[:-1]
    slot = np.arange(len(vid)) - run_start[vid[by_voxel]]
    take = (slot < max_pts) & (vid[by_voxel] < M)  # later voxels are dropped WITH their points: the `continue` rule
    voxels = np.zeros((M, max_pts, C), np.float32)
    voxels[vid[by_voxel][take], slot[take]] = points[src[by_voxel][take]]
    occupancy = np.minimum(counts[order][:M], max_pts).astype(np.int32)
    coords = c[first[order][:M]][:, ::-1].astype(np.int32)  # (z, y, x)
    return voxels, coords, occupancy


def vfe_mean(voxels, occupancy):
    """fp32 sum of the max_pts slots in slot order, the zero slots included, divided by the occupancy in fp32."""
    voxels = np.asarray(voxels, np.float32)
    acc = np.zeros((voxels.shape[0], voxels.shape[2]), np.float32)
    for k in range(voxels.shape[1]):
        acc = acc + voxels[:, k, :]
    return acc / np.asarray(occupancy).astype(np.float32)[:, None]


def voxelize(frames, voxel_size, bounds, max_pts, max_voxels):
    """frames: list of (N_b, C) float32 clouds -> voxels (M, max_pts, C), coords (M, 4) int32 (b, z, y, x), occupancy (M,) int32,
    mean (M, C).  Voxels in first-touch order per frame, at most max_voxels per frame, the frames one after the other."""
    C = frames[0].shape[1] if len(frames) else 4
    vox, coords, occ = [np.zeros((0, max_pts, C), np.float32)], [np.zeros((0, 4), np.int32)], [np.zeros((0,), np.int32)]
    for b, pts in enumerate(frames):
        v, c, o = _voxelize_frame(pts, voxel_size, bounds, int(max_pts), int(max_voxels))
        vox.append(v)
        coords.append(np.concatenate([np.full((len(c), 1), b, np.int32), c], 1))
        occ.append(o)
    vox, coords, occ = np.concatenate(vox), np.concatenate(coords), np.concatenate(occ)
    return vox, coords, occ, vfe_mean(vox, occ)


# ------------------------------------------------------------------------------------------------ rulebooks
def _keys(b, z, y, x, shape):
    return ((b.astype(np.int64) * shape[0] + z) * shape[1] + y) * shape[2] + x


def _keyed(coords):
    return (coords[:, 0] >= 0) & (coords[:, 0] < MAX_BATCH)


def subm_rulebook(coords, n, shape, ksize):
    """-> nbr (K, n) int32: nbr[k][o] = the row at coords[o] + k - ks // 2 (same batch, inside the grid) or -1; the centre tap is the
    row itself.  Rows with b outside [0, 64) are nobody's neighbour and find none."""
    ks = _triple(ksize)
    co = np.asarray(coords, np.int64).reshape(-1, 4)[:n]
    K = ks[0] * ks[1] * ks[2]
    keyed = _keyed(co)
    rows = np.nonzero(keyed)[0]
    keys = _keys(co[rows, 0], co[rows, 1], co[rows, 2], co[rows, 3], shape)
    srt = np.argsort(keys, kind="stable")
    skeys, srows = keys[srt], rows[srt]
    nbr = np.full((K, n), -1, np.int32)
    for k in range(K):
        kx, ky, kz = k % ks[2], (k // ks[2]) % ks[1], k // (ks[2] * ks[1])
        if (kz, ky, kx) == (ks[0] // 2, ks[1] // 2, ks[2] // 2):
            nbr[k] = np.arange(n)
            continue
        z, y, x = co[:, 1] + kz - ks[0] // 2, co[:, 2] + ky - ks[1] // 2, co[:, 3] + kx - ks[2] // 2
        ok = keyed & (z >= 0) & (z < shape[0]) & (y >= 0) & (y < shape[1]) & (x >= 0) & (x < shape[2])
        if not len(skeys):
            continue
        q = _keys(co[:, 0], z, y, x, shape)
        pos = np.minimum(np.searchsorted(skeys, q), len(skeys) - 1)
        hit = ok & (skeys[pos] == q)
        nbr[k, hit] = srows[pos[hit]]
    return nbr


def sparse_rulebook(coords, n, shape, ksize, stride, pad, cap_out=None):
    """-> coords_out (n_out, 4) int32, nbr (K, n_out) int32, out_shape [3], overflow.  Input i with offset k reaches output
    (c + pad - k) / stride when that is divisible, non-negative and inside out_shape; outputs are numbered in the order a loop over
    (i, k), k fastest, first touches them; with cap_out only the first cap_out survive."""
    ks, st, pd = _triple(ksize), _triple(stride), _triple(pad)
    co = np.asarray(coords, np.int64).reshape(-1, 4)[:n]
    K = ks[0] * ks[1] * ks[2]
    out_shape = [(int(shape[j]) + 2 * pd[j] - ks[j]) // st[j] + 1 for j in range(3)]
    k = np.arange(K)
    kk = [k // (ks[2] * ks[1]), (k // ks[2]) % ks[1], k % ks[2]]
    ok = np.broadcast_to(_keyed(co)[:, None], (n, K)).copy()
    o = []
    for j in range(3):
        v = co[:, 1 + j, None] + pd[j] - kk[j][None, :]
        ok &= (v >= 0) & (v % st[j] == 0) & (v // st[j] < out_shape[j])
        o.append(v // st[j])
    t = np.nonzero(ok.ravel())[0]  # the live tickets i * K + k, ascending
    ti, tk = t // K, t % K
    b = co[ti, 0]
    oz, oy, ox = o[0].ravel()[t], o[1].ravel()[t], o[2].ravel()[t]
    uniq, first, inv = np.unique(_keys(b, oz, oy, ox, out_shape), return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")
    number = np.empty(len(uniq), np.int64)
    number[order] = np.arange(len(uniq))
    T = len(uniq)
    n_out = T if cap_out is None else min(T, int(cap_out))
    creators = first[order][:n_out]
    coords_out = np.stack([b[creators], oz[creators], oy[creators], ox[creators]], 1).astype(np.int32).reshape(-1, 4)
    nbr = np.full((K, n_out), -1, np.int32)
    out = number[inv]
    live = out < n_out
    nbr[tk[live], out[live]] = ti[live]
    overflow = bool((cap_out is not None and T > cap_out) or not _keyed(co).all())
    return coords_out, nbr, out_shape, overflow


def transpose(nbr, n_out, n_in):
    """-> nbrT (K, n_in) int32: nbrT[k][i] = o iff nbr[k][o] = i, -1 elsewhere."""
    nbr = np.asarray(nbr)[:, :n_out]
    out = np.full((nbr.shape[0], n_in), -1, np.int32)
    k, o = np.nonzero(nbr >= 0)
    out[k, nbr[k, o]] = o
    return out
