"""Voxel RoI pooling of PV-RCNN's stage 2 (cfg.VOXELPOOL) restated in numpy float64: the specification the kernels of
csrc/voxel_pool.hip and the torch statements of detector/voxel_roi_pool.py are tested against.  Upstream has no such module; the
definition is this repository's.

  grid points   RoI (x, y, z, w, l, h, yaw), grid index (i, j, k) in [0, G)^3, point (i * G + j) * G + k:
                centre + Rz(yaw) . (((i + .5) / G - .5) w, ((j + .5) / G - .5) l, ((k + .5) / G - .5) h)
  voxel query   per point p and level (stride s, active coordinates (b, z, y, x), size = float32(base_voxel_size * s), offset):
                corner(u) = u * size + offset, centre(u) = corner(u) + size / 2; home cell v = floor((p - offset) / size);
                candidates v + (dz, dy, dx) with |d| <= (rz, ry, rx) in ascending lexicographic (dz, dy, dx) order; a hit lies inside
                the level's shape, is an active site of the RoI's own frame and has |centre(u) - p|^2 < RADIUS^2 (strict); the first
                NSAMPLE hits are taken, missing slots repeat the first hit, no hit: indices -1, pooled features exactly zero
  pooling       row of a hit = [centre(u) - p, feat(u)] through the level's shared MLP (Linear without bias, BatchNorm eps 1e-3, ReLU per
                layer), max over the slots; levels concatenated on channels; per RoI the (G^3 * C) row in (grid point, channel) order
                through the reduction MLP (Linear without bias + ReLU per layer).

The query is defined on float32 values; this restatement evaluates it in float64 and MARKS the points whose answer a float32
evaluation may legitimately decide the other way (`undecidable`): (p - offset) / size within 1e-4 of an integer on some axis, or a
candidate with |d^2 - r^2| < 1e-4 r^2.  Comparisons leave those points out."""
import numpy as np

BN_EPS = 1e-3
EDGE = 1e-4


def grid_samples(g):
    """(G^3, 3) float32: ((i + .5) / G, (j + .5) / G, (k + .5) / G), point (i * G + j) * G + k."""
    t = ((np.arange(g, dtype=np.float32) + np.float32(0.5)) / np.float32(g)).astype(np.float32)
    i, j, k = np.meshgrid(t, t, t, indexing="ij")
    return np.stack([i, j, k], -1).reshape(-1, 3)


def grid_points(rois, g):
    """rois (..., 7) -> (..., G^3, 3) float64."""
    rois = np.asarray(rois, np.float64)
    local = (grid_samples(g).astype(np.float64) - 0.5) * rois[..., None, 3:6]
    c, s = np.cos(rois[..., None, 6]), np.sin(rois[..., None, 6])
    rot = np.stack([c * local[..., 0] - s * local[..., 1], s * local[..., 0] + c * local[..., 1], local[..., 2]], -1)
    return rois[..., None, 0:3] + rot


def level_scale(base_voxel_size, stride):
    """(x, y, z) size of a level's voxels: the float32 product, as SparseCNNBase.to_global rounds it."""
    return (np.asarray(base_voxel_size, np.float32) * np.float32(stride)).astype(np.float32)


def centres(zyx, scale, offset):
    """integer (.., 3) = (z, y, x) -> (.., 3) = (x, y, z) metric centres, float64."""
    scale, offset = np.asarray(scale, np.float64), np.asarray(offset, np.float64)
    return np.asarray(zyx, np.float64)[..., ::-1] * scale + offset + 0.5 * scale


def voxel_query(points, frames, coords, shape, scale, offset, rng, radius, nsample):
    """points (R, 3), frames (R,) frame of every point, coords (n, 4) = (b, z, y, x) the live rows of the level.
    -> idx (R, nsample) int32, empty (R,) bool, undecidable (R,) bool."""
    points = np.asarray(points, np.float64)
    scale64, offset64 = np.asarray(scale, np.float64), np.asarray(offset, np.float64)
    table = {tuple(int(v) for v in c): r for r, c in enumerate(np.asarray(coords).reshape(-1, 4))}
    rz, ry, rx = (int(v) for v in rng)
    r2 = float(radius) ** 2
    n_pts = points.shape[0]
    idx = np.full((n_pts, nsample), -1, np.int32)
    empty = np.ones(n_pts, bool)
    undecidable = np.zeros(n_pts, bool)
    for r in range(n_pts):
        p = points[r]
        f = (p - offset64) / scale64  # x, y, z
        if (np.abs(f - np.round(f)) < EDGE).any():
            undecidable[r] = True
        vx, vy, vz = (int(v) for v in np.floor(f))
        hits = []
        for dz in range(-rz, rz + 1):
            for dy in range(-ry, ry + 1):
                for dx in range(-rx, rx + 1):
                    z, y, x = vz + dz, vy + dy, vx + dx
                    if not (0 <= z < shape[0] and 0 <= y < shape[1] and 0 <= x < shape[2]):
                        continue
                    row = table.get((int(frames[r]), z, y, x))
                    if row is None:
                        continue
                    d2 = float(((centres((z, y, x), scale, offset) - p) ** 2).sum())
                    if abs(d2 - r2) < EDGE * r2:
                        undecidable[r] = True
                    if d2 < r2:
                        hits.append(row)
        if hits:
            empty[r] = False
            taken = hits[:nsample]
            idx[r] = taken + [taken[0]] * (nsample - len(taken))
    return idx, empty, undecidable


def mlp_layers(state, prefix, bn=True):
    """[(W (out, in), gamma, beta, mean, var) or (W,)] of a layers.MLP from a numpy state_dict, as float64."""
    out, i = [], 0
    while f"{prefix}linear_{i}.weight" in state:
        w = np.asarray(state[f"{prefix}linear_{i}.weight"], np.float64)
        if bn:
            out.append((w,) + tuple(np.asarray(state[f"{prefix}batchnorm_{i}.{k}"], np.float64)
                                    for k in ("weight", "bias", "running_mean", "running_var")))
        else:
            out.append((w,))
        i += 1
    return out


def mlp(x, layers):
    """Linear without bias [+ eval BatchNorm(eps 1e-3)] + ReLU per layer, float64."""
    x = np.asarray(x, np.float64)
    for layer in layers:
        x = x @ layer[0].T
        if len(layer) > 1:
            _, gamma, beta, mean, var = layer
            x = (x - mean) / np.sqrt(var + BN_EPS) * gamma + beta
        x = np.maximum(x, 0.0)
    return x


def pool_level(points, idx, coords, feats, scale, offset, layers):
    """points (R, 3), idx (R, ns) from voxel_query, coords (n, 4), feats (n, C) -> (R, C_out) float64; empty points: zeros."""
    points, feats = np.asarray(points, np.float64), np.asarray(feats, np.float64)
    n_pts, ns = idx.shape
    c_out = layers[-1][0].shape[0]
    out = np.zeros((n_pts, c_out))
    live = idx[:, 0] >= 0
    if not live.any():
        return out
    ii = idx[live]  # (L, ns)
    rel = centres(np.asarray(coords)[ii][..., 1:4], scale, offset) - points[live][:, None, :]
    rows = np.concatenate([rel, feats[ii]], -1)
    out[live] = mlp(rows.reshape(-1, rows.shape[-1]), layers).reshape(ii.shape[0], ns, c_out).max(1)
    return out


def voxel_roi_pool(rois, levels, cfg, state, prefix=""):
    """rois (B, n, 7); levels: list (one per cfg LEVELS entry) of dict(coords (n, 4), feats (n, C), shape, scale, offset);
    cfg: dict(GRID, RANGE, RADIUS, NSAMPLE); state: numpy state_dict of the VoxelRoiPool.  -> pooled (B, n, C_red) float64,
    undecidable (B, n) bool (some grid point of the RoI is undecidable on some level)."""
    rois = np.asarray(rois)
    b, n = rois.shape[:2]
    g = int(cfg["GRID"])
    pts = grid_points(rois, g).reshape(-1, 3)
    frames = np.repeat(np.arange(b), n * g ** 3)
    blocks, und = [], np.zeros(pts.shape[0], bool)
    for k, lv in enumerate(levels):
        idx, _, u = voxel_query(pts, frames, lv["coords"], lv["shape"], lv["scale"], lv["offset"], cfg["RANGE"][k], cfg["RADIUS"][k],
                                int(cfg["NSAMPLE"]))
        und |= u
        blocks.append(pool_level(pts, idx, lv["coords"], lv["feats"], lv["scale"], lv["offset"], mlp_layers(state, f"{prefix}mlps.{k}.")))
    per_roi = np.concatenate(blocks, -1).reshape(b, n, -1)
    return mlp(per_roi, mlp_layers(state, f"{prefix}reduction.", bn=False)), und.reshape(b, n, -1).any(-1)


# ---- cases shared by the host and the GPU tests
def make_level(seed, batch=2, shape=(5, 24, 24), per_frame=300, channels=8, scale=(0.4, 0.4, 0.8), offset=(0.0, -4.8, -3.0)):
    """A hand-built sparse level: `per_frame` distinct active sites per frame, frame-sorted rows; cell (1, 3, 3) is active in frame 0
    only.  -> dict(coords (n, 4) int32, feats (n, C) float32, shape, scale float32 (3,), offset float32 (3,))."""
    rng = np.random.default_rng(seed)
    cells = int(np.prod(shape))
    special = (1 * shape[1] + 3) * shape[2] + 3
    rows = []
    for b in range(batch):
        pick = rng.choice(cells, per_frame, replace=False)
        pick = pick[pick != special]
        if b == 0:
            pick = np.concatenate([pick, [special]])
        pick = rng.permutation(pick)
        z, y, x = np.unravel_index(pick, shape)
        rows.append(np.stack([np.full_like(z, b), z, y, x], 1))
    coords = np.concatenate(rows).astype(np.int32)
    feats = rng.normal(0, 1, (coords.shape[0], channels)).astype(np.float32)
    return dict(coords=coords, feats=feats, shape=list(shape), scale=np.asarray(scale, np.float32), offset=np.asarray(offset, np.float32))


def make_rois(seed, level, batch=2):
    """(batch, 3, 7) float32 per frame: a RoI inside the level, one straddling its edge, one wholly outside."""
    rng = np.random.default_rng(seed)
    lo = level["offset"].astype(np.float64)
    hi = lo + level["scale"].astype(np.float64) * np.asarray(level["shape"][::-1])
    out = np.zeros((batch, 3, 7), np.float32)
    for b in range(batch):
        mid = lo + (hi - lo) * rng.uniform(0.35, 0.65, 3)
        if b == 1:  # around the cell that is active in frame 0 only (make_level): frame 1 must not find it
            mid = centres((1, 3, 3), level["scale"], level["offset"]) + 0.07
        out[b, 0] = [*mid, *rng.uniform(1.5, 3.5, 2), rng.uniform(1.2, 2.0), rng.uniform(-3.1, 3.1)]
        out[b, 1] = [lo[0] + rng.uniform(-0.3, 0.3), mid[1], hi[2] - rng.uniform(0.0, 0.4), *rng.uniform(1.5, 3.5, 2), 1.6,
                     rng.uniform(-3.1, 3.1)]
        out[b, 2] = [hi[0] + 30.0, hi[1] + 30.0, mid[2], 3.9, 1.6, 1.5, rng.uniform(-3.1, 3.1)]
    return out
