"""Seeded cases of the voxelizer and the rulebook builders at their chunk and grid edges, shared by tests/test_host_geometry_ref.py and
the two GPU files (tests/test_gpu_voxelize_edges.py, tests/test_gpu_rulebook_edges.py).  numpy only; nothing here computes an
expected value.  `build(name)` returns the case as a dict; the *_RUNS tables say with which parameters the tests run it.

Voxelizer cases: dict(kind="voxel", frames=[(N_b, C) float32, ...], voxel_size, bounds).  The voxelizer walks the points in chunks of
VOX_CHUNK = 256 (one workgroup each); one frame takes the chained scan, several frames the count + scan + emit form.
Rulebook cases: dict(kind="sites", coords=(n, 4) int32 rows (b, z, y, x) in random order, shape=[D, H, W], batch).  The strided
builder scans tickets (Kc = prod(ceil(ks / stride)) per input row) in chunks of 2 048; both chained scans add up their predecessors'
counts 256 at a time, so more than 256 chunks is a second trip.
"""
import numpy as np

VOX_CHUNK = 256
SCAN_CHUNK = 2048
SUBM_KPT_MIN_ROWS = 40960  # csrc/rb_device.h: from this capacity on a 3x3x3 table takes nine offsets per thread

SMALL_BOUNDS = [0.0, -4.0, -3.0, 6.4, 4.0, 1.0]
SMALL_VOXEL = [0.1, 0.1, 4.0]  # 64 x 80 x 1 cells
KITTI_BOUNDS = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
KITTI_VOXEL = [0.05, 0.05, 0.1]  # not representable in binary: 1408 x 1600 x 40 cells
BIG_BOUNDS = [0.0, -204.8, -3.0, 409.6, 204.8, 48.2]
BIG_VOXEL = [0.1, 0.1, 0.1]  # 4096 x 4096 x 512 = 2^33 cells

ONE_FRAME_SIZES = [1, 255, 256, 257, 511, 512, 513, 66000]
CLIP_DISTINCT = 300  # the clip case opens with this many points in cells of their own
BATCH_SIZES = {
    "batch_chunk_boundaries": (256, 256, 1, 0, 255, 257),  # frame boundaries on chunk boundaries, an empty frame in the middle
    "batch_trailing_empty": (300, 0, 0),
    "batch_leading_empty": (0, 300),
}
CHANNELS = [3, 4, 5, 7]


def _rng(name):
    return np.random.default_rng([20261, sum(ord(ch) * (i + 1) for i, ch in enumerate(name))])


# ------------------------------------------------------------------------------------------------ voxelizer
def _sweep_cloud(rng, n, C=4):
    """n points on the small grid that walk through its cells with the point index, about three to a cell and a few cells of jitter (so
    voxels are opened in every chunk and collect several points; the last point opens the last cell), about 4 % of them outside the
    bounds, a NaN and an inf where n allows."""
    cells = 64 * 80
    span = max(1, min(cells - 1, n // 3))
    cell = np.clip(np.floor(np.arange(n) * span / n + rng.uniform(-4.0, 4.0, n)), 0, span - 1).astype(np.int64)
    cell[-1] = cells - 1
    u = rng.uniform(0.1, 0.9, (n, 2))
    p = np.empty((n, C), np.float64)
    p[:, 0] = (cell % 64 + u[:, 0]) * 0.1
    p[:, 1] = -4.0 + (cell // 64 + u[:, 1]) * 0.1
    p[:, 2] = rng.uniform(-3.0, 1.0, n)
    p[:, 3:] = rng.uniform(0.0, 1.0, (n, C - 3))
    if n > 1:
        out = np.nonzero(rng.random(n - 1) < 0.04)[0]
        p[out[::2], 1] += 8.05
        p[out[1::2], 2] -= 4.5
    p = p.astype(np.float32)
    if n >= 200:
        p[n // 3, 1] = np.nan
        p[n // 2, 0] = np.inf
        p[n // 2 + 1, 2] = -np.inf
    return p


def _box_cloud(rng, n, C=4, cells=(12, 10)):
    """n points over a cells[0] x cells[1] patch of the small grid: a few points per cell at the frame sizes used here."""
    p = np.empty((n, C), np.float64)
    p[:, 0] = rng.uniform(0.0, cells[0] * SMALL_VOXEL[0], n)
    p[:, 1] = rng.uniform(-4.0, -4.0 + cells[1] * SMALL_VOXEL[1], n)
    p[:, 2] = rng.uniform(-3.0, 1.0, n)
    p[:, 3:] = rng.uniform(0.0, 1.0, (n, C - 3))
    return p.astype(np.float32)


def _clip_cloud(rng):
    """about 2 000 points: the first CLIP_DISTINCT sit in cells of their own (all first touchers, so a cut at 255 / 256 / 257 voxels
    falls inside, at the end of and just behind the first chunk), the rest revisit those cells and open several hundred more."""
    n = 2000
    cell = rng.choice(64 * 80, size=900, replace=False)
    which = np.concatenate([np.arange(CLIP_DISTINCT), rng.integers(0, 900, n - CLIP_DISTINCT)])
    u = rng.uniform(0.1, 0.9, (n, 2))
    p = np.empty((n, 4), np.float64)
    p[:, 0] = (cell[which] % 64 + u[:, 0]) * 0.1
    p[:, 1] = -4.0 + (cell[which] // 64 + u[:, 1]) * 0.1
    p[:, 2] = rng.uniform(-3.0, 1.0, n)
    p[:, 3] = rng.uniform(0.0, 1.0, n)
    return p.astype(np.float32)


def face_candidates(axis):
    """Every cell face lo + k * vs of a KITTI axis (k = 0 .. grid: both bounds included), the product rounded once to fp32 and
    rounded as fp32 arithmetic, each with its two fp32 neighbours; and +-0.0 relative to lo."""
    lo, vs = np.float32(KITTI_BOUNDS[axis]), np.float32(KITTI_VOXEL[axis])
    grid = int(round((KITTI_BOUNDS[3 + axis] - KITTI_BOUNDS[axis]) / KITTI_VOXEL[axis]))
    k = np.arange(grid + 1)
    exact = (KITTI_BOUNDS[axis] + k * KITTI_VOXEL[axis]).astype(np.float32)
    fp32 = lo + k.astype(np.float32) * vs
    face = np.unique(np.concatenate([exact, fp32]))
    inf = np.float32(np.inf)
    out = np.concatenate([face, np.nextafter(face, -inf), np.nextafter(face, inf), [lo + np.float32(0.0), lo - np.float32(0.0)]])
    if lo == 0:
        out = np.concatenate([out, np.array([0.0, -0.0], np.float32)])
    return out.astype(np.float32)


def reciprocal_disagrees(values, axis):
    """True where floor((p - lo) / vs) and floor((p - lo) * (1 / vs)), both in fp32, differ."""
    lo, vs = np.float32(KITTI_BOUNDS[axis]), np.float32(KITTI_VOXEL[axis])
    d = values.astype(np.float32) - lo
    return np.floor(d / vs) != np.floor(d * (np.float32(1) / vs))


def _face_cloud(rng):
    """Every face candidate of every axis at random other coordinates, each with two companions that differ from it along the axis
    only and sit in the middle of the cell the fp32 quotient puts it in and of the cell below: a point that lands in the wrong cell
    leaves one companion's voxel and joins the other's, whichever of the two cell computations (key, coordinates) is wrong."""
    parts = []
    for axis in range(3):
        v = face_candidates(axis)
        lo, vs = np.float32(KITTI_BOUNDS[axis]), np.float32(KITTI_VOXEL[axis])
        grid = int(round((KITTI_BOUNDS[3 + axis] - KITTI_BOUNDS[axis]) / KITTI_VOXEL[axis]))
        p = np.empty((len(v), 4), np.float32)
        p[:, 0] = rng.uniform(10.0, 60.0, len(v))
        p[:, 1] = rng.uniform(-30.0, 30.0, len(v))
        p[:, 2] = rng.uniform(-2.5, 0.5, len(v))
        p[:, 3] = rng.uniform(0.0, 1.0, len(v))
        p[:, axis] = v
        parts.append(p)
        cell = np.clip(np.floor((v - lo) / vs), 0, grid - 1).astype(np.int64)
        for below in (0, 1):
            q = p.copy()
            q[:, axis] = (KITTI_BOUNDS[axis] + (np.maximum(cell - below, 0) + 0.5) * KITTI_VOXEL[axis]).astype(np.float32)
            q[:, 3] = rng.uniform(0.0, 1.0, len(v))
            parts.append(q)
    p = np.concatenate(parts)
    return p[rng.permutation(len(p))]


def _big_grid_frames(rng):
    """two frames of about 500 points in the eight corners and the centre of the 2^33-cell grid, several to a cell."""
    grid = np.array([4096, 4096, 512])
    lo, vs = np.array(BIG_BOUNDS[:3]), np.array(BIG_VOXEL)
    frames = []
    for _ in range(2):
        anchors = [np.array([cx, cy, cz]) for cx in (0, 1) for cy in (0, 1) for cz in (0, 1)]
        cells = []
        for a in anchors:
            base = np.where(a == 1, grid - 3, 0)
            cells.append(base + rng.integers(0, 3, (52, 3)))
        cells.append(grid // 2 - 1 + rng.integers(0, 3, (84, 3)))
        cells = np.concatenate(cells)
        cells[:8] = [np.where(a == 1, grid - 1, 0) for a in anchors]  # the corner cells themselves
        cells = cells[rng.permutation(len(cells))]
        p = np.empty((len(cells), 4), np.float64)
        p[:, :3] = lo + (cells + rng.uniform(0.25, 0.75, cells.shape)) * vs
        p[:, 3] = rng.uniform(0.0, 1.0, len(cells))
        frames.append(p.astype(np.float32))
    return frames


def _voxel_case(name):
    rng = _rng(name)
    small = dict(kind="voxel", name=name, voxel_size=SMALL_VOXEL, bounds=SMALL_BOUNDS)
    if name == "one_frame_clip":
        return dict(small, frames=[_clip_cloud(rng)])
    if name.startswith("one_frame_"):
        return dict(small, frames=[_sweep_cloud(rng, int(name.rsplit("_", 1)[1]))])
    if name in BATCH_SIZES:
        return dict(small, frames=[_box_cloud(rng, n) for n in BATCH_SIZES[name]])
    if name == "batch_64_frames":
        return dict(small, frames=[_box_cloud(rng, int(n), cells=(4, 3)) for n in rng.integers(7, 41, 64)])
    if name.startswith("channels_"):
        C = int(name.rsplit("_", 1)[1])
        xyz = _box_cloud(_rng("channels"), 700)[:, :3]  # the same xyz for every C
        return dict(small, frames=[np.concatenate([xyz, rng.uniform(0.0, 1.0, (700, C - 3)).astype(np.float32)], 1)])
    if name == "face":
        return dict(kind="voxel", name=name, voxel_size=KITTI_VOXEL, bounds=KITTI_BOUNDS, frames=[_face_cloud(rng)])
    if name == "big_grid":
        return dict(kind="voxel", name=name, voxel_size=BIG_VOXEL, bounds=BIG_BOUNDS, frames=_big_grid_frames(rng))
    raise KeyError(name)


# (id, case, max_pts, max_voxels): what the host test runs against the oracle and the GPU test against the reference
VOXEL_RUNS = []
for _n in ONE_FRAME_SIZES:
    for _p in (1, 5, 8):
        VOXEL_RUNS.append((f"one_frame_{_n}-p{_p}", f"one_frame_{_n}", _p, 70000))
for _mv in (1, 255, 256, 257, 2000):  # 2000 = n_points
    VOXEL_RUNS.append((f"one_frame_clip-mv{_mv}", "one_frame_clip", 5, _mv))
for _name in list(BATCH_SIZES) + ["batch_64_frames"]:
    VOXEL_RUNS.append((_name, _name, 5, 20000))
VOXEL_RUNS.append(("batch_chunk_boundaries-mv3", "batch_chunk_boundaries", 5, 3))
VOXEL_RUNS.append(("batch_64_frames-mv3", "batch_64_frames", 3, 3))
for _c in CHANNELS:
    for _p in (1, 8):
        VOXEL_RUNS.append((f"channels_{_c}-p{_p}", f"channels_{_c}", _p, 20000))
VOXEL_RUNS.append(("face", "face", 5, 60000))
VOXEL_RUNS.append(("big_grid", "big_grid", 5, 20000))
VOXEL_RUN_IDS = [r[0] for r in VOXEL_RUNS]


# ------------------------------------------------------------------------------------------------ rulebooks
def corners(shape, batch):
    return np.array([[b, z, y, x] for b in range(batch) for z in (0, shape[0] - 1) for y in (0, shape[1] - 1)
                     for x in (0, shape[2] - 1)], np.int32)


def _sites(rng, shape, batch, n=None, density=0.3, sweep=False):
    """A random subset of the grid in random row order, all eight corners of every frame among them; n rows, or density * cells.
    sweep: rows ordered by the x of the stride-2 output they reach, then along y, with a little noise, so a kernel-3 stride-2 layer's
    outputs are first touched in every chunk of tickets, the last ones included."""
    cells = batch * shape[0] * shape[1] * shape[2]
    n = int(round(density * cells)) if n is None else n
    cor = corners(shape, batch)
    ckey = ((cor[:, 0].astype(np.int64) * shape[0] + cor[:, 1]) * shape[1] + cor[:, 2]) * shape[2] + cor[:, 3]
    ckey = np.unique(ckey)
    if n <= len(ckey):
        key = ckey[:n]
    else:
        rest = np.setdiff1d(np.arange(cells), ckey)
        key = np.concatenate([ckey, rng.choice(rest, size=n - len(ckey), replace=False)])
    key = key[rng.permutation(len(key))]
    co = np.stack([key // (shape[0] * shape[1] * shape[2]), key // (shape[1] * shape[2]) % shape[0], key // shape[2] % shape[1],
                   key % shape[2]], 1).astype(np.int32)
    if sweep:
        co = co[np.argsort((co[:, 3] + 1) // 2 * 200 + co[:, 2] + rng.uniform(0.0, 4.0, len(co)), kind="stable")]
    return co


STRIDED_GEOMETRIES = {  # id: (ksize, stride, pad)
    "k3s2p1": ([3, 3, 3], [2, 2, 2], [1, 1, 1]),
    "k3s2p0": ([3, 3, 3], [2, 2, 2], [0, 0, 0]),
    "k2s2p0": ([2, 2, 2], [2, 2, 2], [0, 0, 0]),
    "k3s1p1": ([3, 3, 3], [1, 1, 1], [1, 1, 1]),
    "k3s3p0": ([3, 3, 3], [3, 3, 3], [0, 0, 0]),
    "k1s2p0": ([1, 1, 1], [2, 2, 2], [0, 0, 0]),
    "k311s211p0": ([3, 1, 1], [2, 1, 1], [0, 0, 0]),
    "k3s2p011": ([3, 3, 3], [2, 2, 2], [0, 1, 1]),
}
SUBM_KERNELS = [[3, 3, 3], [3, 1, 1], [1, 3, 3], [3, 3, 5], [1, 1, 1], [5, 5, 1]]

# name: (shape, batch, n or None for 30 % of the grid, sweep)
SITE_CASES = {
    "few_hundred": ([5, 11, 13], 2, None, False),       # 429 of 1 430 cells: the submanifold kernels
    "odd_grid": ([7, 41, 47], 2, None, False),          # the strided geometries: the last output plane is cut by out_shape
    "kpt_40959": ([8, 80, 80], 2, SUBM_KPT_MIN_ROWS - 1, False),
    "kpt_40960": ([8, 80, 80], 2, SUBM_KPT_MIN_ROWS, False),
    "rows_255": ([5, 11, 13], 2, 255, False),           # x Kc = 8: 2 040 tickets, eight short of a chunk
    "rows_256": ([5, 11, 13], 2, 256, False),           # exactly one chunk
    "rows_257": ([5, 11, 13], 2, 257, False),
    "rows_512": ([5, 11, 13], 2, 512, False),
    "rows_513": ([5, 11, 13], 2, 513, False),
    "rows_1024": ([5, 15, 17], 2, 1024, False),         # x Kc = 2: exactly one chunk
    "rows_1025": ([5, 15, 17], 2, 1025, False),
    "rows_66000": ([9, 99, 101], 2, 66000, True),       # x Kc = 8: 258 chunks
}
# the ticket-scan chunk edges: (site case, geometry, tickets)
CHUNK_RUNS = [(f"rows_{n}", "k3s2p1", n * 8) for n in (255, 256, 257, 512, 513)] + \
             [(f"rows_{n}", "k311s211p0", n * 2) for n in (1024, 1025)] + [("rows_66000", "k3s2p1", 66000 * 8)]

PAD_ROWS = 300  # "live count below capacity": rows [n, n + PAD_ROWS) hold other in-grid sites that must be ignored
KEY_RANGE_SHAPE = [64, 16384, 16383]  # just under 2^34 cells; with b = 63 the keys reach just under 2^40
REFUSED_SHAPE = [64, 16384, 16384]    # 2^34 cells


def _key_range_sites(rng):
    shape = KEY_RANGE_SHAPE
    rows = []
    for b in (0, 63):
        for c in corners(shape, 1):
            z, y, x = int(c[1]), int(c[2]), int(c[3])
            rows.append([b, z, y, x])
            rows.append([b, z + (1 if z == 0 else -1), y, x])                        # a z neighbour of the corner
            rows.append([b, z, y + (1 if y == 0 else -1), x + (1 if x == 0 else -1)])  # a diagonal one
        for _ in range(12):  # pairs of adjacent cells anywhere
            z, y, x = (int(rng.integers(1, s - 1)) for s in shape)
            rows.append([b, z, y, x])
            rows.append([b, z + int(rng.integers(-1, 2)), y + int(rng.integers(-1, 2)), x + 1])
    co = np.unique(np.array(rows, np.int32), axis=0)
    return co[rng.permutation(len(co))]


def _site_case(name):
    rng = _rng(name)
    if name == "key_range":
        return dict(kind="sites", name=name, coords=_key_range_sites(rng), shape=list(KEY_RANGE_SHAPE), batch=64)
    if name == "padded":  # odd_grid's kind of sites with PAD_ROWS further distinct in-grid rows behind the live ones
        shape, batch = [7, 41, 47], 2
        co = _sites(rng, shape, batch, n=2000 + PAD_ROWS)
        return dict(kind="sites", name=name, coords=co, shape=shape, batch=batch, n_live=2000)
    if name == "bad_batch":  # interior rows (every one reaches an output) whose batch index has no key
        shape, batch = [7, 41, 47], 2
        co = _sites(rng, shape, batch, n=1500)
        interior = np.nonzero(np.all((co[:, 1:] >= 2) & (co[:, 1:] <= np.array(shape) - 3), 1))[0]
        bad = interior[rng.choice(len(interior), size=6, replace=False)]
        co[bad, 0] = [64, -1, 64, -1, 64, -1]
        return dict(kind="sites", name=name, coords=co, shape=shape, batch=batch, bad_rows=np.sort(bad))
    shape, batch, n, sweep = SITE_CASES[name]
    return dict(kind="sites", name=name, coords=_sites(rng, shape, batch, n=n, sweep=sweep), shape=list(shape), batch=batch)


_CACHE = {}


def build(name):
    """The case `name`, built once per process; the arrays are shared between the tests and must not be written to."""
    if name not in _CACHE:
        case = _site_case(name) if (name in SITE_CASES or name in ("key_range", "padded", "bad_batch")) else _voxel_case(name)
        for v in case.values():
            for a in (v if isinstance(v, list) else [v]):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _CACHE[name] = case
    return _CACHE[name]
