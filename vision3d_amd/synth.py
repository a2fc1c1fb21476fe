"""Seeded synthetic lidar sweeps shaped like the clouds the reference consumes.

There is no KITTI data in this environment, so bench.py, the tests and smoke() use this ray-cast
generator (spec: SURVEY.md section 8(d)).  A sweep is what `dataset/kitti_dataset.py:135-140`
hands to the preprocessor: float32 (N, 4) = x, y, z, intensity, already cropped to GRID_BOUNDS.

Scene: sensor at the origin, ground plane z = -1.73 m, two walls parallel to the x axis and a set of
axis-aligned car-sized boxes; nearest hit per ray, gaussian range noise, half-open crop to the grid
bounds, shuffle, first `n_points`.
"""
import numpy as np

KITTI_BOUNDS = (0.0, -40.0, -3.0, 70.4, 40.0, 1.0)
WAYMO_BOUNDS = (-75.2, -75.2, -2.0, 75.2, 75.2, 4.0)
CAR_WLH = (1.6, 3.9, 1.56)


def _ray_scene(rng, az, el, n_cars, x_rng, y_rng, wall_rng):
    """Return (hit points (R,3), hit mask (R,), car boxes (n_cars,7) as x,y,z,w,l,h,yaw)."""
    a, e = np.meshgrid(az, el, indexing="ij")
    a, e = a.ravel(), e.ravel()
    d = np.stack([np.cos(e) * np.cos(a), np.cos(e) * np.sin(a), np.sin(e)], 1)
    big = 1e9
    t = np.full(d.shape[0], big)
    # ground
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = np.where(d[:, 2] < 0, -1.73 / d[:, 2], big)
    t = np.minimum(t, tg)
    # walls y = +-yw, 4 m tall from the ground
    for sgn in (+1.0, -1.0):
        yw = sgn * rng.uniform(*wall_rng)
        with np.errstate(divide="ignore", invalid="ignore"):
            tw = np.where(d[:, 1] * sgn > 1e-9, yw / d[:, 1], big)
        zw = tw * d[:, 2]
        tw = np.where((zw >= -1.73) & (zw <= 2.27), tw, big)
        t = np.minimum(t, tw)
    # axis-aligned cars (random 90 degree swap of footprint)
    w, l, h = CAR_WLH
    boxes = np.zeros((n_cars, 7))
    for i in range(n_cars):
        cx, cy = rng.uniform(*x_rng), rng.uniform(*y_rng)
        swap = rng.random() < 0.5
        sx, sy = (w, l) if swap else (l, w)  # extent along x / y
        boxes[i] = (cx, cy, -0.95, w, l, h, np.pi / 2 if swap else 0.0)
        lo = np.array([cx - sx / 2, cy - sy / 2, -0.95 - h / 2])
        hi = np.array([cx + sx / 2, cy + sy / 2, -0.95 + h / 2])
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = lo / d, hi / d
        tn = np.nanmax(np.minimum(t0, t1), 1)
        tf = np.nanmin(np.maximum(t0, t1), 1)
        tb = np.where((tn <= tf) & (tn > 0), tn, big)
        t = np.minimum(t, tb)
    hit = t < big
    t = t + rng.normal(0.0, 0.02, t.shape)
    return d * t[:, None], hit, boxes


def _morton_key(pts, bounds, vs=(0.05, 0.05, 0.1)):
    c = np.floor((pts[:, :3].astype(np.float32) - np.asarray(bounds[:3], np.float32)) / np.asarray(vs, np.float32)).astype(np.int64)
    key = np.zeros(pts.shape[0], np.uint64)
    for j in range(3):
        x = c[:, j].astype(np.uint64)
        for i in range(13):
            key |= ((x >> np.uint64(i)) & np.uint64(1)) << np.uint64(3 * i + j)
    return key


def make_cloud(seed=0, n_points=16384, bounds=KITTI_BOUNDS, fov_deg=45.0, az_steps=1000, n_beams=64,
               n_cars=12, return_boxes=False, order="shuffled"):
    """One synthetic sweep, float32 (n_points, 4).  Deterministic in `seed`.

    order="shuffled" (default; what every test and golden fixture uses): the returns in random order -- what the TRAINING
    dataset hands over (`kitti_dataset.py:154` shuffles the points).  order="scan": the SAME returns in firing order (azimuth
    step by azimuth step, 64 beams each) -- what the inference dataset hands over (`kitti_dataset.py:135-140`: `read_velo`,
    the .bin file in sensor order)."""
    rng = np.random.default_rng(seed)
    bounds = np.asarray(bounds, np.float64)
    x_rng = (max(bounds[0], -65.0) + 6.0, min(bounds[3], 71.0) - 5.4) if bounds[0] >= 0 else (bounds[0] + 8, bounds[3] - 8)
    y_rng = (-25.0, 25.0) if bounds[1] >= -40.0 else (bounds[1] + 8, bounds[4] - 8)
    el = np.deg2rad(np.linspace(-24.8, 2.0, n_beams))
    steps = az_steps
    while True:
        sub = np.random.default_rng(rng.integers(1 << 31))
        az = np.deg2rad(np.linspace(-fov_deg, fov_deg, steps, endpoint=(fov_deg < 180.0)))
        pts, hit, boxes = _ray_scene(sub, az, el, n_cars, x_rng, y_rng, (10.0, 22.0))
        pts = pts[hit].astype(np.float32)
        lo, hi = bounds[:3].astype(np.float32), bounds[3:].astype(np.float32)
        keep = np.all((pts >= lo) & (pts < hi), 1)
        pts = pts[keep]
        if pts.shape[0] >= n_points:
            break
        steps *= 2  # denser azimuth sampling until the crop holds enough returns
    if order in ("scan", "morton"):  # the same subset as the shuffled sweep (same generator draws), restored to firing order
        sel = np.arange(pts.shape[0])
        sub.shuffle(sel)
        pts = pts[np.sort(sel[:n_points])]
        if order == "morton":  # (experiments: the returns sorted by the 3-D Morton key of their 0.05 x 0.05 x 0.1 m cell, stable)
            pts = pts[np.argsort(_morton_key(pts, bounds), kind="stable")]
    else:
        sub.shuffle(pts)
        pts = pts[:n_points]
    inten = sub.uniform(0.0, 1.0, (pts.shape[0], 1)).astype(np.float32)
    cloud = np.ascontiguousarray(np.concatenate([pts, inten], 1), dtype=np.float32)
    if return_boxes:
        return cloud, boxes.astype(np.float32)
    return cloud


def make_kitti_batch(batch_size=1, seed0=0, n_points=16384):
    return [make_cloud(seed0 + i, n_points) for i in range(batch_size)]


def make_waymo_cloud(seed=0, n_points=180000, order="shuffled"):
    """configs[4]: 360 degree sweep, 0.05 m voxels over +-75.2 m (HBM-bound stress case)."""
    return make_cloud(seed, n_points, WAYMO_BOUNDS, fov_deg=180.0, az_steps=3000, n_beams=64, n_cars=40, order=order)


CLASS_WLH = (CAR_WLH, (0.6, 0.8, 1.73), (0.6, 1.76, 1.73))  # the default anchors' sizes (core/config.py)


ROI_LEVELS_FG = (0, 0, 0, 0, 0, 0, 0, 1, 2, 3)  # per ten RoIs: seven at the small noise level, one medium, one large, one far away
ROI_LEVELS_BG = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3)


def jitter_rois(gt, topk, rng, levels=ROI_LEVELS_FG):
    """`topk` RoIs made from the ground truths `gt` (g, 7), walking through them in turn: offsets and size changes of ~2 %, ~10 %
    and ~25 % of the box dimensions (levels 0, 1, 2), or moved hundreds of metres away (level 3: overlaps nothing); RoI i of ten
    is at `levels[i % 10]`.  Each ground truth is the source of some RoI once topk >= 10 g."""
    base = np.array([0.02, 0.10, 0.25])
    out = np.zeros((topk, 7), np.float32)
    for i in range(topk):
        src, lvl = gt[(i // len(levels)) % len(gt)], levels[i % len(levels)]
        roi = np.array(src, np.float64)
        if lvl == 3:
            roi[:2] += rng.choice([-1.0, 1.0], 2) * rng.uniform(200, 300, 2)
        else:
            amp = base[lvl] * rng.uniform(0.5, 1.5, 7) * rng.choice([-1.0, 1.0], 7)
            roi[0:3] += amp[0:3] * src[3:6]
            roi[3:6] *= np.exp(amp[3:6])
            roi[6] += amp[6]
        out[i] = roi
    return out


def make_refine_case(seed=0, n_cls=1, batch=1, topk=100, gt_per_class=8):
    """Inputs of the stage-2 target assignment: per frame `gt_per_class` ground truths of every class, and RoIs in the
    (n_cls, topk) group-major layout of PV_RCNN.stage1_proposals made by `jitter_rois` from the ground truths of the group's class.
    Even frames are mostly foreground, odd frames mostly background.
    -> proposals (batch, n_cls * topk, 7) f32, proposal_class (n_cls * topk,) i64, boxes / class_idx per-frame lists, draws
    (batch, n_cls * topk) f32 in [0, 1).  Deterministic in `seed`."""
    rng = np.random.default_rng(70_000 + seed)
    proposals = np.zeros((batch, n_cls * topk, 7), np.float32)
    boxes, class_idx = [], []
    for b in range(batch):
        g = n_cls * gt_per_class
        gt = np.zeros((g, 7))
        cls = np.repeat(np.arange(n_cls), gt_per_class)
        gt[:, 0], gt[:, 1], gt[:, 2] = rng.uniform(5, 65, g), rng.uniform(-30, 30, g), rng.uniform(-1.2, -0.7, g)
        gt[:, 3:6] = np.asarray(CLASS_WLH)[cls % 3] * rng.uniform(0.9, 1.1, (g, 3))
        gt[:, 6] = rng.uniform(-np.pi, np.pi, g)
        for c in range(n_cls):
            proposals[b, c * topk:(c + 1) * topk] = jitter_rois(gt[cls == c], topk, rng, ROI_LEVELS_FG if b % 2 == 0 else ROI_LEVELS_BG)
        boxes.append(gt.astype(np.float32))
        class_idx.append(cls.astype(np.int64))
    proposal_class = np.repeat(np.arange(n_cls), topk).astype(np.int64)
    draws = rng.random((batch, n_cls * topk)).astype(np.float32)
    return proposals, proposal_class, boxes, class_idx, draws


def make_gt_boxes(seed=0, n_extra=15):
    """GT boxes (n,7) for the train configuration: the scene's cars + `n_extra` sampled ones
    (configs/second/car.yaml:18 AUG.NUM_SAMPLE_OBJECTS)."""
    _, boxes = make_cloud(seed, return_boxes=True)
    rng = np.random.default_rng(10_000 + seed)
    extra = np.zeros((n_extra, 7), np.float32)
    extra[:, 0] = rng.uniform(6, 65, n_extra)
    extra[:, 1] = rng.uniform(-25, 25, n_extra)
    extra[:, 2] = -0.95
    extra[:, 3:6] = np.asarray(CAR_WLH, np.float32) * rng.uniform(0.9, 1.1, (n_extra, 3))
    extra[:, 6] = rng.uniform(-np.pi, np.pi, n_extra)
    return np.concatenate([boxes, extra], 0).astype(np.float32)


def make_keypoint_case(seed=0, batch=2, n_points=1500, n_sectors=6, n_proposals=5, counts=None, r_range=(5.0, 25.0), margin=1e-3):
    """Inputs of the sectorized keypoint sampling (pointnet2_utils.sector_point_sample): -> points (batch, n_points, 4) f32,
    proposals (batch, n_proposals, 7) f32.  Points are drawn in polar form -- a sector, a position inside it, a range from
    `r_range`, z in [-2, 1) -- and shuffled; `counts` (n_sectors ints summing to n_points) fixes how many fall into each sector
    (default: a random share each).  Every point's azimuth * n_sectors / 2 pi, evaluated in float64 on the float32 coordinates,
    stays at least `margin` away from an integer (offenders are drawn again), so that two fp32 atan2 implementations agree on every
    sector.  Proposals: car-sized boxes centred on points of the frame.  Deterministic in `seed`."""
    rng = np.random.default_rng(90_000 + seed)
    S = int(n_sectors)
    points = np.zeros((batch, n_points, 4), np.float32)
    proposals = np.zeros((batch, n_proposals, 7), np.float32)
    for b in range(batch):
        if counts is None:
            sec = rng.choice(S, n_points, p=rng.dirichlet(np.full(S, 2.0)))
        else:
            assert len(counts) == S and sum(counts) == n_points
            sec = np.repeat(np.arange(S), counts)
        rng.shuffle(sec)
        xyz = np.zeros((n_points, 3), np.float32)
        todo = np.arange(n_points)
        while len(todo):
            t = sec[todo] + rng.uniform(0.02, 0.98, len(todo))
            az = t / S * 2 * np.pi - np.pi
            r = rng.uniform(r_range[0], r_range[1], len(todo))
            xyz[todo] = np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-2.0, 1.0, len(todo))], 1).astype(np.float32)
            got = (np.arctan2(xyz[todo, 1].astype(np.float64), xyz[todo, 0].astype(np.float64)) + np.pi) * (S / (2 * np.pi))
            bad = (np.abs(got - np.round(got)) < 10 * margin) | (np.floor(got) != sec[todo])
            todo = todo[bad]
        points[b, :, :3] = xyz
        points[b, :, 3] = rng.uniform(0.0, 1.0, n_points)
        if n_proposals:
            centre = xyz[rng.integers(0, n_points, n_proposals)] + rng.normal(0.0, 0.3, (n_proposals, 3))
            proposals[b, :, :3] = centre
            proposals[b, :, 3:6] = np.asarray(CAR_WLH) * rng.uniform(0.8, 1.25, (n_proposals, 3))
            proposals[b, :, 6] = rng.uniform(-np.pi, np.pi, n_proposals)
    return points, proposals
