"""Seeded inputs of the centre-head tests (tests/test_host_center_head.py, tests/test_gpu_center_head.py), numpy only.

Two correct implementations in different arithmetic agree on a case only where no decision sits on a rounding.  The compared cases keep
these margins (looked up with the float64 restatement, tests/center_head_ref.py):
    fx, fy of a live object            >= 1e-3 from an integer        (the floor that picks the cell)
    min(r1, r2, r3)                    >= 1e-6 from an integer        (the truncation that picks the radius)
    |pred - target|                    >= 1e-3 for every masked box component   (the sign of the L1 gradient)
    heat logits                        all distinct                   (peak tests and the top-k order)
The generator makes the first, third and fourth by construction -- positions are drawn as cell + U(0.05, 0.95), predictions at an
object's cell as (largest target of the cell's objects) + U(0.05, 1) or (smallest) - U(0.05, 1), logits as a permutation of a grid --
because drawing them freely would reject far more than the 2 % the tests allow (ten objects put twenty coordinates within 1e-3 of
an integer 4 % of the time; 10^5 normal float32 draws always hold a repeated value).  A draw that still misses a margin is rejected
and the next seed of the sequence is drawn; `draw_stats` counts both."""
import numpy as np

import center_head_ref as R

PX = PY = 0.4
CAR, PED, TRUCK = (1.6, 3.9, 1.56), (0.6, 0.8, 1.73), (3.0, 12.0, 3.5)  # radii 2 (the minimum), 2 and 6 cells


def geometry(H, W):
    """(px, py, x_lo, y_lo) of an (H, W) map: x from 0, y centred; the half cell beyond the map keeps the grid count off a rounding."""
    return (PX, PY, 0.0, -0.5 * PY * (H + 0.5))


def distinct_grid(rng, shape, lo, hi):
    """A random arrangement of a regular float32 grid over (lo, hi): all values distinct."""
    n = int(np.prod(shape))
    vals = ((rng.permutation(n) + 0.5) / n * (hi - lo) + lo).astype(np.float32)
    assert len(np.unique(vals)) == n
    return vals.reshape(shape)


def _box(rng, geom, ix, iy, wlh=None, scale=(0.85, 1.15)):
    px, py, x_lo, y_lo = geom
    fx, fy = ix + rng.uniform(0.05, 0.95), iy + rng.uniform(0.05, 0.95)
    if wlh is None:
        wlh = (rng.uniform(0.5, 2.2), rng.uniform(0.7, 4.5), rng.uniform(1.4, 1.9))
    w, l, h = np.asarray(wlh) * rng.uniform(*scale, 3)
    return [fx * px + x_lo, fy * py + y_lo, rng.uniform(-1.5, 0.0), w, l, h, rng.uniform(-np.pi, np.pi)]


def draw_targets(H, W, seed, n_cls=2):
    """-> boxes [3 x (n_b, 7) float32], class_idx [3 x (n_b,) int32] of one draw.  Frame 0: windows clipped at each of the four borders
    and at a corner, two same-class objects with overlapping windows, two same-class objects in one cell, one object outside the grid,
    one of class n_cls, one with w = 0, a few free ones; frame 1: empty; frame 2: free objects, two objects of different classes in
    one cell and a truck."""
    rng = np.random.default_rng(310_000 + seed)
    g = geometry(H, W)
    cell = lambda: (int(rng.integers(3, W - 3)), int(rng.integers(3, H - 3)))
    b0, c0 = [], []
    for ix, iy in ((0, H // 2), (W - 1, H // 3), (W // 2, 0), (W // 3, H - 1), (W - 1, H - 1)):
        b0.append(_box(rng, g, ix, iy, CAR)), c0.append(0)
    ix, iy = cell()
    b0 += [_box(rng, g, ix, iy, CAR), _box(rng, g, min(ix + 2, W - 1), iy, CAR)]  # overlapping windows, same class
    c0 += [1, 1]
    ix, iy = cell()
    b0 += [_box(rng, g, ix, iy, PED), _box(rng, g, ix, iy, PED)]  # one cell, same class
    c0 += [1, 1]
    out = _box(rng, g, 2, 2, CAR)
    out[0] = g[2] - 3.0  # left of the grid
    b0.append(out), c0.append(0)
    b0.append(_box(rng, g, *cell(), CAR)), c0.append(n_cls)  # a class the head does not have
    flat = _box(rng, g, *cell(), CAR)
    flat[3] = 0.0
    b0.append(flat), c0.append(0)
    for _ in range(3):
        b0.append(_box(rng, g, *cell())), c0.append(int(rng.integers(0, n_cls)))
    b2, c2 = [], []
    for _ in range(5):
        b2.append(_box(rng, g, *cell())), c2.append(int(rng.integers(0, n_cls)))
    ix, iy = cell()
    b2 += [_box(rng, g, ix, iy, CAR), _box(rng, g, ix, iy, PED)]  # one cell, two classes
    c2 += [0, 1]
    b2.append(_box(rng, g, *cell(), TRUCK)), c2.append(0)  # a window of 13 x 13 cells
    boxes = [np.asarray(b0, np.float32), np.zeros((0, 7), np.float32), np.asarray(b2, np.float32)]
    return boxes, [np.asarray(c0, np.int32), np.zeros(0, np.int32), np.asarray(c2, np.int32)]


def draw_maps(H, W, seed, n_cls, B, tgt=None):
    """Fused maps (B, n_cls + 8, H, W) float32: heat logits a permutation of a grid over (-4, 4), z a permutation of a grid over
    (-2, 1) (distinct too: the tests find a decoded box's cell by its z, which decode copies), the other channels normal draws.
    tgt (the reference's targets): the box channels at every masked object's cell are set off the cell's targets (see above)."""
    rng = np.random.default_rng(320_000 + seed)
    maps = rng.normal(0, 0.5, (B, n_cls + 8, H, W)).astype(np.float32)
    maps[:, :n_cls] = distinct_grid(rng, (B, n_cls, H, W), -4.0, 4.0)
    maps[:, n_cls + 2] = distinct_grid(rng, (B, H, W), -2.0, 1.0)
    if tgt is not None:
        flat = maps.reshape(B, n_cls + 8, H * W)
        for b in range(B):
            for cell in np.unique(tgt["ind"][b][tgt["mask"][b] > 0]):
                rows = tgt["reg"][b][(tgt["ind"][b] == cell) & (tgt["mask"][b] > 0)]
                up = rng.random(8) < 0.5
                off = rng.uniform(0.05, 1.0, 8)
                flat[b, n_cls:, cell] = np.where(up, rows.max(0) + off, rows.min(0) - off).astype(np.float32)
    return maps


draw_stats = dict(drawn=0, rejected=0)


def margins_ok(tgt, maps, n_cls):
    logits = maps[:, :n_cls]
    ref = R.loss(maps, tgt["heat"], tgt["ind"], tgt["mask"], tgt["reg"], n_cls)
    return bool(tgt["fmargin"] >= 1e-3 and tgt["rmargin"] >= 1e-6 and ref["reg_margin"] >= 1e-3
                and len(np.unique(logits)) == logits.size), ref


def train_case(H, W, seed=0, n_cls=2):
    """The first draw of the sequence seed, seed + 1000, ... that keeps every margin -> dict(boxes, class_idx, geom, n_cls, H, W, maps,
    tgt: the reference's targets, loss: the reference's loss and gradient)."""
    for attempt in range(20):
        boxes, class_idx = draw_targets(H, W, seed + 1000 * attempt, n_cls)
        tgt = R.targets(boxes, class_idx, n_cls, H, W, geometry(H, W))
        maps = draw_maps(H, W, seed + 1000 * attempt, n_cls, len(boxes), tgt)
        ok, ref = margins_ok(tgt, maps, n_cls)
        draw_stats["drawn"] += 1
        if ok:
            return dict(boxes=boxes, class_idx=class_idx, geom=geometry(H, W), n_cls=n_cls, H=H, W=W, maps=maps, tgt=tgt, loss=ref)
        draw_stats["rejected"] += 1
    raise AssertionError("no draw kept its margins")


TRAIN_SHAPES = [(20, 24), (33, 47)]  # neither a multiple of the 256-cell tile; 1 551 cells: seven tiles, the last one ragged


def decode_case(name):
    """-> dict(maps, n_cls, geom, topk, ref: the reference's decode).
    train_20x24 / train_33x47: the maps of the training cases (fewer / more than TOPK peaks per group);  pads: an 8 x 8 map, TOPK 100;
    tie: 8 x 8 with two equal adjacent logits above all others -- both peaks, the lower cell first;  slices: 200 x 176, n_cls 3, B 1,
    nine slices of 4 096 cells in the selection, the last one ragged."""
    if name.startswith("train_"):
        H, W = (int(v) for v in name[6:].split("x"))
        maps, n_cls, topk = train_case(H, W)["maps"], 2, 100
    elif name in ("pads", "tie"):
        H, W, n_cls, topk = 8, 8, 2, 100
        maps = draw_maps(H, W, 7 if name == "pads" else 8, n_cls, 3)
        if name == "tie":
            maps[1, 0, 3, 4] = maps[1, 0, 3, 5] = 5.0  # cells 28 and 29 of frame 1, class 0
            maps[2, 1, 7, 7] = maps[2, 1, 6, 6] = 4.5  # a diagonal pair in the corner: cells 54 and 63
    elif name == "slices":
        H, W, n_cls, topk = 200, 176, 3, 100
        maps = draw_maps(H, W, 9, n_cls, 1)
    else:
        raise KeyError(name)
    geom = geometry(H, W)
    return dict(maps=maps, n_cls=n_cls, geom=geom, topk=topk, H=H, W=W, ref=R.decode(maps, n_cls, geom, topk))


DECODE_CASES = ["train_20x24", "train_33x47", "pads", "tie", "slices"]
