"""Seeded inputs of the object-noise tests (tests/test_host_object_noise.py, tests/test_gpu_object_noise.py), numpy only.

What the cases are built for.  Two correct implementations in different arithmetic agree on a case only where no decision sits on a
rounding: the tests ask for an IoU margin >= 1e-4 and a face margin >= 1e-4 m (tests/object_noise_ref.py).  The face margin is made
here (points too close to a face of any box are drawn again); the IoU margin is a property of the seed, looked up with the float64
restatement alone and asserted by the tests.

Where the boxes stand.  The tests hold every moved coordinate to 4 float32 ulps OF ITS OWN VALUE.  The roundings of the definition
are not relative to that value but to its intermediates: x - cx (half an ulp of <= 2.5 m: 1.2e-7), cosf / sinf (an ulp or two of 1,
times <= 2.5 m: up to 4e-7), two products and their sum (3.6e-7), then the centre and the translation added back (half an ulp of the
result each) -- at most ~9e-7 m + 1 ulp.  That is below 4 ulps where an ulp is at least 4.8e-7 m, i.e. for |value| >= 4 m; a box
straddling an axis would put results near zero, where the same absolute error is thousands of ulps and the rule says nothing about the
arithmetic.  So the boxes stand at x in [12, 60], |y| in [12, 36] (car-sized: half diagonal < 2.5 m; translations of a few sigma = 1 m
keep every moved x and y beyond 4 m in magnitude -- asserted on the reference's output by the tests).  z moves by one add: half an ulp."""
import numpy as np

from object_noise_ref import inside_distance

CAR_WLH = (1.6, 3.9, 1.56)
MIN_MAGNITUDE = 4.0  # metres: every moved x and y of a compared case (see above)


def make_case(n, T, N, C=4, seed=0, std=(1.0, 1.0, 0.5), rotation=(-0.7853981634, 0.7853981634), pairs=0, stuck=0, face_margin=2e-4):
    """-> points (N, C) f32, boxes (n, 7) f32, trans (n, T, 3) f32, rot (n, T) f32.  Deterministic in the arguments.
    pairs: boxes 2k + 1, k < pairs, are copies of box 2k shifted by 0.5 .. 1 m -- they overlap and share points.
    stuck: the draws of boxes 2k, k < stuck <= pairs, are scaled by 1e-3 -- every try collides with the partner: chosen = -1."""
    rng = np.random.default_rng(120_000 + seed)
    boxes = np.zeros((n, 7))
    boxes[:, 0] = rng.uniform(12, 60, n)
    boxes[:, 1] = rng.uniform(12, 36, n) * rng.choice([-1.0, 1.0], n)
    boxes[:, 2] = rng.uniform(-1.2, -0.6, n)
    boxes[:, 3:6] = np.asarray(CAR_WLH) * rng.uniform(0.9, 1.1, (n, 3))
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, n)
    for k in range(pairs):
        boxes[2 * k + 1] = boxes[2 * k]
        boxes[2 * k + 1, :2] += rng.uniform(0.35, 0.7, 2)
        boxes[2 * k + 1, 6] += rng.uniform(-0.2, 0.2)
    boxes = boxes.astype(np.float32)
    trans = rng.normal(0, std, (n, T, 3))
    rot = rng.uniform(rotation[0], rotation[1], (n, T))
    for k in range(stuck):
        trans[2 * k] *= 1e-3
        rot[2 * k] *= 1e-3
    trans, rot = trans.astype(np.float32), rot.astype(np.float32)

    def draw_points(m):
        p = np.zeros((m, C))
        near = (rng.random(m) < 0.6) & (n > 0)
        k = rng.integers(0, max(n, 1), m)
        b = boxes[k].astype(np.float64) if n else np.zeros((m, 7))
        u, v, w = (rng.uniform(-0.65, 0.65, m) * b[:, 3 + a] for a in range(3))
        c, s = np.cos(b[:, 6]), np.sin(b[:, 6])
        p[:, 0] = np.where(near, b[:, 0] + c * u - s * v, rng.uniform(5, 68, m))
        p[:, 1] = np.where(near, b[:, 1] + s * u + c * v, rng.uniform(-40, 40, m))
        p[:, 2] = np.where(near, b[:, 2] + w, rng.uniform(-2.5, 0.5, m))
        p[:, 3:] = rng.random((m, C - 3))
        return p.astype(np.float32)

    points = draw_points(N)
    for _ in range(100):
        if not N or not n:
            break
        d = np.min([np.abs(inside_distance(points, b)) for b in boxes], 0)
        bad = np.flatnonzero(d < face_margin)
        if not len(bad):
            break
        points[bad] = draw_points(len(bad))
    return points, boxes, trans, rot


# (n, T, N, C, keyword arguments of make_case): the shapes of the GPU comparison.  n = 2 and n = 3: two overlapping boxes that share
# points (wider translations, so that some try frees them).  (65, 7): more than a wave of boxes, 7 tries per round -- one full chunk;
# (65, 9) adds the ragged last chunk and
# (27, 100) (18 tries per round, 100 = 5 * 18 + 10) reaches it through its stuck box; (128, 5) is the largest frame, (3, 256) the most
# tries (4 rounds of 64 for its stuck box).  The seeds are those whose IoU margin (float64 restatement) is >= 1e-4.
GPU_CASES = [
    (2, 2, 257, 4, dict(seed=0, pairs=1, std=(3.0, 3.0, 0.5))),
    (3, 4, 1000, 5, dict(seed=0, pairs=1, std=(2.0, 2.0, 0.5))),
    (27, 100, 4099, 4, dict(seed=0, pairs=2, stuck=1)),
    (65, 7, 513, 5, dict(seed=0, pairs=1)),
    (65, 9, 300, 4, dict(seed=0, pairs=1, stuck=1)),
    (128, 5, 300, 4, dict(seed=0)),
    (3, 256, 200, 4, dict(seed=0, pairs=1, stuck=1)),
]


def _box(x, y, yaw=0.0, z=-1.0):
    return [x, y, z, 2.0, 4.0, 1.5, yaw]  # yaw = 0: 2 m along x, 4 m along y


def _draws(rows):
    """rows: per box a list of tries (dx, dy, dz, rot) -> trans (n, T, 3), rot (n, T) float32."""
    a = np.asarray(rows, np.float32).reshape(len(rows), -1, 4)
    return np.ascontiguousarray(a[:, :, :3]), np.ascontiguousarray(a[:, :, 3])


def _points(boxes, extra=()):
    """Two points inside every box (off centre), one above it, and `extra`; 4 columns."""
    rows = []
    for b in boxes:
        rows += [[b[0] + 0.5, b[1] + 0.25, b[2] + 0.1, 0.5], [b[0] - 0.25, b[1] - 1.5, b[2] - 0.5, 0.25], [b[0], b[1], b[2] + 2.0, 0.75]]
    rows += [list(e) for e in extra]
    return np.asarray(rows, np.float32).reshape(-1, 4)


def hand_cases():
    """name -> (points, boxes, trans, rot, expected chosen).  Axis-aligned 2 x 4 m boxes around (20, 20); overlaps are whole decimetres,
    so every margin is large."""
    far = (0.0, 9.0, 0.0, 0.0)
    out = {}
    # box 0: try 0 pushes it 0.5 m into box 1 (IoU 2 / 14), try 1 is free; box 1 then keeps its try 0, a quarter turn in place
    boxes = [_box(20, 20), _box(23, 20)]
    out["second_try"] = (_points(boxes), boxes, *_draws([[(1.5, 0, 0, 0), (-1, 0.5, 0.125, 0.5)], [(0, 0, 0.25, np.pi / 2), far]]), [1, 0])
    # every try of box 0 collides; box 1 (tries far away) moves
    out["all_collide"] = (_points(boxes), boxes, *_draws([[(1.5, 0, 0, 0), (2, 0.5, 0, 0.25)], [far, far]]), [-1, 0])
    out["one_try"] = (_points(boxes), boxes, *_draws([[(1.5, 0, 0, 0)], [(0, 5, 0, 0.25)]]), [-1, 0])
    out["no_boxes"] = (_points([_box(20, 20)]), np.zeros((0, 7), np.float32), np.zeros((0, 3, 3), np.float32), np.zeros((0, 3), np.float32), [])
    # j < i is read MOVED: box 0 leaves (try 0: 5 m to the left); box 1's try 0 lands on box 0's ORIGINAL place, which is free by then
    boxes = [_box(20, 20), _box(24, 20), _box(40, 20)]
    idle = (0.0, 0.0, 0.0, 0.0)
    out["earlier_box_moved_away"] = (_points(boxes), boxes, *_draws([[(-5, 0, 0, 0), far], [(-2.5, 0, 0, 0), far], [idle, far]]), [0, 0, 0])
    # ... and the reverse: box 0 moves next to box 1 (free against box 1's original pose); box 1's try 0 (stay) collides with box 0's MOVED
    # pose, not with its original one, so box 1 takes try 1
    out["earlier_box_moved_in"] = (_points(boxes), boxes, *_draws([[(1.0, 0, 0, 0), far], [(-1.5, 0, 0, 0), far], [idle, far]]), [0, 1, 0])
    # j > i is read ORIGINAL: box 0's try 0 lands on box 2's original place and collides, although box 2 moves away later
    out["later_box_original"] = (_points(boxes), boxes, *_draws([[(19.5, 0, 0, 0), far], [idle, far], [(0, -9, 0, 0), far]]), [1, 0, 0])
    return {k: (v[0], np.asarray(v[1], np.float32).reshape(-1, 7), v[2], v[3], np.asarray(v[4], np.int64)) for k, v in out.items()}
