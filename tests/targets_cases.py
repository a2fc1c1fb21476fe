"""Seeded inputs for anchor target assignment (csrc/targets.hip) at its staging, band, tie and stride edges; shared by
tests/test_host_targets_ref.py, which proves on the reference alone that every case has the property it is named for, and
tests/test_gpu_targets_edges.py.  `case(name)` -> dict(gt (n, 7) f32, gt_class (n,) i64, anchors (n_cls, A, 7) f32, thresh (n_cls, 2)
f32, low_quality[, cfg = (n_cls, anchor yaws) for the cases whose anchors are an AnchorGenerator grid: make_cfg(*cfg)]); cached,
read-only.  `reference(name, low_quality)` is the float64 result of tests/targets_ref.py, computed once per process.

The anchors are hand-made and go straight to the C entry, so A is free and rows may repeat.  A "lattice" is car-sized anchors 0.9 m x
1.7 m apart in rows of ceil(sqrt(A)), every centre jittered by up to 0.15 m (no two IoUs tie by symmetry), yaws 0 and 1.5708
alternating; anchor i belongs to workgroup i // 256.

  grid-A{1,63,64,65,255,256,257,513}   one class, three ground truths; from 257 on, ground truth 0 lies between anchors 255 and 256
  band-{at_lo,at_hi,above_lo,above_hi}  a 2 x 2 anchor strictly inside a 4 x 4 ground truth: IoU = 0.25 exactly, in fp32 and float64
  first_max, first_max-reversed         two ground truths of one BEV rectangle (z and h differ), one of another class between them
  interleaved-c{3,16}                   classes round-robin in the input, class 1 empty, ids -1 and n_cls present
  low_quality-{clear,dup_anchors,far_gt,below_lo}   a best IoU under lo; its anchor twice (rows 3 and 300); a ground truth 50 m away;
                                        nothing but such ground truths
  crowd-{128,129,200,257}, crowd-mixed  that many cars on a line, the last one decisive; 200 boxes of three classes, 130 of them cars
  encode-{yaw,size}                     yaw differences at 0, -1e-7, +-(float)pi, +-2 (float)pi, +-3.5; size ratios 1/8 .. 8
  empty, stale-{high,low}               no ground truth; two frames of one shape for the workspace reuse
"""
import functools

import numpy as np

import targets_ref as ref

F = np.float32
CAR = (1.6, 3.9, 1.56)
CAR_THRESH = (0.45, 0.6)
GRID_SIZES = [1, 63, 64, 65, 255, 256, 257, 513]
CROWD_SIZES = [128, 129, 200, 257]
YAW_DIFFS = [0.0, -1e-7, ref.PI32, -ref.PI32, 2 * ref.PI32, -2 * ref.PI32, 3.5, -3.5]
SIZE_RATIOS = [(0.125, 0.125, 0.125), (0.25, 0.5, 8.0), (0.5, 0.25, 4.0), (2.0, 4.0, 0.25), (4.0, 2.0, 0.5), (8.0, 8.0, 8.0)]
BAND = {"at_lo": ((0.25, 0.6), -1), "at_hi": ((0.125, 0.25), 1),
        "above_lo": ((float(np.nextafter(F(0.25), F(1))), 0.6), 0), "above_hi": ((0.125, float(np.nextafter(F(0.25), F(1)))), -1)}
MIXED_YAWS = (0.0, 35.0)
BAND_SHIFTS = [(0.0, 0.0), (16.0, 0.0), (0.0, -32.0), (64.0, 64.0), (-128.0, 32.0)]

# a seed per case, chosen on the host: tests/test_host_targets_ref.py asserts the margins
SEEDS = {"interleaved-c16": 2, "stale": 1, "grid-A65": 1}


def _rng(name):
    return np.random.default_rng([20263, sum(ord(ch) * (i + 1) for i, ch in enumerate(name)), SEEDS.get(name, 0)])


def lattice(rng, A, size=CAR, origin=(0.0, 0.0), z=-1.0):
    """(A, 7) float32"""
    cols = int(np.ceil(np.sqrt(A)))
    i = np.arange(A)
    out = np.zeros((A, 7))
    out[:, 0] = origin[0] + 0.9 * (i % cols) + rng.uniform(-0.15, 0.15, A)
    out[:, 1] = origin[1] + 1.7 * (i // cols) + rng.uniform(-0.15, 0.15, A)
    out[:, 2] = z
    out[:, 3:6] = size
    out[:, 6] = np.where(i % 2 == 0, 0.0, 1.5708)
    return out.astype(F)


def near(anchor, dx, dy, yaw, scale=1.0, dz=0.1):
    """a ground truth of the anchor's size times `scale`, its centre moved by (dx, dy, dz)"""
    b = np.array(anchor, np.float64)
    b[0] += dx
    b[1] += dy
    b[2] += dz
    b[3:6] *= scale
    b[6] = yaw
    return b


def _pack(gt, gt_class, anchors, thresh, low_quality, **extra):
    out = dict(gt=np.ascontiguousarray(np.asarray(gt, np.float64).reshape(-1, 7), F), gt_class=np.asarray(gt_class, np.int64).reshape(-1),
               anchors=np.ascontiguousarray(anchors, F), thresh=np.asarray(thresh, F).reshape(-1, 2), low_quality=bool(low_quality), **extra)
    assert out["anchors"].ndim == 3 and out["thresh"].shape[0] == out["anchors"].shape[0] and len(out["gt"]) == len(out["gt_class"])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _grid(rng, A):
    an = lattice(rng, A)
    if A == 1:  # all three on the one anchor, at three different overlaps
        gt = [near(an[0], 0.1, 0.2, 0.3), near(an[0], 0.5, -0.9, -2.0), near(an[0], -0.9, 1.5, 40.0)]
    else:
        # ground truth 0 between two anchors that are neighbours in a row: 255 | 256 where they exist (two workgroups), else 0 | 1
        right, cols = 256 if A >= 257 else 1, int(np.ceil(np.sqrt(A)))
        step = an[right - 1, :2].astype(np.float64) - an[right, :2]
        gt = [near(an[right], 0.4 * step[0], 0.4 * step[1], 0.05),
              near(an[A // 2], 0.07, -0.11, 40.0, scale=1.05),  # a real turn: 40 degrees
              near(an[cols - 1], 0.5, -1.3, -3.0)]              # off the first row's end: a best IoU under lo
    return _pack(gt, [0, 0, 0], an[None], [CAR_THRESH], True)


def _band(which):
    thresh, _ = BAND[which]
    an, gt = [], []
    for sx, sy in BAND_SHIFTS:
        an.append([sx, sy, 0.0, 2.0, 2.0, 1.5, 0.0])
        gt.append([sx + 0.5, sy + 0.5, 0.0, 4.0, 4.0, 1.5, 0.0])
    return _pack(gt, [0] * len(gt), np.asarray(an)[None], [thresh], False)


def _first_max(rng, reverse):
    an0 = lattice(rng, 70)
    an1 = lattice(rng, 70, size=(0.6, 0.8, 1.73), z=-0.6)
    first = near(an0[33], 0.06, 0.1, 0.2, dz=0.1)
    second = first.copy()
    second[2] += 0.3  # the same BEV rectangle: the IoUs are the same numbers; z and h tell the two apart in G_reg
    second[5] *= 1.25
    other = near(an1[12], 0.02, 0.03, 1.0)
    pair = (second, first) if reverse else (first, second)
    return _pack([pair[0], other, pair[1]], [0, 1, 0], np.stack([an0, an1]), [CAR_THRESH, (0.2, 0.35)], False)


def _interleaved(rng, n_cls):
    sizes = [(1.6 - 0.05 * c, 3.9 - 0.15 * c, 1.56 + 0.02 * c) for c in range(n_cls)]
    anchors = np.stack([lattice(rng, 70, size=sizes[c]) for c in range(n_cls)])
    order = [c for c in range(n_cls) if c != 1] + [-1, n_cls]  # class 1 has no ground truth; two ids belong to no class
    gt, cls = [], []
    for i in range(2 * len(order)):
        c = order[i % len(order)]
        a = anchors[min(max(c, 0), n_cls - 1)][(7 * i + 3) % 70]
        gt.append(near(a, rng.uniform(-0.3, 0.3), rng.uniform(-0.6, 0.6), rng.uniform(-3.0, 3.0), scale=rng.uniform(0.9, 1.1)))
        cls.append(c)
    return _pack(gt, cls, anchors, [(0.45 - 0.01 * c, 0.6 - 0.01 * c) for c in range(n_cls)], True)


def _low_quality(rng, which):
    A = 320 if which == "dup_anchors" else 70
    an = lattice(rng, A)
    gt = []
    if which != "below_lo":
        gt.append(near(an[A // 2 + 1], 0.05, -0.08, 0.1))  # a clear positive
    gt.append(near(an[3], 0.1, -1.9, -0.2))  # below the first row: anchor 3 is its best, at about 0.3
    if which == "dup_anchors":
        an[300] = an[3]
    if which == "far_gt":
        gt.append(near(an[0], -50.0, -50.0, 0.4))
    if which == "below_lo":
        gt.append(near(an[A - 4], -0.12, 1.8, 3.0))  # above the last row
    return _pack(gt, [0] * len(gt), an[None], [CAR_THRESH], True)


def make_cfg(n_cls, yaws=None, low_quality=False):
    """direction_cases.make_cfg(n_cls, bounds=TARGET_BOUNDS) -- 5 x 7 cells, two yaws: A = 70 per class, direction head on --, optionally
    with other anchor yaws"""
    import direction_cases
    cfg = direction_cases.make_cfg(n_cls, bounds=direction_cases.TARGET_BOUNDS)
    cfg.ALLOW_LOW_QUALITY_MATCHES = bool(low_quality)
    if yaws is not None:
        for a in cfg.ANCHORS:
            a["yaw"] = list(yaws)
    return cfg


def _cfg_anchors(n_cls, yaws=None):
    from vision3d_amd.core.anchor_generator import AnchorGenerator
    cfg = make_cfg(n_cls, yaws)
    return AnchorGenerator(cfg).anchors.numpy().reshape(n_cls, 70, 7), [a["iou_thresh"] for a in cfg.ANCHORS[:n_cls]]


def _crowd(rng, n):
    """n cars on a line 3 m apart along x; only the last one reaches the anchor grid (x in 0.2 .. 2.7)"""
    anchors, thresh = _cfg_anchors(1)
    gt = np.zeros((n, 7))
    gt[:, 0] = 1.5 - 3.0 * np.arange(n - 1, -1, -1)
    gt[:, 1] = 0.1
    gt[:, 2] = -1.0 + rng.uniform(-0.2, 0.2, n)
    gt[:, 3:6] = np.asarray(CAR) * rng.uniform(0.95, 1.05, (n, 3))
    gt[:, 6] = rng.uniform(-3.0, 3.0, n)
    gt[-1, 3:6] = CAR
    return _pack(gt, np.zeros(n), anchors, thresh, False, cfg=(1, None))


def _crowd_mixed(rng):
    """200 boxes on the anchor grid of the 3-class configuration: 130 of class 0, 30 of class 1, 40 of class 2, interleaved.  Every
    box overlaps some anchor (no maximum is 0).  The sizes stay within 3 % of the anchor's: a box that contains an anchor, or lies in
    one, has the same IoU with its neighbours too -- a tie in exact arithmetic that every rounding breaks its own way.  One box in four
    hangs over the grid's last column by half its width: a best IoU in the lower bands, positive by the low-quality rule alone.  The
    anchor yaws are 0 and 35 (read as degrees, a real turn): at 0 and pi / 2 "degrees" the two anchors of a cell tie to about 1e-5."""
    anchors, thresh = _cfg_anchors(3, MIXED_YAWS)
    n = 200
    cls = np.where(np.arange(n) % 20 < 13, 0, np.where(np.arange(n) % 20 < 16, 1, 2))
    gt = np.zeros((n, 7))
    gt[:, 0] = rng.uniform(0.1, 2.8, n)
    over = np.arange(n) % 4 == 3
    gt[over, 0] = (anchors[0, :, 0].max() + rng.uniform(0.45, 0.75, n) * anchors[cls, 0, 3])[over]
    gt[:, 1] = rng.uniform(-1.0, 1.0, n)
    gt[:, 2] = -0.6 + rng.uniform(-0.2, 0.2, n)
    gt[:, 3:6] = anchors[cls, 0, 3:6] * rng.uniform(0.97, 1.03, (n, 3))
    gt[:, 6] = rng.uniform(-3.0, 3.0, n) + np.where(np.arange(n) % 2 == 0, MIXED_YAWS[0], MIXED_YAWS[1])
    last = np.flatnonzero(cls == 0)[-1]  # the 130th car sits on an anchor of its own: that anchor's match is past the staging limit
    gt[last, :2] = anchors[0, 45, :2] + (0.02, -0.03)
    gt[last, 6] = anchors[0, 45, 6] + 0.5
    return _pack(gt, cls, anchors, thresh, True, cfg=(3, MIXED_YAWS))


def _encode_yaw():
    an, gt = [], []
    for i, d in enumerate(YAW_DIFFS):  # anchor yaw 0: the float32 difference is the ground truth's yaw
        an.append([10.0 * i, 0.0, -1.0, *CAR, 0.0])
        gt.append([10.0 * i, 0.0, -1.0, *CAR, F(d)])
    base = F(1.5708)
    for i, y in enumerate([F(base + F(ref.PI32)), F(-1.5708), F(4.7), F(-4.8)]):
        an.append([10.0 * i, 20.0, -1.0, *CAR, base])
        gt.append([10.0 * i, 20.0, -1.0, *CAR, y])
    return _pack(gt, [0] * len(gt), np.asarray(an, np.float64)[None], [CAR_THRESH], False)


def _encode_size():
    an, gt = [], []
    for i, r in enumerate(SIZE_RATIOS):
        a = np.array([50.0 * i, 0.0, -1.0, *CAR, 0.0 if i % 2 else 1.5708])
        b = a.copy()
        b[:3] += (0.3, -0.2, 0.5)
        b[3:6] *= r
        b[6] = 0.7
        an.append(a)
        gt.append(b)
    return _pack(gt, [0] * len(gt), np.asarray(an)[None], [CAR_THRESH], True)


def _stale(rng, which):
    """two frames of one shape (2 ground truths, 70 anchors): `high` sits on its anchors, `low` is low_quality-below_lo's kind"""
    an = lattice(rng, 70)
    if which == "high":
        gt = [near(an[3], 0.01, 0.02, 0.0), near(an[66], -0.02, 0.01, 0.0)]
    else:
        gt = [near(an[3], 0.1, -1.9, -0.2), near(an[66], -0.12, 1.8, 3.0)]
    return _pack(gt, [0, 0], an[None], [CAR_THRESH], True)


@functools.lru_cache(maxsize=None)
def case(name):
    kind, _, arg = name.partition("-")
    rng = _rng(name)
    if kind == "grid":
        return _grid(rng, int(arg[1:]))
    if kind == "band":
        return _band(arg)
    if kind == "first_max":
        return _first_max(_rng("first_max"), arg == "reversed")
    if kind == "interleaved":
        return _interleaved(rng, int(arg[1:]))
    if kind == "low_quality":
        return _low_quality(rng, arg)
    if name == "crowd-mixed":
        return _crowd_mixed(rng)
    if kind == "crowd":
        return _crowd(rng, int(arg))
    if name == "encode-yaw":
        return _encode_yaw()
    if name == "encode-size":
        return _encode_size()
    if name == "empty":
        return _pack(np.zeros((0, 7)), [], np.stack([lattice(rng, 70), lattice(rng, 70, size=(0.6, 0.8, 1.73))]),
                     [CAR_THRESH, (0.2, 0.35)], True)
    if kind == "stale":
        return _stale(_rng("stale"), arg)
    raise KeyError(name)


GRID = [f"grid-A{a}" for a in GRID_SIZES]
BANDS = [f"band-{k}" for k in BAND]
LOW_QUALITY = [f"low_quality-{k}" for k in ("clear", "dup_anchors", "far_gt", "below_lo")]
CROWD = [f"crowd-{n}" for n in CROWD_SIZES] + ["crowd-mixed"]
NAMES = GRID + BANDS + ["first_max", "first_max-reversed", "interleaved-c3", "interleaved-c16"] + LOW_QUALITY + CROWD + \
    ["encode-yaw", "encode-size", "empty", "stale-high", "stale-low"]
# (name, low_quality): every case with its own setting, the low-quality cases and the mixed crowd also with the rule off
RUNS = [(n, case(n)["low_quality"]) for n in NAMES] + [(n, False) for n in LOW_QUALITY + ["crowd-mixed", "grid-A257"]]
RUN_IDS = [f"{n}{'' if lq == case(n)['low_quality'] else '-rule_off'}" for n, lq in RUNS]
assert len(set(RUN_IDS)) == len(RUN_IDS)


@functools.lru_cache(maxsize=None)
def reference(name, low_quality):
    c = case(name)
    out = ref.assign(c["gt"], c["gt_class"], c["anchors"], c["thresh"], low_quality)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------- direction
DIRECTION_SIZES = [1, 255, 262144, 262145, 300000]  # 262 144 = 1 024 workgroups x 256: the last size of one trip
DIRECTION_N_GT = 5
BAD_MATCHES = [-1, DIRECTION_N_GT, 2 ** 40]


@functools.lru_cache(maxsize=None)
def direction_case(n):
    """-> dict(gt (5, 7) f32, matches (n,) i64, m_reg (n,) bool).  The yaws -- both bits, three turns -- stay BIN_MARGIN from a bin edge;
    one element in eight is no positive, one in eight holds a match outside [0, 5) (the last element always does, and is marked
    positive)."""
    import direction_cases
    import direction_ref
    rng = _rng(f"direction-{n}")
    gt = np.zeros((DIRECTION_N_GT, 7), F)
    gt[:, 3:6] = CAR
    gt[:, 6] = np.asarray([0.3, 1.2, -2.5, 4.1, -5.9], F)  # bits 1, 0, 0, 1, 1
    assert (direction_ref.bin_edge_distance(gt[:, 6].astype(np.float64)) >= direction_cases.BIN_MARGIN).all()
    assert len(set(direction_ref.bit(gt[:, 6].astype(np.float64)).tolist())) == 2
    matches = rng.integers(0, DIRECTION_N_GT, n).astype(np.int64)
    m_reg = rng.random(n) > 0.125
    bad = rng.random(n) < 0.125
    matches[bad] = rng.choice(BAD_MATCHES, int(bad.sum()))
    matches[-1], m_reg[-1] = BAD_MATCHES[(n % 3)], True
    if n > 1:
        matches[-2], m_reg[-2] = 0, True  # bit 1 on the last valid element
    for v in (gt, matches, m_reg):
        v.setflags(write=False)
    return dict(gt=gt, matches=matches, m_reg=m_reg)
