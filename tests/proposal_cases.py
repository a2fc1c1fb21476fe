"""The case tables of tests/test_gpu_proposal_edges.py and the builders of their inputs, shared with tests/test_host_proposal_ref.py,
which proves on the CPU -- on the reference alone -- that every case is well-posed (scores separated, NMS decisions clear of the
threshold, survivor share, the property a hand-built case is named for).  Every builder is deterministic and cached: a case and
its reference are computed once per process and must not be modified by a test."""
import functools
import zlib

import numpy as np

import proposal_ref as R

# (n_yaw, H, W, topk): the level-1 slicing each row hits is asserted in test_host_proposal_ref.py::test_slicing_of_the_table
SELECT_ROWS = [
    (1, 2, 5, 10),        # n == K, one slice of 10
    (2, 7, 9, 10),        # 3 slices of 64: 64, 62, 0
    (1, 9, 29, 16),       # 4 slices of 128: 128, 128, 5 (< K), 0
    (2, 5, 13, 1),        # K = 1, 32 slices, 29 of them empty
    (2, 24, 24, 64),      # K equal to its padding
    (2, 24, 24, 65),      # ... and one over it
    (2, 40, 40, 256),     # last rank sort
    (2, 40, 40, 257),     # first bitonic sort
    (2, 60, 60, 300),     # bitonic select and a multi-slice merge
    (1, 64, 64, 1024),    # cand[] full, one slice of 4096
    (1, 181, 181, 1024),  # <8>, 4 slices of 8192, merge of exactly 4096
    (2, 288, 288, 100),   # <8>, 40 slices of 4160
]
FILLS = ("lattice", "specials")
# (row, B, n_cls): one group takes the fused merge + decode launch, six groups the separate merge and decode launches
SELECT_CASES = [(row, 1, 1, fill) for row in SELECT_ROWS for fill in FILLS] + \
               [(row, 2, 3, fill) for row in (SELECT_ROWS[1], SELECT_ROWS[2]) for fill in FILLS]
TIE_ROWS = [SELECT_ROWS[2], SELECT_ROWS[4], SELECT_ROWS[5], SELECT_ROWS[11]]
TIE_KINDS = ("straddle", "all_equal", "all_zero", "signed_zero")
TIE_CASES = [(row, kind) for row in TIE_ROWS for kind in TIE_KINDS]
NONFINITE_ROW = SELECT_ROWS[2]
DECODE_CASES = [(SELECT_ROWS[1], 2, 3), (SELECT_ROWS[6], 1, 1), (SELECT_ROWS[7], 1, 1)]
STAGE_CASES = [SELECT_ROWS[2], SELECT_ROWS[6], SELECT_ROWS[7]]  # three classes each: 48 (LDS mask), 768 and 771 (global mask)
STAGE_THRESH = (0.80, 0.84, 0.87)  # inside the score range of the top-k of a lattice map, so the cut drops some and keeps some
STAGE_IOU = 0.01
# the acceptance edge: 40 slices of exactly 8192 anchors; one more W column passes 8192
EDGE_SHAPE, EDGE_TOPK = (2, 320, 512), 100

TAIL_SHAPES = [(1, 1, 63), (1, 1, 64), (1, 1, 65), (1, 1, 341), (1, 1, 342), (1, 1, 1024), (2, 3, 50), (3, 2, 170)]
TAIL_IOUS = (0.01, 0.3)
# (B, n_cls, topk, iou, mode): "mix" = per-class thresholds with 0.5 among them, "none" = every threshold 1.0, "all" = every -1
TAIL_CASES = [(*s, iou, "mix") for s in TAIL_SHAPES for iou in TAIL_IOUS] + \
             [(2, 3, 50, 0.3, "none"), (2, 3, 50, 0.3, "all"), (1, 1, 342, 0.01, "none"), (1, 1, 342, 0.01, "all")]
TAIL_THRESH = {"mix": (0.5, 0.4, 0.6), "none": (1.0, 1.0, 1.0), "all": (-1.0, -1.0, -1.0)}
# seeds chosen on the CPU so that batched_margin > 1e-5 and the survivor share hold (test_host_proposal_ref.py asserts both);
# a case not listed uses seed 0
TAIL_SEEDS = {(1, 1, 63, 0.3, "mix"): 1, (1, 1, 1024, 0.01, "mix"): 1, (1, 1, 342, 0.01, "none"): 1}
STAGE_SEEDS = {(2, 40, 40, 257): 1}
MARGIN = 1e-5  # the margin the project's NMS fixtures use
# whole-stage cases: the kernel's NMS sees its own fp32 decode, an ulp or two of a 70 m coordinate (~1e-5 m, ~1e-5 of an IoU of
# car-sized boxes) from the float64 decode the margin is measured on -- so their seeds are chosen for ten times the margin
STAGE_MARGIN = 1e-4


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def case_id(case):
    return "-".join("x".join(map(str, p)) if isinstance(p, tuple) else str(p) for p in case)


@functools.lru_cache(maxsize=None)
def select_case(row, B, n_cls, fill):
    """Index anchors, zero regression, lattice logits -> dict(maps, anchors, logits, idx, scores)"""
    n_yaw, H, W, topk = row
    logits = R.lattice_logits(_rng("select", row, B, n_cls, fill), (B, n_cls, n_yaw * H * W), specials=fill == "specials")
    return _select_dict(logits, row, B, n_cls)


def _select_dict(logits, row, B, n_cls, want_logits=None):
    n_yaw, H, W, topk = row
    idx, sc = R.select_topk(logits if want_logits is None else want_logits, topk)
    return dict(maps=R.maps_from_logits(logits, B, n_cls, n_yaw, H, W), anchors=R.index_anchors(n_cls, n_yaw, H, W), logits=logits,
                idx=idx, scores=sc, geom=(B, n_cls, n_yaw, H, W, topk))


@functools.lru_cache(maxsize=None)
def tie_case(row, kind):
    """The hand-built tie maps (B = n_cls = 1).
    straddle:    K // 3 >= 1 anchors strictly above a tie class that holds two anchors in three of the map -- far more members than
                 free rows in every slice and in the merge -- over a lower lattice background
    all_equal:   one lattice value everywhere
    all_zero:    -110 and -120 alternating in runs of three: every score 0.0 from two different keys
    signed_zero: +0.0 / -0.0 checkerboard: every score 0.5 from two different keys"""
    n_yaw, H, W, topk = row
    n = n_yaw * H * W
    rng = _rng("tie", row, kind)
    i = np.arange(n)
    if kind == "straddle":
        x = (-6.0 + R.LATTICE_STEP * rng.integers(0, 64 * 5, size=n)).astype(np.float32)  # background in [-6, -1)
        x[i % 3 != 0] = 0.5
        above = rng.permutation(n)[:max(1, topk // 3)]
        x[above] = (1.0 + R.LATTICE_STEP * rng.integers(0, 65, size=above.size)).astype(np.float32)
    elif kind == "all_equal":
        x = np.full(n, 1.25, np.float32)
    elif kind == "all_zero":
        x = np.where((i // 3) % 2 == 0, R.SPECIAL_ZERO[0], R.SPECIAL_ZERO[1]).astype(np.float32)
    else:
        x = np.where((i + i // W) % 2 == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    return _select_dict(x.reshape(1, 1, n), row, 1, 1)


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """Row 3 with a few +NaN, -NaN, +inf and -inf logits over the lattice; expected: select_topk with NaN replaced by -inf.  The
    last slice of this row holds 5 anchors for K = 16: two of them are NaN, so NaN rows ARE selected there and must lose the merge."""
    n_yaw, H, W, topk = NONFINITE_ROW
    n = n_yaw * H * W
    rng = _rng("nonfinite")
    x = R.lattice_logits(rng, (1, 1, n))
    where = rng.permutation(n - 5)[:16]
    pos_nan, neg_nan = np.array([0x7FC00000, 0xFFC00000], np.uint32).view(np.float32)
    x[0, 0, where[0:5]] = pos_nan
    x[0, 0, where[5:10]] = neg_nan
    x[0, 0, where[10:13]] = np.inf
    x[0, 0, where[13:16]] = -np.inf
    x[0, 0, n - 4], x[0, 0, n - 2] = pos_nan, neg_nan
    return _select_dict(x, NONFINITE_ROW, 1, 1, want_logits=R.nan_as_neg_inf(x))


@functools.lru_cache(maxsize=None)
def decode_case(row, B, n_cls):
    """Random anchors in KITTI ranges, regression channels N(0, 0.3), lattice logits -> maps, anchors, idx, scores, boxes (float64)"""
    n_yaw, H, W, topk = row
    rng = _rng("decode", row, B, n_cls)
    n = n_yaw * H * W
    logits = R.lattice_logits(rng, (B, n_cls, n))
    reg = (rng.standard_normal((B, n_cls, 7, n)) * 0.3).astype(np.float32)
    maps, anchors = R.maps_from_logits(logits, B, n_cls, n_yaw, H, W, reg), R.kitti_anchors(rng, n_cls, n_yaw, H, W)
    idx, sc, boxes = R.candidates(maps, anchors, B, n_cls, n_yaw, H, W, topk)
    return dict(maps=maps, anchors=anchors, logits=logits, idx=idx, scores=sc, boxes=boxes, geom=(B, n_cls, n_yaw, H, W, topk))


@functools.lru_cache(maxsize=None)
def stage_case(row):
    """The whole stage at B = 1, three classes, random anchors and deltas, distinct thresholds -> inputs and `R.stage`'s result"""
    n_yaw, H, W, topk = row
    B, n_cls = 1, 3
    rng = _rng("stage", row, STAGE_SEEDS.get(row, 0))
    n = n_yaw * H * W
    logits = R.lattice_logits(rng, (B, n_cls, n))
    reg = (rng.standard_normal((B, n_cls, 7, n)) * 0.3).astype(np.float32)
    side = float(np.sqrt(topk * 12.0))  # as crowded as a tail case: the NMS has work to do at any topk
    maps, anchors = R.maps_from_logits(logits, B, n_cls, n_yaw, H, W, reg), R.kitti_anchors(rng, n_cls, n_yaw, H, W, (side, side / 2))
    ref = R.stage(maps, anchors, B, n_cls, n_yaw, H, W, topk, STAGE_THRESH, STAGE_IOU)
    return dict(maps=maps, anchors=anchors, logits=logits, ref=ref, geom=(B, n_cls, n_yaw, H, W, topk), thresh=STAGE_THRESH, iou=STAGE_IOU)


TAIL_CONF_VALUES = np.array([-2.0, -1.0, -0.5, 0.0, -0.0, 0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 20.0, 30.0, -110.0], np.float32)
# m^2 of scatter region per car (a car covers ~6.4), by IoU threshold: the looser threshold needs the denser scene for the same share
AREA_PER_BOX = {0.01: 10.0, 0.3: 4.0}


@functools.lru_cache(maxsize=None)
def tail_case(B, n_cls, topk, iou, mode):
    """Stage-2 tail inputs with ZERO deltas (refined == proposals bit for bit), boxes of our choosing:
      * KITTI-like cars scattered over a square sized so that between a quarter and three quarters survive the NMS;
      * a block of identical boxes (rows [2, 2 + blk) of group 0);
      * with more than one group, one identical box in row 0 of groups 0 and 1, away from everything else: both must survive;
      * z of candidate i is i itself, so an output row names its candidate.
    Confidence logits: a handful of lattice values (many equal scores: the order is by candidate index), exact 0.0 / -0.0 (score
    exactly 0.5, the threshold of class 0 in "mix": dropped by the strict cut), and saturated values."""
    G, N = B * n_cls, B * n_cls * topk
    rng = _rng("tail", B, n_cls, topk, iou, mode, TAIL_SEEDS.get((B, n_cls, topk, iou, mode), 0))
    side = float(np.sqrt(topk * AREA_PER_BOX[iou]))
    p = np.zeros((G, topk, 7), np.float32)
    p[..., 0] = rng.uniform(0.0, side, (G, topk))
    p[..., 1] = rng.uniform(-side / 2, side / 2, (G, topk))
    p[..., 3] = rng.uniform(1.5, 1.8, (G, topk))
    p[..., 4] = rng.uniform(3.5, 4.3, (G, topk))
    p[..., 5] = 1.5
    p[..., 6] = rng.uniform(-np.pi, np.pi, (G, topk))
    blk = max(3, topk // 10)
    p[0, 2:2 + blk] = p[0, 2]
    pair = None
    if G > 1:
        p[0, 0] = p[1, 0] = np.array([-30.0, -side / 2 - 30.0, 0, 1.6, 3.9, 1.5, 0.3], np.float32)
        pair = (0, topk)
    p = p.reshape(N, 7)
    p[:, 2] = np.arange(N, dtype=np.float32)
    conf = TAIL_CONF_VALUES[rng.integers(0, len(TAIL_CONF_VALUES), size=N)]
    if pair:
        conf[list(pair)] = 2.0  # the best score there is in their groups apart from the saturated ones: nothing else is near them anyway
    thresh = TAIL_THRESH[mode][:n_cls]
    deltas = np.zeros((N, 7), np.float32)
    ref = R.refine_stage(deltas, p, conf, B, n_cls, topk, thresh, iou)
    return dict(deltas=deltas, proposals=p, conf=conf, thresh=thresh, iou=iou, ref=ref, geom=(B, n_cls, topk), block=(2, 2 + blk), pair=pair)
