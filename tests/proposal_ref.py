"""An independent statement of the proposal stage (csrc/proposal.hip) in plain numpy, float64 arithmetic, no torch.topk (whose tie
order is unspecified) and no GPU -- plus the input builders that make its result independent of how the last bit of expf rounds.

Order (the header of proposal.hip): the candidates of a (frame, class) group are ordered by (fp32 sigmoid score descending, anchor
index ascending).  A NaN logit counts as -inf: the callers that want that rule replace NaN before they call `select_topk`.

Layouts (those of the C ABI): head maps (B, n_cls * n_yaw * 8, H, W) = [class logits, channel c * n_yaw + yaw | regression, channel
n_cls * n_yaw + (c * 7 + q) * n_yaw + yaw]; anchors (n_cls, n_yaw, H, W, 7); flat anchor index of a group = (yaw * H + y) * W + x.
"""
import numpy as np

from oracle import oracle as O

SEPARATION_ULPS = 64
LATTICE_STEP, LATTICE_LO, LATTICE_HI = 1.0 / 64, -6.0, 2.0
# Logits whose score saturates: both of a pair give the same score from different radix keys.  (The zero pair is -110 / -120:
# under the score formula below a logit of -100 gives 1 / (1 + e^100) = 3.7e-44, a float32 DENORMAL 27 ulps above 0.0, where
# float32 arithmetic overflows expf(100) and gives 0.0 -- such a value is not `assert_separated`; e^110 = 5.9e47 rounds to 0.0 in
# float32 either way.)
SPECIAL_ONE, SPECIAL_ZERO, SPECIAL_HALF = (20.0, 30.0), (-110.0, -120.0), (0.0, -0.0)
SPECIALS = np.array(SPECIAL_ONE + SPECIAL_ZERO + SPECIAL_HALF, np.float32)


def score(x):
    """float32(1 / (1 + exp(-float64(x))))"""
    with np.errstate(over="ignore"):
        return (1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))).astype(np.float32)


def nan_as_neg_inf(x):
    x = np.array(x, np.float32)
    x[np.isnan(x)] = -np.inf
    return x


def select_topk(logits, k):
    """logits (..., n) -> (anchor indices (..., k) int64, scores (..., k) float32): score descending, then index ascending."""
    s = score(logits)
    order = np.argsort(-s, axis=-1, kind="stable")[..., :k]  # stable: equal scores stay in index order
    return order.astype(np.int64), np.take_along_axis(s, order, -1)


def decode(deltas, anchors):
    """core/box_encode.py decode in float64: (*, 7), (*, 7) -> (*, 7)."""
    d, a = np.asarray(deltas, np.float64), np.asarray(anchors, np.float64)
    diag = np.sqrt(a[..., 3] ** 2 + a[..., 4] ** 2)
    out = np.empty(np.broadcast(d, a).shape, np.float64)
    out[..., 0] = d[..., 0] * diag + a[..., 0]
    out[..., 1] = d[..., 1] * diag + a[..., 1]
    out[..., 2] = d[..., 2] * a[..., 5] + a[..., 2]
    out[..., 3:6] = np.exp(d[..., 3:6]) * a[..., 3:6]
    out[..., 6] = d[..., 6] + a[..., 6]
    return out


def class_logits(maps, B, n_cls, n_yaw, H, W):
    return np.asarray(maps)[:, :n_cls * n_yaw].reshape(B, n_cls, n_yaw * H * W)


def candidates(maps, anchors, B, n_cls, n_yaw, H, W, topk):
    """select + decode -> (anchor indices (B, n_cls, topk), scores float32 (B, n_cls, topk), boxes float64 (B, n_cls, topk, 7))"""
    n = n_yaw * H * W
    idx, sc = select_topk(class_logits(maps, B, n_cls, n_yaw, H, W), topk)
    reg = np.asarray(maps)[:, n_cls * n_yaw:].reshape(B, n_cls, 7, n).transpose(0, 1, 3, 2)
    gi = idx[..., None]
    deltas = np.take_along_axis(reg, gi, 2)
    anc = np.take_along_axis(np.broadcast_to(np.asarray(anchors).reshape(1, n_cls, n, 7), (B, n_cls, n, 7)), gi, 2)
    return idx, sc, decode(deltas, anc)


def _tail(boxes, scores, B, n_cls, topk, thresh, iou_thr):
    """batched rotated NMS over group = class + n_cls * batch (oracle/second_cpu.proposals), then the STRICT score cut."""
    boxes, scores = boxes.reshape(-1, 7), scores.reshape(-1)
    bi = np.repeat(np.arange(B), n_cls * topk)
    ci = np.tile(np.repeat(np.arange(n_cls), topk), B)
    kept = O.batched_nms_rotated(boxes[:, [0, 1, 3, 4, 6]], scores, ci + n_cls * bi, iou_thr)
    out = kept[scores[kept] > np.asarray(thresh, np.float32)[ci[kept]]]
    return dict(cand=out, boxes=boxes[out], batch=bi[out], cls=ci[out], scores=scores[out], kept=kept, n_nms=len(kept),
                bev=boxes[:, [0, 1, 3, 4, 6]], groups=ci + n_cls * bi, all_scores=scores)


def stage(maps, anchors, B, n_cls, n_yaw, H, W, topk, thresh, iou_thr):
    """The whole stage.  -> dict: cand (flat candidate rows that survive, in output order), boxes (float64), batch, cls, scores
    (float32), n_nms (survivors of the NMS, before the cut) and the NMS inputs (bev, groups, all_scores) for `batched_margin`."""
    _, sc, boxes = candidates(maps, anchors, B, n_cls, n_yaw, H, W, topk)
    return _tail(boxes, sc, B, n_cls, topk, thresh, iou_thr)


def refine_stage(deltas, proposals, conf, B, n_cls, topk, thresh, iou_thr):
    """The stage-2 tail (v3d_refine_nms): candidates arrive in (B, n_cls, topk) order; score = sigmoid of the confidence logit."""
    return _tail(decode(np.reshape(deltas, (-1, 7)), np.reshape(proposals, (-1, 7))), score(np.reshape(conf, -1)), B, n_cls, topk,
                 thresh, iou_thr)


def batched_margin(boxes5, scores, groups, thr):
    """min |IoU - thr| over the pairs the greedy pass evaluates, on the boxes as `oracle.batched_nms_rotated` sees them."""
    return O.nms_margin(O.group_offset_boxes(boxes5, groups), scores, thr)


# ------------------------------------------------------------------------------------------------------------- input builders
def lattice_logits(rng, shape, specials=False):
    """Multiples of 1/64 in [-6, 2] (513 values: heavy natural ties); specials=True overwrites about one element in eight with
    the saturating / signed-zero values."""
    steps = int(round((LATTICE_HI - LATTICE_LO) / LATTICE_STEP))
    x = (LATTICE_LO + LATTICE_STEP * rng.integers(0, steps + 1, size=shape)).astype(np.float32)
    if specials:
        flat = x.reshape(-1)
        n_sp = max(len(SPECIALS), flat.size // 8)
        where = rng.permutation(flat.size)[:n_sp]
        flat[where] = SPECIALS[np.arange(n_sp) % len(SPECIALS)]  # every special value at least once when the map has room
    return x


def ulp_distance(a, b):
    """Number of float32 values between two non-negative, finite float32 numbers."""
    a, b = (np.asarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    return np.abs(a - b)


def assert_separated(logits, extra_scores=()):
    """The condition on the inputs, checked on the reference alone: any two float32 reference scores (and `extra_scores`, e.g. the
    thresholds of a score cut) are bit-equal or at least 64 float32 ulps apart -- far above the few-ulp error of expf plus one
    division, so a kernel's score order and cut cannot differ from the reference's by rounding."""
    x = np.asarray(logits, np.float32).reshape(-1)
    assert not np.isnan(x).any()
    s = np.unique(np.concatenate([score(x), np.asarray(extra_scores, np.float32).reshape(-1)]))
    s = s[s >= 0]  # a negative threshold lies below every score by more than any rounding
    assert s.size and np.isfinite(s).all()
    gaps = ulp_distance(s[1:], s[:-1])
    assert gaps.size == 0 or gaps.min() >= SEPARATION_ULPS, f"scores {SEPARATION_ULPS} ulps apart: closest pair {gaps.min()} ulps"


def index_anchors(n_cls, n_yaw, H, W):
    """Anchors for selection cases: column 0 is the flat anchor index of the class (exact below 2^24), column 1 the class, sizes
    1 and everything else 0.  With zero regression channels d * diag + a == a and expf(0) * 1 == 1 bit for bit: the decoded box
    names the selected anchor."""
    n = n_yaw * H * W
    assert n < 2 ** 24
    a = np.zeros((n_cls, n, 7), np.float32)
    a[:, :, 0] = np.arange(n, dtype=np.float32)[None]
    a[:, :, 1] = np.arange(n_cls, dtype=np.float32)[:, None]
    a[:, :, 3:6] = 1.0
    return a.reshape(n_cls, n_yaw, H, W, 7)


def maps_from_logits(logits, B, n_cls, n_yaw, H, W, reg=None):
    """class logits (B, n_cls, n_yaw * H * W) [+ regression (B, n_cls, 7, n_yaw * H * W), default zero] -> head maps"""
    n_a = n_cls * n_yaw
    maps = np.zeros((B, n_a * 8, H, W), np.float32)
    maps[:, :n_a] = np.asarray(logits, np.float32).reshape(B, n_a, H, W)
    if reg is not None:
        maps[:, n_a:] = np.asarray(reg, np.float32).reshape(B, n_a * 7, H, W)
    return maps


def kitti_anchors(rng, n_cls, n_yaw, H, W, extent=(70.4, 40.0)):
    """Random anchors in KITTI ranges (for decode cases): centres anywhere in the detection range x in [0, extent[0]], |y| <=
    extent[1], car / pedestrian / cyclist-like sizes, any yaw."""
    a = np.empty((n_cls, n_yaw, H, W, 7), np.float32)
    a[..., 0] = rng.uniform(0.0, extent[0], a.shape[:-1])
    a[..., 1] = rng.uniform(-extent[1], extent[1], a.shape[:-1])
    a[..., 2] = rng.uniform(-3.0, 1.0, a.shape[:-1])
    a[..., 3] = rng.uniform(0.5, 2.0, a.shape[:-1])
    a[..., 4] = rng.uniform(0.7, 4.5, a.shape[:-1])
    a[..., 5] = rng.uniform(1.4, 1.9, a.shape[:-1])
    a[..., 6] = rng.uniform(-np.pi, np.pi, a.shape[:-1])
    return a
