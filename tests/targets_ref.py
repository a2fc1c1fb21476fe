"""Anchor <-> ground-truth target assignment (csrc/targets.hip: v3d_assign_targets, v3d_direction_targets) restated in float64 numpy.
Reads nothing from vision3d_amd; the IoU is the convex clipper of tests/object_noise_ref.py, the direction bit is tests/direction_ref.py.

  IoU        of the BEV rectangles (x, y, w, l, yaw) = columns 0, 1, 3, 4, 6.  The yaw column holds radians and the operator reads
             DEGREES (H1, core/proposal_targets.py): the rectangle is turned by yaw * pi / 180.
  match      per class, over the class's ground truths in input order: an anchor's best IoU and the FIRST ground truth attaining it;
             label 0 below lo, -1 in [lo, hi), +1 from hi on; with the low-quality rule every anchor attaining some ground truth's
             maximum is +1 -- ties included, and a ground truth that overlaps nothing has maximum 0, attained by every anchor that
             does not overlap it.  A class without ground truth: label 0, match 0.
  assign     G_cls = label clamped at 0, M_cls = label != -1, M_reg = label == 1, matches = INPUT index of the best ground truth,
             G_reg = encode(gt[match], anchor) at M_reg and 0 elsewhere.  A class id outside [0, n_cls) belongs to no class.
  encode     the VoxelNet residuals.  The inputs are the float32 values; the yaw difference is ONE float32 subtraction (it is the
             input of the wrap); everything else -- sqrt, the divisions, log, remainder(., (float)pi) with the sign of the modulus --
             is float64.

Besides the result, `assign` returns the MARGINS of the case, so that a test can tell whether two correct implementations in different
arithmetic must agree on it:
  band     the smallest |best - lo| and |best - hi| over the anchors of the classes that have ground truth;
  gt_gap   the smallest gap between an anchor's best IoU and its best IoU against a DISTINCT ground truth (one whose row differs from
           the matched one's), over the anchors whose best is positive (an anchor that overlaps nothing ties every ground truth at
           exactly 0 and takes the first);
  row_gap  the smallest gap between a ground truth's maximum and the best anchor that does not attain it.

The keyword switches (lo_closed, hi_closed, strict, ties, zero_row, stage_limit, wrap_sign; `trips` of direction_strided) are single-
line MUTATIONS of this statement, off by default: tests/test_host_targets_ref.py turns each on to show which case would notice a kernel
that made the same mistake.
"""
import numpy as np

import direction_ref
from object_noise_ref import rect_iou

F = np.float32
PI32 = float(np.float32(np.pi))
BEV = [0, 1, 3, 4, 6]
BLOCK = 256                 # threads of a workgroup (V3D_BLOCK)
DIRECTION_MAX_BLOCKS = 1024  # ta_direction_kernel's grid: it strides beyond 1 024 x 256 elements


def bev_iou(gt, anchors):
    """(M, 7) x (N, 7) float32 -> (M, N) float64"""
    gt, anchors = np.asarray(gt, F).reshape(-1, 7), np.asarray(anchors, F).reshape(-1, 7)
    a = gt[:, BEV].astype(np.float64)
    b = anchors[:, BEV].astype(np.float64)
    a[:, 4] *= np.pi / 180.0
    b[:, 4] *= np.pi / 180.0
    out = np.zeros((len(a), len(b)))
    for i in range(len(a)):
        for j in range(len(b)):
            out[i, j] = rect_iou(a[i], b[j])
    return out


def match(iou, lo, hi, low_quality, lo_closed=True, hi_closed=True, strict=True, ties=True, zero_row=True):
    """(M, N) IoU -> labels (N,) in {-1, 0, 1}, matches (N,) = row of the first maximal ground truth."""
    iou = np.asarray(iou, np.float64)
    M, N = iou.shape
    if M == 0:
        return np.zeros(N, np.int64), np.zeros(N, np.int64)
    best = iou.max(0)
    arg = iou.argmax(0) if strict else M - 1 - iou[::-1].argmax(0)  # mutation: >= keeps the LAST maximal ground truth
    below_lo = best < lo if lo_closed else best <= lo
    below_hi = best < hi if hi_closed else best <= hi
    labels = np.where(below_lo, 0, np.where(below_hi, -1, 1)).astype(np.int64)
    if low_quality:
        top = iou.max(1, keepdims=True)
        hit = iou == top
        if not ties:  # mutation: only the first anchor attaining a maximum
            first = np.zeros_like(hit)
            first[np.arange(M), hit.argmax(1)] = True
            hit = first
        if not zero_row:  # mutation: a ground truth that overlaps nothing promotes nobody
            hit = hit & (top > 0)
        labels[hit.any(0)] = 1
    return labels, arg.astype(np.int64)


def encode(boxes, anchors, wrap_sign="modulus"):
    """(k, 7) float32 x (k, 7) float32 -> (k, 7) float64"""
    boxes, anchors = np.asarray(boxes, F).reshape(-1, 7), np.asarray(anchors, F).reshape(-1, 7)
    b, a = boxes.astype(np.float64), anchors.astype(np.float64)
    out = np.zeros(b.shape)
    diag = np.sqrt(a[:, 3] * a[:, 3] + a[:, 4] * a[:, 4])
    out[:, 0] = (b[:, 0] - a[:, 0]) / diag
    out[:, 1] = (b[:, 1] - a[:, 1]) / diag
    out[:, 2] = (b[:, 2] - a[:, 2]) / a[:, 5]
    out[:, 3:6] = np.log(b[:, 3:6] / a[:, 3:6])
    d = (boxes[:, 6] - anchors[:, 6]).astype(F).astype(np.float64)  # one float32 subtraction
    out[:, 6] = np.remainder(d, PI32) if wrap_sign == "modulus" else np.fmod(d, PI32)  # mutation: the sign of the dividend
    return out


def assign(gt, gt_class, anchors, thresh, low_quality, stage_limit=None, wrap_sign="modulus", **mutation):
    """gt (n, 7) f32, gt_class (n,) int, anchors (n_cls, A, 7) f32, thresh (n_cls, 2) -> dict(G_cls int8, M_cls, M_reg bool,
    matches int64 -- all (n_cls, A) --, G_reg (n_cls, A, 7) float64, iou = the per-class matrices, band, gt_gap, row_gap)."""
    gt = np.asarray(gt, F).reshape(-1, 7)
    gt_class = np.asarray(gt_class, np.int64).reshape(-1)
    anchors = np.asarray(anchors, F)
    n_cls, A = anchors.shape[:2]
    thresh = np.asarray(thresh, F).reshape(n_cls, 2).astype(np.float64)
    labels = np.zeros((n_cls, A), np.int64)
    matches = np.zeros((n_cls, A), np.int64)
    G_reg = np.zeros((n_cls, A, 7))
    band = gt_gap = row_gap = np.inf
    ious = []
    for c in range(n_cls):
        idx = np.flatnonzero(gt_class == c)
        if stage_limit is not None:  # mutation: the staging cut short
            idx = idx[:stage_limit]
        iou = bev_iou(gt[idx], anchors[c])
        ious.append(iou)
        lab, arg = match(iou, thresh[c, 0], thresh[c, 1], low_quality, **mutation)
        labels[c] = lab
        if len(idx) == 0:
            continue
        matches[c] = idx[arg]
        pos = lab == 1
        G_reg[c][pos] = encode(gt[matches[c][pos]], anchors[c][pos], wrap_sign)
        best = iou.max(0)
        band = min(band, float(np.abs(best - thresh[c, 0]).min()), float(np.abs(best - thresh[c, 1]).min()))
        for a in np.flatnonzero(best > 0):
            distinct = (gt[idx] != gt[idx[arg[a]]]).any(1)
            if distinct.any():
                gt_gap = min(gt_gap, float(best[a] - iou[distinct, a].max()))
        for i in range(len(idx)):
            rest = iou[i][iou[i] < iou[i].max()]
            if rest.size:
                row_gap = min(row_gap, float(iou[i].max() - rest.max()))
    return dict(G_cls=np.maximum(labels, 0).astype(np.int8), M_cls=labels != -1, M_reg=labels == 1, matches=matches, G_reg=G_reg,
                labels=labels, iou=ious, band=band, gt_gap=gt_gap, row_gap=row_gap)


def direction(gt, matches, m_reg, offset=direction_ref.OFFSET):
    """G_dir int8 in the shape of `matches`: direction_ref.targets, a match outside [0, n_gt) counting as "not positive"."""
    gt = np.asarray(gt, F).reshape(-1, 7)
    matches = np.asarray(matches, np.int64)
    ok = np.asarray(m_reg).reshape(matches.shape).astype(bool) & (matches >= 0) & (matches < len(gt))
    return direction_ref.targets(gt[:, 6].astype(np.float64), np.where(ok, matches, 0), ok, offset)


def direction_strided(gt, matches, m_reg, offset=direction_ref.OFFSET, trips=None, untouched=7):
    """The launch of v3d_direction_targets restated: min(1 024, ceil(n / 256)) workgroups of 256, element i written on trip
    i // (workgroups * 256).  trips = None: as many as it takes; a number: the loop cut after that many (mutation).  Elements never
    written keep `untouched`."""
    matches = np.asarray(matches, np.int64).reshape(-1)
    n = matches.size
    blocks = min(DIRECTION_MAX_BLOCKS, -(-n // BLOCK))
    reach = n if trips is None else min(n, trips * blocks * BLOCK)
    out = np.full(n, untouched, np.int8)
    out[:reach] = direction(gt, matches, np.asarray(m_reg).reshape(-1))[:reach]
    return out
