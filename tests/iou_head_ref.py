"""The IoU-aware confidence head of the anchor head (cfg.IOU_HEAD) restated in plain numpy, float64: the decode
relative to the anchor's centre, the IoU target, the loss with its gradient with respect to the fused [cls | reg | (dir) | iou] head
maps, and the score rule of the proposal stage.  No GPU.  The rotated 3-D IoU of a pair is that of tests/iou_loss_ref.py (float64, by
an algorithm other than the kernels' clipper).

Layouts (those of the C ABI): maps (B, n_anchor * (9 + with_dir), H, W), n_anchor = n_cls * n_yaw -- class channel c * n_yaw + yaw, box
channel n_anchor + (c * 7 + d) * n_yaw + yaw, direction channel n_anchor * 8 + c * n_yaw + yaw, IoU channel n_anchor * (8 + with_dir) +
c * n_yaw + yaw; anchors (n_cls, n_yaw, H, W, 7); targets (B, n_cls, n_yaw, H, W[, 7 | 1]).
"""
import math

import numpy as np

import direction_ref as D
import proposal_ref as R

PI = math.pi
POWERS = (0, 1, 4)


# ------------------------------------------------------------------------------------------------------------------------ layout
def split_maps(maps, n_cls, n_yaw, with_dir):
    """fused maps -> (P_cls (B, n_cls, n_yaw, H, W), P_reg (..., 7), P_dir like P_cls or None, P_iou like P_cls)"""
    maps = np.asarray(maps)
    B, O, H, W = maps.shape
    na = n_cls * n_yaw
    assert O == na * (9 + bool(with_dir))
    p_cls = maps[:, :na].reshape(B, n_cls, n_yaw, H, W)
    p_reg = maps[:, na:8 * na].reshape(B, n_cls, 7, n_yaw, H, W).transpose(0, 1, 3, 4, 5, 2)
    p_dir = maps[:, 8 * na:9 * na].reshape(B, n_cls, n_yaw, H, W) if with_dir else None
    p_iou = maps[:, (8 + bool(with_dir)) * na:].reshape(B, n_cls, n_yaw, H, W)
    return p_cls, p_reg, p_dir, p_iou


# ------------------------------------------------------------------------------------------------------------------------ target
def relative_boxes(deltas, anchors):
    """decode without the anchor's centre: (d_xyz * (diag, diag, a_h), exp(d_wlh) * a_wlh, d_yaw + a_yaw), float64"""
    d, a = np.asarray(deltas, np.float64), np.asarray(anchors, np.float64)
    diag = np.sqrt(a[..., 3] ** 2 + a[..., 4] ** 2)
    out = np.empty(np.broadcast(d, a).shape, np.float64)
    out[..., 0] = d[..., 0] * diag
    out[..., 1] = d[..., 1] * diag
    out[..., 2] = d[..., 2] * a[..., 5]
    with np.errstate(over="ignore"):
        out[..., 3:6] = np.exp(d[..., 3:6]) * a[..., 3:6]
    out[..., 6] = d[..., 6] + a[..., 6]
    return out


def pair_iou(a, b):
    """(N, 7), (N, 7) float64 -> (N,) rotated 3-D IoU (tests/iou_loss_ref.py; bad rows, judged in float32, give 0)"""
    import torch

    import iou_loss_ref
    if len(a) == 0:
        return np.zeros(0)
    # a size that overflows float32 is a bad row of the native pass: make it one here (inf) before the restatement judges it
    a32, b32 = np.asarray(a, np.float64).copy(), np.asarray(b, np.float64).copy()
    for x in (a32, b32):
        with np.errstate(over="ignore"):
            x[~np.isfinite(x.astype(np.float32))] = np.inf
    return iou_loss_ref.iou3d_terms(torch.from_numpy(a32), torch.from_numpy(b32), "iou")[1].numpy()


def iou_target(p_reg, g_reg, anchors, m_reg):
    """t (B, n_cls, n_yaw, H, W) float64: clamp(IoU3D(box(P_reg), box(G_reg)), 0, 1) at the positives, 0 elsewhere"""
    p_reg = np.asarray(p_reg, np.float64)
    pos = np.asarray(m_reg).astype(bool).reshape(p_reg.shape[:-1])
    anc = np.broadcast_to(np.asarray(anchors, np.float64).reshape((1,) + p_reg.shape[1:]), p_reg.shape)
    t = np.zeros(pos.shape)
    t[pos] = np.clip(pair_iou(relative_boxes(p_reg[pos], anc[pos]), relative_boxes(np.asarray(g_reg, np.float64)[pos], anc[pos])), 0.0, 1.0)
    return t


# -------------------------------------------------------------------------------------------------------------------------- loss
def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def soft_bce(z, t):
    """max(z, 0) - z t + log1p(exp(-|z|)); gradient sigmoid(z) - t"""
    return np.maximum(z, 0.0) - z * t + np.log1p(np.exp(-np.abs(z)))


def loss(maps, anchors, G_cls, M_cls, G_reg, M_reg, G_dir, n_cls, n_yaw, sin_yaw=True, lam=1.0, dir_weight=0.2, iou_weight=1.0,
         alpha=0.25, gamma=2.0):
    """G_dir None: no direction group.  -> dict(cls_loss, reg_loss, dir_loss (0.0 without the group), iou_loss, loss, normalizer,
    target, grads = (d cls_loss, d reg_loss, d dir_loss, d iou_loss), each in the maps' shape)."""
    maps = np.asarray(maps, np.float64)
    B, _, H, W = maps.shape
    na = n_cls * n_yaw
    with_dir = G_dir is not None
    p_cls, p_reg, p_dir, p_iou = split_maps(maps, n_cls, n_yaw, with_dir)
    m_cls = np.asarray(M_cls).astype(bool)
    pos = np.asarray(M_reg).astype(bool).reshape(m_cls.shape)
    n = max(int(pos.sum()), 1)
    # focal (ops/focal_loss.py)
    t = (np.asarray(G_cls) > 0).astype(np.float64)
    prob = _sigmoid(p_cls)
    bce = soft_bce(p_cls, t)
    q = 1.0 - (prob * t + (1.0 - prob) * (1.0 - t))
    w = alpha * t + (1.0 - alpha) * (1.0 - t)
    focal = w * bce * q ** gamma
    d_focal = w * ((prob - t) * q ** gamma - bce * gamma * q ** (gamma - 1.0) * prob * (1.0 - prob) * (2.0 * t - 1.0))
    cls_loss = float((focal * m_cls).sum()) / n
    # box terms: smooth-L1, the yaw column / pi counted three times; with a direction group and sin_yaw its argument is sin(P - G)
    diff = p_reg - np.asarray(G_reg, np.float64)
    ad = np.abs(diff)
    val, grad = np.where(ad < 1.0, 0.5 * diff * diff, ad - 0.5), np.clip(diff, -1.0, 1.0)
    if with_dir and sin_yaw:
        s = np.sin(diff[..., 6])
        val[..., 6], grad[..., 6] = np.where(np.abs(s) < 1.0, 0.5 * s * s, np.abs(s) - 0.5), np.clip(s, -1.0, 1.0) * np.cos(diff[..., 6])
    wd = np.array([1.0] * 6 + [3.0 / PI])
    reg_loss = float((val * wd * pos[..., None]).sum()) / n
    grads = [np.zeros_like(maps) for _ in range(4)]
    grads[0][:, :na] = (d_focal * m_cls / n).reshape(B, na, H, W)
    grads[1][:, na:8 * na] = (grad * wd * pos[..., None] / n).transpose(0, 1, 5, 2, 3, 4).reshape(B, 7 * na, H, W)
    dir_loss = 0.0
    if with_dir:
        g = (np.asarray(G_dir) > 0).astype(np.float64)
        dir_loss = float((soft_bce(p_dir, g) * pos).sum()) / n
        grads[2][:, 8 * na:9 * na] = ((_sigmoid(p_dir) - g) * pos / n).reshape(B, na, H, W)
    # IoU confidence: the target is a constant
    target = iou_target(p_reg, G_reg, anchors, pos)
    iou_loss = float((soft_bce(p_iou, target) * pos).sum()) / n
    grads[3][:, (8 + with_dir) * na:] = ((_sigmoid(p_iou) - target) * pos / n).reshape(B, na, H, W)
    total = cls_loss + lam * reg_loss + (dir_weight * dir_loss if with_dir else 0.0) + iou_weight * iou_loss
    return dict(cls_loss=cls_loss, reg_loss=reg_loss, dir_loss=dir_loss, iou_loss=iou_loss, loss=total, normalizer=n, target=target,
                grads=tuple(grads))


# ------------------------------------------------------------------------------------------------------------------- score rule
def rectify(s, z, power):
    """s' = s * q^power in float64, q = 1 / (1 + exp(-z)) with a NaN z counted as -inf (q = 0); a sentinel (s < 0) keeps its score"""
    s, z = np.asarray(s, np.float64), np.array(z, np.float64)
    z[np.isnan(z)] = -np.inf
    with np.errstate(over="ignore"):
        q = 1.0 / (1.0 + np.exp(-z))
    out = s.copy()
    for _ in range(int(power)):
        out = out * q
    return np.where(s >= 0, out, s)


def reorder(rect):
    """(..., k) rectified scores in class-score order -> the stable descending order (ties: position in the class-score order)"""
    return np.argsort(-np.asarray(rect), axis=-1, kind="stable")


def relative_gaps(rect):
    """(..., k) -> the smallest |a - b| / max(a, b) over the pairs of DISTINCT values of a group (inf where a group has one value)"""
    flat = np.asarray(rect, np.float64).reshape(-1, np.shape(rect)[-1])
    worst = np.inf
    for row in flat:
        v = np.unique(row[row >= 0])
        if v.size > 1:
            worst = min(worst, float(((v[1:] - v[:-1]) / v[1:]).min()))
    return worst


def candidates(maps, anchors, B, n_cls, n_yaw, H, W, topk, with_dir, power):
    """Selection by class score (proposal_ref.candidates on the class / box channels), the score rule, the stable reorder.
    -> dict(idx (anchor indices, final order), pos (position in the class-score order), scores (s', float64), class_scores (float32),
    iou_logit, boxes (float64; with_dir: the yaw by the direction rule), rect_unordered)"""
    maps = np.asarray(maps)
    na, n = n_cls * n_yaw, n_yaw * H * W
    idx, sc, boxes = R.candidates(maps[:, :na * 8], anchors, B, n_cls, n_yaw, H, W, topk)
    if with_dir:
        logit = np.take_along_axis(maps[:, na * 8:na * 9].reshape(B, n_cls, n), idx, 2)
        boxes = boxes.copy()
        boxes[..., 6] = D.decode_yaw(boxes[..., 6], logit)
    z = np.take_along_axis(maps[:, na * (8 + bool(with_dir)):].reshape(B, n_cls, n), idx, 2)
    rect = rectify(sc, z, power)
    order = reorder(rect) if power > 0 else np.broadcast_to(np.arange(topk), rect.shape)
    take = lambda a: np.take_along_axis(a, order, 2)
    return dict(idx=take(idx), pos=order, scores=take(rect), class_scores=take(sc), iou_logit=take(z),
                boxes=np.take_along_axis(boxes, order[..., None], 2), rect_unordered=rect)


def stage(maps, anchors, B, n_cls, n_yaw, H, W, topk, thresh, iou_thr, with_dir, power):
    """The whole stage: `candidates`, then proposal_ref's tail (batched rotated NMS, strict score cut) on s'."""
    c = candidates(maps, anchors, B, n_cls, n_yaw, H, W, topk, with_dir, power)
    out = R._tail(c["boxes"], c["scores"], B, n_cls, topk, thresh, iou_thr)
    out["candidates"] = c
    return out
