"""numpy restatement of PV-RCNN's stage-2 targets and loss (the repository's own definition: upstream has none), on top of
oracle.box_iou_rotated_3d -- the operator tests/test_gpu_iou_nms.py::test_iou_3d_vs_oracle holds the device bit-equal to.
Targets in float32 in the stated operation order (every threshold decision is comparable exactly); loss and gradient in float64.
Imported by tests/test_host_refine_targets.py and the GPU tests; not a test module itself."""
import math

import numpy as np

from oracle import oracle as O

F = np.float32
HALF_PI, PI = F(1.57079637050628662), F(3.14159274101257324)
DEFAULTS = dict(conf_iou=(0.25, 0.75), reg_iou=0.55, fg_iou=0.55, rois_per_frame=128, fg_fraction=0.5)

# (n_cls, batch) x seeds of the GPU comparisons; tests/test_host_refine_targets.py asserts what the generator gives for each
CONFIGS = ((1, 1), (1, 4), (3, 1), (3, 4))
SEEDS = (0, 5)


def match(proposals, proposal_class, boxes, class_idx):
    """-> iou (B, n) f32, match (B, n) i64 into the concatenated ground-truth list (-1: none)."""
    proposals = np.asarray(proposals, F)
    B, n = proposals.shape[:2]
    iou, mt = np.zeros((B, n), F), np.full((B, n), -1, np.int64)
    off = 0
    for b in range(B):
        gt = np.asarray(boxes[b], F).reshape(-1, 7)
        gc = np.asarray(class_idx[b]).reshape(-1)
        if len(gt):
            m = O.box_iou_rotated_3d(proposals[b], gt)
            m = np.where(gc[None, :] == np.asarray(proposal_class)[:, None], m, F(-1))  # other classes are never matched
            best, arg = m.max(1), m.argmax(1)  # argmax: the first maximal
            ok = best > 0
            iou[b], mt[b] = np.where(ok, best, F(0)), np.where(ok, off + arg, -1)
        off += len(gt)
    return iou, mt


def conf_target(iou, lo, hi):
    return np.clip((iou - F(lo)) / (F(hi) - F(lo)), F(0), F(1)).astype(F)


def encode(gt, roi):
    """Inverse of box_encode.decode(., roi), yaw residual wrapped to [-pi/2, pi/2); float32, one operation at a time."""
    gt, roi = np.asarray(gt, F), np.asarray(roi, F)
    out = np.empty_like(gt)
    diag = np.sqrt(roi[..., 3] * roi[..., 3] + roi[..., 4] * roi[..., 4])
    out[..., 0] = (gt[..., 0] - roi[..., 0]) / diag
    out[..., 1] = (gt[..., 1] - roi[..., 1]) / diag
    out[..., 2] = (gt[..., 2] - roi[..., 2]) / roi[..., 5]
    out[..., 3:6] = np.log(gt[..., 3:6] / roi[..., 3:6])
    out[..., 6] = np.remainder((gt[..., 6] - roi[..., 6]) + HALF_PI, PI) - HALF_PI
    return out


def sample(iou, draws, fg_iou, rois_per_frame, fg_fraction):
    B, n = iou.shape
    taken = np.zeros((B, n), bool)
    quota = max(int(math.floor(rois_per_frame * fg_fraction)), 0)
    for b in range(B):
        if rois_per_frame <= 0:
            taken[b] = True
            continue
        fg = iou[b] >= F(fg_iou)
        order = np.lexsort((np.arange(n), draws[b]))  # by (draw, index)
        n_fg = min(int(fg.sum()), quota)
        n_bg = min(int((~fg).sum()), max(rois_per_frame - n_fg, 0))
        taken[b, order[fg[order]][:n_fg]] = True
        taken[b, order[~fg[order]][:n_bg]] = True
    return taken


def assign(proposals, proposal_class, boxes, class_idx, draws, conf_iou=DEFAULTS["conf_iou"], reg_iou=DEFAULTS["reg_iou"],
           fg_iou=DEFAULTS["fg_iou"], rois_per_frame=DEFAULTS["rois_per_frame"], fg_fraction=DEFAULTS["fg_fraction"]):
    proposals = np.asarray(proposals, F)
    iou, mt = match(proposals, proposal_class, boxes, class_idx)
    gt = np.concatenate([np.asarray(b, F).reshape(-1, 7) for b in boxes]) if len(boxes) else np.zeros((0, 7), F)
    reg = (mt >= 0) & (iou >= F(reg_iou))
    G = np.zeros(proposals.shape, F)
    if reg.any():
        G[reg] = encode(gt[mt[reg]], proposals[reg])
    taken = sample(iou, np.asarray(draws, F), fg_iou, rois_per_frame, fg_fraction)
    return dict(R_iou=iou, R_match=mt, G_conf=conf_target(iou, *conf_iou), G_rreg=G, M_rcls=taken, M_rreg=taken & reg)


def loss(R_reg, R_cls, G_conf, G_rreg, M_rcls, M_rreg, lam=1.0):
    """float64 loss terms, counts and the gradients of the two terms."""
    x = np.asarray(R_cls, np.float64).reshape(np.shape(G_conf))
    q, Mc, Mr = np.asarray(G_conf, np.float64), np.asarray(M_rcls, bool), np.asarray(M_rreg, bool)
    n_cls, n_reg = max(int(Mc.sum()), 1), max(int(Mr.sum()), 1)
    bce = np.maximum(x, 0) - x * q + np.log1p(np.exp(-np.abs(x)))
    cls = float((bce * Mc).sum() / n_cls)
    d = np.asarray(R_reg, np.float64) - np.asarray(G_rreg, np.float64)
    ad = np.abs(d)
    reg = float((np.where(ad < 1, 0.5 * d * d, ad - 0.5) * Mr[..., None]).sum() / n_reg)
    sig = np.where(x >= 0, 1 / (1 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1 + np.exp(-np.abs(x))))
    return dict(refine_cls_loss=cls, refine_reg_loss=reg, loss=cls + lam * reg, n_cls=int(Mc.sum()), n_reg=int(Mr.sum()),
                dR_cls=(sig - q) * Mc / n_cls, dR_reg=np.clip(d, -1, 1) * Mr[..., None] / n_reg)
