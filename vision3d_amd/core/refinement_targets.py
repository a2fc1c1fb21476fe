"""RoI <-> ground-truth targets of PV-RCNN's second stage.  Upstream's vision3d/core/refinement_targets.py is dead code (it reads
an `anchor['radius']` no config defines and its `forward` raises); the definition is this repository's, restated in
numpy in tests/refine_targets_ref.py.  Per frame, with the RoIs of `PV_RCNN.stage1_proposals` ((n_cls, TOPK) group-major):

  R_iou / R_match  best `ops.box_iou_rotated_3d(roi, gt)` over the frame's ground truths of the RoI's class and the index of the
                   first maximal one in the concatenated ground-truth list; no positive overlap: 0 and -1
  G_conf           clamp((iou - lo) / (hi - lo), 0, 1), [lo, hi] = TRAIN.REFINEMENT_CONF_IOU (PV-RCNN's IoU-guided confidence)
  G_rreg           `encode_refinements(gt, roi)` where iou >= TRAIN.REFINEMENT_REG_IOU and a ground truth is matched, else 0
  M_rcls           sampled RoIs: foreground = iou >= TRAIN.REFINEMENT_FG_IOU; with R = TRAIN.REFINEMENT_ROIS_PER_FRAME and
                   f = TRAIN.REFINEMENT_FG_FRACTION, min(#fg, floor(R f)) foreground and min(#bg, R - that) background RoIs, in
                   each group those with the smallest (draw, index); R <= 0: every RoI
  M_rreg           M_rcls and a box target

`forward` is one launch of csrc/refine_targets.hip (no (n x g) matrix, no host synchronisation); `forward_torch` is the op-by-op
statement (IoU matrix per frame + torch) kept as the on-device cross-check and the path beyond the kernel's staging limits.
"""
import math

import torch
from torch import nn

from .. import _lib as L
from ..ops import box_iou_rotated_3d


class RefinementTargetAssigner(nn.Module):

    MAX_GT, MAX_ROI = 128, 2048  # per frame: what csrc/refine_targets.hip stages in LDS

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        train = cfg.TRAIN  # (read with defaults here: config files written before stage-2 training have none of these keys)
        self.conf_iou = tuple(float(v) for v in train.get("REFINEMENT_CONF_IOU", (0.25, 0.75)))
        self.reg_iou = float(train.get("REFINEMENT_REG_IOU", 0.55))
        self.fg_iou = float(train.get("REFINEMENT_FG_IOU", 0.55))
        self.rois_per_frame = int(train.get("REFINEMENT_ROIS_PER_FRAME", 128))
        self.fg_fraction = float(train.get("REFINEMENT_FG_FRACTION", 0.5))
        if not self.conf_iou[1] > self.conf_iou[0]:
            raise ValueError("TRAIN.REFINEMENT_CONF_IOU must be [lo, hi] with lo < hi")
        self.generator = None  # optional torch.Generator of the sampling draws (as RoiGridPool.generator)

    def fg_quota(self):
        return max(int(math.floor(self.rois_per_frame * self.fg_fraction)), 0)

    def _inputs(self, item):
        proposals = item["proposals"].detach()  # constants here: no gradient flows into stage 1 through the targets
        L.require_gpu("refinement targets", proposals)
        proposals = L.as_f32("refinement targets", proposals)
        if proposals.dim() != 3 or proposals.shape[-1] != 7:
            raise RuntimeError("refinement targets: proposals must be (B, n, 7)")
        dev, (B, n) = proposals.device, proposals.shape[:2]
        proposal_class = item["proposal_class"].to(dev, torch.int64).contiguous()
        boxes, class_idx = item["boxes"], item["class_idx"]
        if torch.is_tensor(boxes):  # one frame handed over without its list
            boxes, class_idx = [boxes], [class_idx]
        if len(boxes) != B or len(class_idx) != B or proposal_class.numel() != n:
            raise RuntimeError("refinement targets: one ground-truth list entry per frame and one class per RoI")
        counts = [int(b.shape[0]) for b in boxes]
        gt = torch.cat([torch.as_tensor(b).to(dev, torch.float32).reshape(-1, 7) for b in boxes])
        gt_class = torch.cat([torch.as_tensor(c).to(dev, torch.int64).reshape(-1) for c in class_idx])
        if gt_class.numel() != gt.shape[0]:
            raise RuntimeError("refinement targets: boxes and class_idx disagree")
        draws = item.get("refine_draws")
        if draws is None:
            draws = torch.rand((B, n), device=dev, generator=self.generator)
        draws = L.as_f32("refinement targets", draws.to(dev))
        if tuple(draws.shape) != (B, n):
            raise RuntimeError("refinement targets: refine_draws must be (B, n)")
        return proposals, proposal_class, gt.contiguous(), gt_class.contiguous(), counts, draws

    def forward(self, item):
        """Fused path: one launch of csrc/refine_targets.hip."""
        proposals, proposal_class, gt, gt_class, counts, draws = self._inputs(item)
        B, n = proposals.shape[:2]
        if n > self.MAX_ROI or max(counts, default=0) > self.MAX_GT:  # beyond the kernel's staging limits
            return self._torch(item, proposals, proposal_class, gt, gt_class, counts, draws)
        dev = proposals.device
        offsets = [0]
        for c in counts:
            offsets.append(offsets[-1] + c)
        offsets = torch.tensor(offsets, dtype=torch.int32).to(dev, non_blocking=True)
        iou = torch.empty((B, n), dtype=torch.float32, device=dev)
        match = torch.empty((B, n), dtype=torch.int64, device=dev)
        conf = torch.empty((B, n), dtype=torch.float32, device=dev)
        G_reg = torch.empty((B, n, 7), dtype=torch.float32, device=dev)
        M_cls = torch.empty((B, n), dtype=torch.bool, device=dev)
        M_reg = torch.empty((B, n), dtype=torch.bool, device=dev)
        with L.device_guard(dev):
            L.check(L.lib().v3d_refine_targets(L.ptr(proposals), L.ptr(proposal_class), B, n, L.ptr(gt), L.ptr(gt_class), L.ptr(offsets),
                                               gt.shape[0], L.ptr(draws), self.conf_iou[0], self.conf_iou[1], self.reg_iou, self.fg_iou,
                                               self.rois_per_frame, self.fg_quota(), L.ptr(iou), L.ptr(match), L.ptr(conf), L.ptr(G_reg),
                                               L.ptr(M_cls), L.ptr(M_reg), L.stream_ptr()), "refine_targets")
        item.update(R_iou=iou, R_match=match, G_conf=conf, G_rreg=G_reg, M_rcls=M_cls, M_rreg=M_reg)
        return item

    def forward_torch(self, item):
        return self._torch(item, *self._inputs(item))

    def _torch(self, item, proposals, proposal_class, gt, gt_class, counts, draws):
        from ..detector.refinement import encode_refinements
        B, n = proposals.shape[:2]
        iou = proposals.new_zeros((B, n))
        match = torch.full((B, n), -1, dtype=torch.int64, device=proposals.device)
        off = 0
        for b, g in enumerate(counts):
            if g:
                m = box_iou_rotated_3d(proposals[b], gt[off:off + g])  # (n, g)
                m = torch.where(gt_class[off:off + g][None, :] == proposal_class[:, None], m, m.new_full((), -1.0))
                best, arg = m.max(dim=1)  # the first maximal ground truth
                ok = best > 0
                iou[b] = torch.where(ok, best, best.new_zeros(()))
                match[b] = torch.where(ok, arg + off, arg.new_full((), -1))
            off += g
        lo, hi = iou.new_tensor(self.conf_iou[0]), iou.new_tensor(self.conf_iou[1])
        conf = ((iou - lo) / (hi - lo)).clamp(0, 1)
        reg = (match >= 0) & (iou >= iou.new_tensor(self.reg_iou))
        G_reg = proposals.new_zeros((B, n, 7))
        if gt.shape[0]:
            enc = encode_refinements(gt[match.clamp(min=0)], proposals)
            G_reg = torch.where(reg.unsqueeze(-1), enc, G_reg)
        R = self.rois_per_frame
        if R <= 0:
            taken = torch.ones((B, n), dtype=torch.bool, device=proposals.device)
        else:
            fg = iou >= iou.new_tensor(self.fg_iou)
            order = torch.argsort(draws, dim=1, stable=True)  # by (draw, index)
            fg_sorted = fg.gather(1, order)
            rank = torch.where(fg_sorted, fg_sorted.cumsum(1), (~fg_sorted).cumsum(1)) - 1  # rank inside the RoI's own group
            n_fg = fg.sum(1).clamp(max=self.fg_quota())
            n_bg = torch.minimum((~fg).sum(1), (R - n_fg).clamp(min=0))
            taken_sorted = rank < torch.where(fg_sorted, n_fg[:, None], n_bg[:, None])
            taken = torch.zeros_like(fg).scatter(1, order, taken_sorted)
        item.update(R_iou=iou, R_match=match, G_conf=conf, G_rreg=G_reg, M_rcls=taken, M_rreg=taken & reg)
        return item
