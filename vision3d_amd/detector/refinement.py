"""Refinement head (interface of vision3d/detector/refinement.py:8-50).  Upstream only the MLP forward
is meaningful: `apply_refinements` raises and `forward` splits with `split(1)` on dim 0, which works
only for batch size 2.  The evident intent -- 7 box deltas + 1 confidence on the last
dim -- is what `forward` returns here; `apply_refinements` is defined as the VoxelNet decoding the rest of the
reference uses for every box residual (core/box_encode.py:13-23), with the proposal in the anchor's role.

Training (no upstream counterpart; the definition is this repository's, restated in tests/refine_targets_ref.py):
`encode_refinements` inverts `apply_refinements`, `RefinementLoss` is the stage-2 loss over the targets of
core/refinement_targets.py -- one native pass (csrc/refine_targets.hip) with the torch expressions kept beside it.  With
TRAIN.REFINEMENT_IOU_LOSS enabled the loss gains a rotated 3-D IoU term on the decoded boxes (ops/iou_loss.py, csrc/iou_loss.hip)."""
import math

import torch
import torch.nn.functional as F
from torch import nn

from ..core.box_encode import decode, encode
from ..ops.iou_loss import KINDS as IOU_LOSS_KINDS, iou3d_loss_torch
from .fused_loss import scale_gradient, take_gradient
from .layers import MLP


def encode_refinements(boxes, proposals):
    """(…, 7) boxes + (…, 7) proposals -> residuals that `apply_refinements` turns back into the boxes: components 0-5 of
    core/box_encode.encode, the yaw residual wrapped to [-pi/2, pi/2) (a perfect proposal gets 0, small errors on either side stay
    small; stage 1 keeps upstream's [0, pi) wrap).  The decoded yaw equals the box's modulo pi."""
    out = encode(boxes, proposals)
    out[..., 6] = torch.remainder((boxes[..., 6] - proposals[..., 6]) + math.pi / 2, math.pi) - math.pi / 2
    return out


class RefinementLayer(nn.Module):

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.mlp = self.build_mlp(cfg)

    def build_mlp(self, cfg):
        channels = cfg.REFINEMENT.MLPS + [cfg.BOX_DOF + 1]
        return MLP(channels, bias=True, bn=False, relu=[True, False])

    def apply_refinements(self, box_deltas, boxes):
        """(…, 7) residuals + (…, 7) proposals -> refined boxes: xyz = d * [diag, diag, h] + xyz_p, wlh = exp(d) * wlh_p,
        yaw = d + yaw_p.  Upstream raises (refinement.py:32-33); SURVEY.md 8(f) rank 3 asks for the decode of
        core/box_encode.py, which is what the encode side of refinement_targets.py would invert."""
        return decode(box_deltas, boxes)

    def forward(self, points, features, boxes):
        """features (B, N, C) pooled RoI features -> (box_deltas (B,N,7), scores (B,N,1))."""
        out = self.mlp(features)
        return out.split([self.cfg.BOX_DOF, 1], dim=-1)


def _rows(t, width):
    """(..., width) float32 -> (tensor to read, row stride in floats): views whose rows are evenly spaced (the two halves of the
    head's (B, n, 8) output) are read in place, anything else through a contiguous copy."""
    t = t.detach()
    if t.dim() >= 2 and (width == 1 or t.stride(-1) == 1) and t.stride(-2) >= width \
            and all(t.stride(i) == t.stride(i + 1) * t.shape[i + 1] for i in range(t.dim() - 2)):
        return t, t.stride(-2)
    return t.contiguous(), width


class FusedRefinementLossFunction(torch.autograd.Function):
    """RefinementLoss.forward_torch and its gradient in one native pass (csrc/refine_targets.hip): (R_reg (..., 7), R_cls (..., 1),
    G_conf, G_rreg, M_rcls u8, M_rreg u8) -> (cls_loss, reg_loss); the kernel's (#M_rcls, #M_rreg) stay on the node as
    `loss.grad_fn.counts`.  The gradient is computed with the forward; backward scales it with the upstream gradients."""

    @staticmethod
    def forward(ctx, r_reg, r_cls, g_conf, g_reg, m_cls, m_reg):
        from .. import _lib as L
        rows = g_conf.numel()
        reg, ld_reg = _rows(r_reg, 7)
        cls, ld_cls = _rows(r_cls, 1)
        dev = r_reg.device
        losses = torch.empty(4, dtype=torch.float32, device=dev)
        # both gradients in one buffer [d_cls: rows | d_reg: rows * 7]: backward scales them in one launch
        grad = torch.empty(rows * 8, dtype=torch.float32, device=dev)
        d_cls, d_reg = grad[:rows].view(r_cls.shape), grad[rows:].view(r_reg.shape)
        with L.device_guard(dev):
            L.check(L.lib().v3d_refine_loss_fwd_bwd(L.ptr(reg), ld_reg, L.ptr(cls), ld_cls, L.ptr(g_conf), L.ptr(g_reg), L.ptr(m_cls),
                                                    L.ptr(m_reg), rows, L.ptr(losses), L.ptr(d_reg), L.ptr(d_cls), L.stream_ptr()),
                    "refine_loss_fwd_bwd")
        ctx.grad, ctx.rows, ctx.shapes = grad, rows, (r_cls.shape, r_reg.shape)
        ctx.counts = losses[2:4]  # (#M_rcls, #M_rreg) as the kernel counted them
        return losses[0], losses[1]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_cls_loss, g_reg_loss):
        grad, rows = take_gradient(ctx, "refinement"), ctx.rows
        d_cls, d_reg = grad[:rows].view(ctx.shapes[0]), grad[rows:].view(ctx.shapes[1])
        scale_gradient("refine_loss_scale", grad, (d_reg, d_cls, rows), (g_cls_loss, g_reg_loss))
        return d_reg, d_cls, None, None, None, None


class FusedRefinementIoULossFunction(torch.autograd.Function):
    """The stage-2 IoU term and its gradient in one native pass (csrc/iou_loss.hip): (R_reg (..., 7), proposals (rows, 7), gt (G, 7),
    R_match (rows) i64, M_rreg u8, kind) -> refine_iou_loss; per row the decode against the proposal, the pair term against the
    matched ground truth and the chain rule back through the decode.  The kernel's count of the rows it took stays on the node as
    `loss.grad_fn.counts`.  The gradient is computed with the forward; backward scales it with the upstream gradient."""

    @staticmethod
    def forward(ctx, r_reg, proposals, gt, match, m_reg, kind):
        from .. import _lib as L
        rows = match.numel()
        reg, ld_reg = _rows(r_reg, 7)
        dev = r_reg.device
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        grad = torch.empty(rows * 7, dtype=torch.float32, device=dev)
        with L.device_guard(dev):
            L.check(L.lib().v3d_refine_iou_loss_fwd_bwd(L.ptr(reg), ld_reg, L.ptr(proposals), L.ptr(gt), gt.shape[0], L.ptr(match),
                                                        L.ptr(m_reg), rows, kind, L.ptr(losses), L.ptr(grad), L.stream_ptr()),
                    "refine_iou_loss_fwd_bwd")
        ctx.grad, ctx.rows, ctx.shape = grad, rows, r_reg.shape
        ctx.counts = losses[1:2]  # (#rows counted) as the kernel counted them
        return losses[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_loss):
        grad = take_gradient(ctx, "refinement IoU")
        scale_gradient("refine_iou_loss_scale", grad, (grad, ctx.rows), (g_loss,))
        return grad.view(ctx.shape), None, None, None, None, None


class RefinementLoss(nn.Module):
    """Stage-2 loss over (R_reg, R_cls) and the targets of RefinementTargetAssigner (G_conf, G_rreg, M_rcls, M_rreg):
    refine_cls_loss = sum over M_rcls of BCE-with-logits(R_cls, G_conf) / max(#M_rcls, 1) (PV-RCNN's IoU-guided confidence),
    refine_reg_loss = sum over M_rreg and the 7 components of smooth-L1 (beta 1) / max(#M_rreg, 1),
    loss = refine_cls_loss + TRAIN.LAMBDA * refine_reg_loss.
    With TRAIN.REFINEMENT_IOU_LOSS.ENABLED (the item then also needs proposals, R_match and the ground-truth boxes):
    refine_iou_loss = sum over M_rreg of term(apply_refinements(R_reg, proposals), cat(boxes)[R_match]) / max(#M_rreg, 1), term =
    1 - IoU (KIND "iou") or 1 - IoU + rho2 / c2 ("diou") of ops/iou_loss.py -- rotated 3-D IoU in the true geometry; proposals and
    ground truths are constants, rows whose match is no ground truth are not counted --, and loss gains WEIGHT * refine_iou_loss."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        iou = cfg.TRAIN.get("REFINEMENT_IOU_LOSS") or {}  # (config files written before the term have no such key)
        self.iou_enabled = bool(iou.get("ENABLED", False))
        self.iou_kind, self.iou_weight = iou.get("KIND", "iou"), float(iou.get("WEIGHT", 1.0))
        if self.iou_kind not in IOU_LOSS_KINDS:
            raise ValueError(f"TRAIN.REFINEMENT_IOU_LOSS.KIND must be one of {sorted(IOU_LOSS_KINDS)}, got {self.iou_kind!r}")

    def _result(self, cls_loss, reg_loss, iou_loss=None):
        loss = cls_loss + self.cfg.TRAIN.LAMBDA * reg_loss
        if iou_loss is None:
            return dict(loss=loss, refine_cls_loss=cls_loss, refine_reg_loss=reg_loss)
        return dict(loss=loss + self.iou_weight * iou_loss, refine_cls_loss=cls_loss, refine_reg_loss=reg_loss, refine_iou_loss=iou_loss)

    def _iou_inputs(self, item):
        """-> (proposals (rows, 7), gt (G, 7), R_match (rows) i64), constants on the device of R_reg."""
        missing = [k for k in ("proposals", "R_match", "boxes") if item.get(k) is None]
        if missing:
            raise RuntimeError(f"RefinementLoss: TRAIN.REFINEMENT_IOU_LOSS is enabled but the item has no {', '.join(missing)} "
                               "(run the refinement target assigner on an item that holds the proposals and the ground-truth boxes)")
        R_reg, boxes = item["R_reg"], item["boxes"]
        boxes = [boxes] if torch.is_tensor(boxes) else list(boxes)
        gt = torch.cat([torch.as_tensor(b).to(R_reg.device, torch.float32).reshape(-1, 7) for b in boxes]) if boxes \
            else R_reg.new_zeros((0, 7), dtype=torch.float32)
        proposals = item["proposals"].detach().to(R_reg.device, torch.float32).reshape(-1, 7)
        match = item["R_match"].to(R_reg.device, torch.int64).reshape(-1)
        if proposals.shape[0] != match.numel() or R_reg.numel() != 7 * match.numel():
            raise RuntimeError("RefinementLoss: proposals, R_match and R_reg disagree on the number of RoIs")
        return proposals.contiguous(), gt.contiguous(), match.contiguous()

    def iou_term_torch(self, item):
        """refine_iou_loss op by op in torch (any device / dtype of R_reg): decode, `iou3d_loss_torch`, masked mean.  A row whose
        decoded box is not finite (an overflowing exp) counts with term 1 and passes no gradient, as in the native pass."""
        R_reg, M_rreg = item["R_reg"], item["M_rreg"].ne(0).reshape(-1)
        proposals, gt, match = self._iou_inputs(item)
        proposals, gt, R = proposals.type_as(R_reg), gt.type_as(R_reg), R_reg.reshape(-1, 7)
        counted = M_rreg & (match >= 0) & (match < gt.shape[0])
        zero, one = R.new_zeros(()), R.new_ones(())
        if gt.shape[0] == 0:
            return torch.where(counted[:, None], R, zero).sum() * zero  # no ground truth at all: 0, still a function of R_reg
        target = gt[match.clamp(0, gt.shape[0] - 1)]
        with torch.no_grad():
            use = counted & torch.isfinite(decode(R, proposals)).all(-1)
        pred = decode(torch.where(use[:, None], R, zero), proposals)
        term = torch.where(use, iou3d_loss_torch(pred, target, self.iou_kind), one)
        return torch.where(counted, term, zero).sum() / counted.sum().clamp(min=1).type_as(R)

    def _iou_fused(self, item):
        R_reg, M_rreg = item["R_reg"], item["M_rreg"]
        proposals, gt, match = self._iou_inputs(item)
        as_u8 = lambda m: (m if m.dtype in (torch.bool, torch.uint8) else m.ne(0)).contiguous().view(torch.uint8)
        return FusedRefinementIoULossFunction.apply(R_reg, proposals, gt, match, as_u8(M_rreg.reshape(-1)), IOU_LOSS_KINDS[self.iou_kind])

    def _fused(self, item):
        """The native pass applies to float32 predictions on the GPU with targets in the assigner's layout; else None."""
        R_reg, R_cls, G_conf, G_rreg, M_rcls, M_rreg = (item[k] for k in ("R_reg", "R_cls", "G_conf", "G_rreg", "M_rcls", "M_rreg"))
        lead = tuple(G_conf.shape)
        if not R_reg.is_cuda or R_reg.dtype != torch.float32 or R_cls.dtype != torch.float32 or G_conf.dtype != torch.float32 \
                or G_rreg.dtype != torch.float32 or tuple(R_reg.shape) != lead + (7,) or tuple(G_rreg.shape) != lead + (7,) \
                or tuple(M_rcls.shape) != lead or tuple(M_rreg.shape) != lead or R_cls.numel() != G_conf.numel():
            return None
        if any(t.device != R_reg.device for t in (R_cls, G_conf, G_rreg, M_rcls, M_rreg)):
            return None
        as_u8 = lambda m: (m if m.dtype in (torch.bool, torch.uint8) else m.ne(0)).contiguous().view(torch.uint8)
        cls_loss, reg_loss = FusedRefinementLossFunction.apply(R_reg, R_cls.reshape(lead + (1,)), G_conf.contiguous(),
                                                              G_rreg.contiguous(), as_u8(M_rcls), as_u8(M_rreg))
        return self._result(cls_loss, reg_loss, self._iou_fused(item) if self.iou_enabled else None)

    def forward_torch(self, item):
        """The same loss op by op in torch (any device / dtype): the fallback and the cross-check of the native pass."""
        R_reg, R_cls, G_conf, G_rreg, M_rcls, M_rreg = (item[k] for k in ("R_reg", "R_cls", "G_conf", "G_rreg", "M_rcls", "M_rreg"))
        M_rcls, M_rreg = M_rcls.ne(0), M_rreg.ne(0)
        zero = R_reg.new_zeros(())
        bce = F.binary_cross_entropy_with_logits(R_cls.reshape(G_conf.shape), G_conf.type_as(R_cls), reduction="none")
        cls_loss = torch.where(M_rcls, bce, zero).sum() / M_rcls.sum().clamp(min=1).type_as(R_reg)
        sl1 = F.smooth_l1_loss(R_reg, G_rreg.type_as(R_reg), reduction="none")
        reg_loss = torch.where(M_rreg.unsqueeze(-1), sl1, zero).sum() / M_rreg.sum().clamp(min=1).type_as(R_reg)
        return self._result(cls_loss, reg_loss, self.iou_term_torch(item) if self.iou_enabled else None)

    def forward(self, item):
        fused = self._fused(item)
        return fused if fused is not None else self.forward_torch(item)
